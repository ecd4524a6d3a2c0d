"""gat(label_input=rate) without a GPU: the package's host Philox (label_mask) against the restated mask of
label_input_ref, the lists the kernels walk, the concatenation identity [X | M onehot(y)] [W ; E] = X W + M E[y] on the three
reference models in fp64, every refusal (which comes before any device work, so None stands in for the context), the ABI,
and the register report of csrc/label_input.hip.  Every test here fails on the code before the feature, from an unknown
keyword or a missing symbol."""
import os
import re
import shutil
import subprocess
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest

import gat_ref
import gatdot_ref
import gatv2_ref
import label_input_ref as li

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the mask and the lists ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [0.0, 0.3, 0.999])
def test_host_count_equals_the_restated_mask(pkg, rate):
    """label_mask.fed_count / fed_mask over T training rows against label_input_ref (dropout_ref's Philox), for several
    epochs and seeds, on small row numbers and on ones above 2^32"""
    lm = import_module(pkg.__name__ + ".label_mask")
    thr = lm.threshold(rate)
    assert thr == li.threshold(rate) == int(np.floor(rate * 2.0 ** 32))
    rng = np.random.default_rng(5)
    small = np.sort(rng.choice(100_000, size=3001, replace=False))
    for rows in (small, small + (1 << 32) + 12345, small.astype(np.uint64) * np.uint64(3_000_000_007)):
        for seed in (0, 7, 0xC0FFEE1234567890):
            for epoch in (0, 1, 2, 1000, (1 << 32) - 1):
                want = li.fed_mask(rows, thr, seed, epoch)
                got = lm.fed_mask(rows, thr, seed, epoch)
                np.testing.assert_array_equal(got, want)
                assert lm.fed_count(rows, thr, seed, epoch) == int(want.sum())
                if rate == 0.0:
                    assert not want.any()
                elif rate == 0.3:
                    assert abs(want.mean() - 0.3) < 0.04         # 3001 draws: 4.8 standard deviations
                else:
                    assert want.mean() > 0.99
    np.testing.assert_array_equal(lm.words(small, 3, 4), li.words(small, 3, 4))
    assert len({int(lm.fed_count(small, lm.threshold(0.3), 1, e)) for e in range(8)}) > 1       # the epoch matters


def test_the_draws_share_no_counter_with_dropout(pkg):
    """the first counter word is 0xFFFFFFFF: a column group that a row of fewer than 2^32 columns never has"""
    lm = import_module(pkg.__name__ + ".label_mask")
    assert lm.COLUMN_GROUP == li.COLUMN_GROUP == 0xFFFFFFFF > ((1 << 32) - 1) >> 2


@pytest.mark.parametrize("rate", [-0.1, 1.0, 1.5, float("nan"), "0.5", None, True])
def test_threshold_refuses(pkg, rate):
    lm = import_module(pkg.__name__ + ".label_mask")
    with pytest.raises(ValueError, match="label_input"):
        lm.threshold(rate)


def test_lists_are_sorted_by_class_then_row(pkg):
    gat = import_module(pkg.__name__ + ".gat")
    rng = np.random.default_rng(2)
    n, C = 500, 7
    S = rng.choice(4, size=n, p=(0.5, 0.2, 0.2, 0.1)).astype(np.int32)
    Y = rng.integers(0, C - 1, size=n).astype(np.int32)                  # class C - 1 is empty
    Y[S != 1] = -5                                                         # labels outside the training rows are not read
    for a, b in zip(gat.label_lists(S.reshape(-1, 1), Y.reshape(-1, 1), 1, C), li.lists(S, Y, 1, C)):
        assert a.dtype == np.int32
        np.testing.assert_array_equal(a, b)
    rows, cls, cls_ptr = gat.label_lists(S, Y, 1, C)
    assert cls_ptr[0] == 0 and cls_ptr[-1] == rows.size == int((S == 1).sum()) and cls_ptr[C - 1] == cls_ptr[C]
    assert len(set(rows.tolist())) == rows.size
    key = cls.astype(np.int64) * n + rows
    assert (np.diff(key) > 0).all()
    Y[np.flatnonzero(S == 1)[3]] = C
    with pytest.raises(ValueError, match="label_input.*outside"):
        gat.label_lists(S, Y, 1, C)


# ---- the concatenation identity ----------------------------------------------------------------------------------------------------------
MODELS = {"v1": (gat_ref.oracle_gat, 1), "v2": (gatv2_ref.oracle_gatv2, 2), "dot": (gatdot_ref.oracle_gatdot, 3)}
# The two sides differ by ONE fp32 rounding of layer 0's Z: fp32(fp32(X W + b) + E[y]) against fp32(X W + E[y] + b) with the
# sums accumulated exactly (Linear(f64acc=True)) and the attention in fp64 -- 2^-24 relative in Z.  Everything after Z is the
# same function on both sides; two layers of attention, the loss and a backward pass are allowed to amplify that 160 times.
IDENTITY_TOL = 1e-5


@pytest.mark.parametrize("variant", ["v1", "v2", "dot"])
@pytest.mark.parametrize("feed_all", [False, True])
def test_the_label_input_is_the_augmented_model(oracle, variant, feed_all):
    """loss, every G_W and G_b, and G_E against the rows of the augmented model's first G_W"""
    n, C, sizes, heads = 160, 5, [16, 32, 5], [4, 1]
    ip, ix, dv, Y = li.planted_partition(n, C, 5, 0.6, seed=3)
    rng = np.random.default_rng(1)
    X = rng.standard_normal((n, sizes[0]), dtype=np.float32)
    S = rng.choice(4, size=n, p=(0.6, 0.15, 0.2, 0.05)).astype(np.int32)
    M, S_e = li.epoch_sets(S, 0, li.threshold(0.5), seed=9, epoch=2, feed_all=feed_all)
    assert M.any() and (feed_all or (S_e == 0).any())
    keep = (S_e == 0) if not feed_all else (S == 1)          # a plain forward has no training loss: any rows will do
    cls, zf = MODELS[variant]
    E = (rng.standard_normal((C, zf * sizes[1])) * 0.3).astype(np.float32)

    def build(sz):
        O = cls(oracle, oracle.Csr(ip.copy(), ix.copy(), dv.copy(), n), sz, heads, loss=li.split_loss(oracle, Y, keep),
                dtype=np.float64)
        for L in O.layers:
            L.lin.f64acc = True
        return O
    plain, aug = build(sizes), build([sizes[0] + C] + sizes[1:])
    W = (rng.standard_normal(plain.layers[0].lin.W.shape) * 0.2).astype(np.float32)
    plain.layers[0].lin.W = W
    aug.layers[0].lin.W = np.ascontiguousarray(np.concatenate([W, E], axis=0))
    wrap = li.oracle_label_input(plain, E, Y, M)
    res_p = plain.train_forward(X, Y)
    plain.backward()
    res_a = aug.train_forward(li.augmented_features(X, Y, M, C), Y)
    aug.backward()
    print(f"[label-input] {variant} feed_all={feed_all}: loss {res_p[0]!r} / augmented {res_a[0]!r}")
    assert abs(res_p[0] - res_a[0]) <= IDENTITY_TOL * abs(res_a[0]) and res_p[1] == res_a[1]
    F = sizes[0]
    pairs = [("G_W0", plain.layers[0].lin.G_W, aug.layers[0].lin.G_W[:F]), ("G_E", wrap.G_E, aug.layers[0].lin.G_W[F:]),
             ("G_b0", plain.layers[0].lin.G_b, aug.layers[0].lin.G_b), ("G_W1", plain.layers[1].lin.G_W, aug.layers[1].lin.G_W)]
    for name, a, b in pairs:
        d = gat_ref.relerr(a, b)
        print(f"[label-input] {variant} feed_all={feed_all} {name}: {d:.3e}")
        assert np.abs(b).max() > 0 and d <= IDENTITY_TOL, (name, d)
    # and the bar can see a wrong table: with E = 0 on the plain side the loss is far outside it
    wrap.E[:] = 0
    off = plain.train_forward(X, Y)[0]
    assert abs(off - res_a[0]) > 100 * IDENTITY_TOL * abs(res_a[0]), (off, res_a[0])


def test_the_learning_fixture_separates_the_two_models(oracle):
    """the reference alone, here on the CPU: without label inputs the noise features leave the validation accuracy far below
    what label_input=0.5 reaches, the recorded figures are the measured ones, and the device test's two bars lie inside
    the gap with room on both sides"""
    got = {"plain": li.reference_learning(oracle, False), "label": li.reference_learning(oracle, True)}
    print(f"[label-input] reference validation accuracy: {got}")
    for k, v in got.items():
        assert abs(v - li.LEARN_REFERENCE[k]) <= 0.02, (k, v)
    assert li.LEARN_REFERENCE["plain"] + 0.15 <= li.LEARN_BARS["plain"] < li.LEARN_BARS["label"] <= li.LEARN_REFERENCE["label"] - 0.15


# ---- refusals, before any device work --------------------------------------------------------------------------------------------------
def _tiny(pkg, n=8):
    return pkg.csr_matrix(np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32), np.ones(n, dtype=np.float32), n)


class _Sets:
    """a stand-in for the int32 dn_matrix of the sets: host memory only"""
    def __init__(self, s): self.s = np.asarray(s, dtype=np.int32).reshape(-1, 1)
    def numpy(self): return self.s
    def n(self): return self.s.shape[0]


def _stand_in(pkg, n=8, C=5, splits=True, **options):
    """a gat object without a device whose label owner must never be reached"""
    gat = import_module(pkg.__name__ + ".gat")
    G = gat.gat.__new__(gat.gat)
    G.variant, G.loss, G.sizes, G.A = "v1", "softmax", [16, 32, C], _tiny(pkg, n)
    G.layers_, G.heads = [], [4, 1]
    G._label_threshold = li.threshold(0.5)
    G.label_input_p = 0.5

    def unreachable(*a, **k):
        raise AssertionError("the device must not be reached")
    G.label = SimpleNamespace(rows=None, set_lists=unreachable, __call__=unreachable)
    S = _Sets([0, 0, 0, 1, 1, 2, 2, 3][:n]) if splits else None
    G.loss_layer = SimpleNamespace(S=S, counts=[3, 2, 2, 1] if splits else None, train_set=0)
    for k, v in options.items():
        setattr(G, k, v)
    return gat, G


def test_constructor_refusals_need_no_gpu(pkg):
    """fails on the code before the feature with TypeError: gat() takes no label_input="""
    A = _tiny(pkg)
    for rate in (-0.25, 1.0, 2, float("nan"), "half"):
        with pytest.raises(ValueError, match="label_input"):
            pkg.gat(A, [16, 32, 5], label_input=rate)
    with pytest.raises(ValueError, match="label_input.*bce"):
        pkg.gat(A, [16, 32, 5], loss="bce", label_input=0.5)
    with pytest.raises(ValueError, match="label_input supports at most 256 classes"):
        pkg.gat(A, [16, 32, 257], label_input=0.5, variant="dot")
    with pytest.raises(ValueError, match="label_weights needs label_input"):
        pkg.gat(A, [16, 32, 5], label_weights=np.zeros((5, 32), dtype=np.float32))
    assert pkg.ops.LABEL_INPUT_MAX_CLASSES == 256 and pkg.ops.LABEL_INPUT_MAX_WIDTH == 3 * pkg.ops.GAT_MAX_WIDTH
    gat = import_module(pkg.__name__ + ".gat")
    assert "label_input" in pkg.__all__ and pkg.label_input is gat.label_input
    assert gat.label_input.params_table == (("label", "E", "G_E", "m", "v", True),) and gat.label_input.adam_fused


def test_set_label_input_refusals_need_no_gpu(pkg):
    Y = np.array([0, 1, 2, 3, 4, 0, 1, 2], dtype=np.int32)
    _, G = _stand_in(pkg, splits=False)
    with pytest.raises(ValueError, match="label_input.*set_splits"):
        G.set_label_input(Y)
    _, G = _stand_in(pkg)
    for rate in (-0.5, 1.0, float("nan")):
        with pytest.raises(ValueError, match="label_input"):
            G.set_label_input(Y, rate=rate)
    bad = Y.copy()
    bad[1] = 5                                              # a training row (set 0) with a label outside [0, 5)
    with pytest.raises(ValueError, match="label_input.*training row 1 has label 5"):
        G.set_label_input(bad)
    bad[1], bad[7] = 1, 99                                  # row 7 trains nothing: its label is not read ...
    with pytest.raises(AssertionError, match="device must not be reached"):
        G.set_label_input(bad)                              # ... and the call gets as far as the upload
    with pytest.raises(ValueError, match="label_input: Y must hold 8 integer labels"):
        G.set_label_input(Y[:7])
    with pytest.raises(ValueError, match="label_input: Y must hold 8 integer labels"):
        G.set_label_input(Y.astype(np.float32))
    assert G._label_Y is None and G.label_epoch == 0        # nothing was stored
    _, G = _stand_in(pkg, label=None, label_input_p=0.0)
    with pytest.raises(ValueError, match="label_input"):
        G.set_label_input(Y)


def test_a_forward_before_set_label_input_is_refused(pkg):
    _, G = _stand_in(pkg)
    for training in (False, True):
        with pytest.raises(ValueError, match="label_input.*set_label_input"):
            G(None, None, training=training)
    with pytest.raises(ValueError, match="label_input.*set_label_input"):
        G.predict(None, None)
    assert G.label_epoch == 0


def test_an_epoch_that_feeds_every_row_is_refused_before_the_launch(pkg):
    """three training rows at rate 0.999: training forward 0 of seed 0 feeds all three"""
    _, G = _stand_in(pkg)
    G.label = SimpleNamespace(rows=object(), S_e=object())
    G._label_splits = (G.loss_layer.S, [3, 2, 2, 1], 0)
    G._label_rows = np.array([0, 1, 2], dtype=np.uint64)
    G._label_threshold, G.label_seed, G.label_epoch = li.threshold(0.999), 0, 0
    assert li.fed_mask(G._label_rows, G._label_threshold, 0, 0).all()
    with pytest.raises(ValueError, match="label_input.*none is left to predict"):
        G(None, None, training=True)
    assert G.label_epoch == 0 and G.loss_layer.counts == [3, 2, 2, 1]


def test_checkpoints_are_refused_and_create_no_file(pkg, tmp_path):
    """save, load and the selector's save_best raise ValueError naming the option with None in the place of the context;
    nothing is written, read or created"""
    _, G = _stand_in(pkg)
    path = tmp_path / "model.ckpt"
    for call in (lambda: G.save(None, str(path)), lambda: G.load(None, str(path)),
                 lambda: G._write_checkpoint(None, str(path), {}, False, 0)):
        with pytest.raises(ValueError, match="label_input"):
            call()
    _, G = _stand_in(pkg, label_input_p=0.0)                 # set_label_input(rate=0) leaves the table in place
    with pytest.raises(ValueError, match="label_input"):
        G.save(None, str(path))
    assert not path.exists() and not list(tmp_path.iterdir())
    gat = import_module(pkg.__name__ + ".gat")
    gat.refuse_checkpoint(gat.gat.__new__(gat.gat), "save")  # a model without the option is not refused


def test_dist_gat_does_not_take_the_options(pkg):
    dist = import_module(pkg.__name__ + ".dist")
    for option in ("label_input", "label_weights"):
        with pytest.raises(TypeError, match=option):
            dist.dist_gat(None, None, None, [16, 32, 5], **{option: None})


def test_parameter_names(pkg):
    """the table is label0 in the checkpoint's naming (what model_selector snapshots), last among layer 0's owners, and a
    layer without it lists what it listed"""
    gat = import_module(pkg.__name__ + ".gat")
    gcn = import_module(pkg.__name__ + ".gcn")
    checkpoint = import_module(pkg.__name__ + ".checkpoint")
    new = lambda c: c.__new__(c)
    layers = [gat.gatdot_layer.__new__(gat.gatdot_layer) for _ in range(2)]
    for l in layers:
        l.lin, l.attn = new(gcn.linear), new(gat.attention_dot)
    layers[0].label = new(gat.label_input)
    assert layers[0].params() == [layers[0].lin, layers[0].label] and layers[1].params() == [layers[1].lin]
    names = [name for name, *_ in checkpoint.model_params(type("m", (), {"layers_": layers})())]
    assert names == ["W0", "b0", "label0", "W1", "b1"]
    o = layers[0].label
    o.E, o.G_E, o.m, o.v = (object() for _ in range(4))
    assert o.adam_tensors(5e-4) == [(o.E, o.G_E, o.m, o.v, 5e-4)]            # decays like W


# ---- the ABI and the wrappers ------------------------------------------------------------------------------------------------------------
def test_abi_and_prototypes(pkg):
    lib = pkg._lib.load()
    header = open(os.path.join(ROOT, "include", "mggcn.h")).read()
    for name, nargs in (("mggcn_label_input_forward_f32", 19), ("mggcn_label_input_backward_f32", 17)):
        assert name in pkg._lib.PROTOTYPES and len(pkg._lib.PROTOTYPES[name][1]) == nargs
        assert hasattr(lib, name) and re.search(r"\bvoid %s\(" % name, header)
        decl = re.search(r"void %s\((.*?)\);" % name, header, flags=re.S).group(1)
        assert decl.count(",") + 1 == nargs
    assert "#define MGGCN_LABEL_INPUT_MAX_CLASSES 256u" in header and "#define MGGCN_LABEL_INPUT_MAX_WIDTH 3072u" in header


def test_ops_refuse_bad_shapes_before_the_library(pkg):
    """the wrappers raise ValueError on stand-ins that own no device memory"""
    class M:
        def __init__(self, n, m): self.N, self.Mm = n, m
        def n(self): return self.N
        def m(self): return self.Mm
        def size(self): return self.N * self.Mm
        def shape(self): return (self.N, self.Mm)
        def buffer(self): raise AssertionError("the library must not be reached")
    ops = pkg.ops
    rows, cls, ptr, E, Z, S = M(10, 1), M(10, 1), M(6, 1), M(5, 32), M(20, 32), M(20, 1)
    fwd = lambda **k: ops.label_input_forward(None, k.get("rows", rows), k.get("cls", cls), k.get("E", E), k.get("Z", Z),
                                              k.get("threshold", 7), False, 0, 0, k.get("row0", 0), k.get("kept_set", 0), 3,
                                              k.get("S", S))
    bwd = lambda **k: ops.label_input_backward(None, k.get("rows", rows), k.get("cls", cls), k.get("ptr", ptr), k.get("Z", Z),
                                               k.get("E", E), k.get("threshold", 7), False, 0, 0, k.get("row0", 0))
    for call in (fwd, bwd):
        with pytest.raises(ValueError, match="1 <= classes <= 256"):
            call(E=M(257, 32))
        with pytest.raises(ValueError, match="1 <= width <= 3072"):
            call(E=M(5, 3073), Z=M(20, 3073))
        with pytest.raises(ValueError, match="the table has 32 columns, the rows 33"):
            call(Z=M(20, 33))
        with pytest.raises(ValueError, match="rows and cls must both be 10 x 1"):
            call(cls=M(9, 1))
        with pytest.raises(ValueError, match="21 listed rows, the matrix has 20"):
            call(rows=M(21, 1), cls=M(21, 1))
        for threshold in (-1, 1 << 32, 0.5):
            with pytest.raises(ValueError, match="threshold must be a uint32"):
                call(threshold=threshold)
        with pytest.raises(ValueError, match="row0 must not be negative"):
            call(row0=-1)
    with pytest.raises(ValueError, match="S_out must be 20 x 1"):
        fwd(S=M(19, 1))
    with pytest.raises(ValueError, match="kept_set must be one of"):
        fwd(kept_set=3)
    with pytest.raises(ValueError, match="cls_ptr must be 6 x 1"):
        bwd(ptr=M(5, 1))


def test_no_instantiation_uses_scratch(tmp_path):
    """csrc/label_input.hip compiled for gfx950 to assembly: the resource metadata of every kernel in it -- the forward and
    the backward on the float4 and the element path, the final pass by segment (and the unused column-sum final that
    reduce.h brings along) -- reports a private segment of zero bytes and zero spilled vector registers"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path / "label_input.s"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-S",
                        "--cuda-device-only", os.path.join(ROOT, "mg-gcn_amd", "csrc", "label_input.hip"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels"):]
    seen = {}
    for b in re.split(r"\n\s*- \.agpr_count:", "\n" + meta)[1:]:
        blk = ".agpr_count:" + b
        nm = re.search(r"\.name:\s+(\S+)", blk)
        if not nm:
            continue
        field = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                 for k in ("private_segment_fixed_size", "vgpr_spill_count", "vgpr_count", "group_segment_fixed_size")}
        seen[nm.group(1)] = field
        print(f"[label-input] {nm.group(1)}: {field}")
        assert field["private_segment_fixed_size"] == 0 and field["vgpr_spill_count"] == 0, (nm.group(1), field)
    for kernel, count in (("label_input_forward_kernel", 2), ("label_input_backward_kernel", 2), ("segsum_final_kernel", 1)):
        assert sum(kernel in k for k in seen) == count, (kernel, sorted(seen))
    assert len(seen) == 6, sorted(seen)
