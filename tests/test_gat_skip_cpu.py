"""The host references of the gat-skip tests, checked without a GPU: the fp64 restatement (gat_skip_ref.restate64) against
torch's autograd in fp64, the fp32 twin against the restatement, the bar of every output by the project's rule and what that
bar must be able to tell apart, the refusals of gat(skip=, norm=) and of the ops wrappers (which come before any device
work), the names the generic parameter readers give the new tensors, and the register report of csrc/gated_skip.hip."""
import os
import re
import shutil
import subprocess
from importlib import import_module

import numpy as np
import pytest

import gat_ref as ref
import gat_skip_ref as gs
import layernorm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _autograd(o, r, w, G, norm=None, leaky=False):
    """y, the gradients of o, r and w (and gamma, beta) of y = [lrelu][layer_norm](skip(o, r, w)) by torch in fp64"""
    import torch
    to, tr = (torch.tensor(M, dtype=torch.float64, requires_grad=True) for M in (o, r))
    leaves = [to, tr]
    if w is None:
        y = to + tr
    else:
        tw = torch.tensor(w, dtype=torch.float64, requires_grad=True)
        leaves.append(tw)
        s = (tw[0] * to + tw[1] * tr + tw[2] * (to - tr)).sum(dim=1, keepdim=True)
        g = torch.sigmoid(s)
        y = g * tr + (1 - g) * to
    if norm is not None:
        gamma, beta = (torch.tensor(p, dtype=torch.float64, requires_grad=True) for p in norm)
        leaves += [gamma, beta]
        y = torch.nn.functional.layer_norm(y, (o.shape[1],), gamma.view(-1), beta.view(-1), layernorm_ref.EPS)
    if leaky:
        y = torch.nn.functional.leaky_relu(y, gs.SLOPE)
    y.backward(torch.tensor(G, dtype=torch.float64))
    return [y.detach().numpy()] + [t.grad.numpy() for t in leaves]


@pytest.mark.parametrize("n,m", [(37, 41), (37, 128), (5, 1023)])
@pytest.mark.parametrize("mode", ["add", "gate", "gate+norm+activation"])
def test_restatement_matches_autograd(n, m, mode):
    """y, G_o, G_r and G_w of the fp64 restatement (behind layernorm_ref's norm and the activation in the third mode, the
    way a layer chains them) against torch CPU autograd in fp64: <= 1e-10"""
    o, r, G, w = gs.inputs(n, m)
    w = None if mode == "add" else w
    if mode == "gate+norm+activation":
        gamma, beta = layernorm_ref.params(m, 7)
        f = gs.restate64(o, r, w, exact=True)
        y, _, _ = layernorm_ref.forward64(f["y"], gamma, beta, leaky=True, exact=True)
        T, G_gamma, G_beta = layernorm_ref.backward64(G, y, f["y"], gamma, leaky=True, exact=True)
        b = gs.restate64(o, r, w, G=T, exact=True)
        want = _autograd(o, r, w, G, norm=(gamma, beta), leaky=True)
        got = [y, b["G_o"], b["G_r"], b["G_w"], G_gamma, G_beta]
    else:
        b = gs.restate64(o, r, w, G=G, exact=True)
        want = _autograd(o, r, w, G)
        got = [b["y"], b["G_o"], b["G_r"]] + ([] if w is None else [b["G_w"]])
    assert len(got) == len(want)
    for k, (a, t) in enumerate(zip(got, want)):
        d = ref.relerr(a, t)
        print(f"[gat-skip] restatement against autograd n={n} m={m} {mode} output {k}: {d:.3e}")
        assert d <= 1e-10, (mode, k, d)


def test_the_sigmoid_saturates_without_nan():
    for T in (np.float32, np.float64):
        s = np.array([-1e30, -200.0, -104.0, 0.0, 17.0, 200.0, 1e30], dtype=T)
        with np.errstate(under="ignore"):
            g = gs.sigmoid(s)
        assert np.isfinite(g).all() and g[3] == 0.5 and g[0] == 0 and g[-1] == 1 and g[-2] == 1
        assert T is np.float64 or (g[1] == 0 and g[4] == 1)


def _worst_twin():
    worst = dict.fromkeys(gs.FWD_NAMES + gs.BWD_NAMES, (0.0, None))
    for n, m, flags in gs.cases():
        c = gs.case(n, m, flags)
        for what, d in gs.distances(c["twin"], c).items():
            if d > worst[what][0]:
                worst[what] = (d, (n, m, flags))
    return worst


def test_the_bars_follow_the_rule():
    """per output: ROW_TOL where the fp32 twin's worst row-scaled distance from the exact restatement over every case the
    device runs stays within ROW_TOL / 8, eight times the twin's worst otherwise -- gat_skip_ref.BAR, fixed here before any
    device run -- and the recorded twin figures are the ones measured"""
    worst = _worst_twin()
    print("[gat-skip] worst row-scaled twin distance per output: " +
          ", ".join(f"{k} {d:.2e} at {where}" for k, (d, where) in worst.items()))
    for what, (d, where) in worst.items():
        assert np.isfinite(d), (what, where)
        assert gs.BAR[what] == pytest.approx(gs.bar_rule(d), rel=0.05), (what, d, where)
        assert d == pytest.approx(gs.TWIN_MEASURED[what], rel=0.05), (what, d)


def test_the_bar_tells_a_wrong_formula_apart():
    """the three mutations of the restatement -- the wrong sign on w[2], g in place of 1 - g in G_o, the last row left out
    of G_w -- each exceed the bar of the output they spoil on at least one case"""
    for mutation, spoiled in gs.MUTATIONS.items():
        worst = 0.0
        for n, m in ((37, 41), (37, 128), (37, 1024)):
            c = gs.case(n, m, gs.GATE | gs.LEAKY)
            r = gs.restate64(c["o"], c["r"], c["w"], True, G=c["G"], act=c["act"], gate=c["gate"], exact=True, mutate=mutation)
            worst = max(worst, gs.distances(r, c)[spoiled] / gs.BAR[spoiled])
        print(f"[gat-skip] mutation {mutation!r}: {spoiled} moves by {worst:.1f} bars")
        assert worst > 1, (mutation, spoiled, worst)


def test_every_instantiation_has_a_width():
    seen = {gs.instantiation(m, v) for m, v in gs.INSTANTIATION_WIDTHS}
    assert len(seen) == 13
    assert {gs.instantiation(m, m % 4 == 0) for m in gs.WIDTHS} | {gs.instantiation(m, False) for m in gs.WIDTHS} == seen
    assert max(gs.rows_per_pass(i) * m for m, v in gs.INSTANTIATION_WIDTHS for i in [gs.instantiation(m, v)]) <= 4200 * 1024


# ---- refusals, before any device work ------------------------------------------------------------------------------------------------------
def _tiny(pkg, n=8):
    return pkg.csr_matrix(np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32), np.ones(n, dtype=np.float32), n)


def _stand_in(pkg, **options):
    """a gat object without a device, as test_gatdot_cpu.py builds its own"""
    gat = import_module(pkg.__name__ + ".gat")
    G = gat.gat.__new__(gat.gat)
    G.variant, G._dropout_layers, G.attn_dropout_p, G._attn_dropout_params = "v1", 2, 0.0, None
    G.dropout_p, G.dropout_seed, G.dropout_epoch = 0.0, 0, 0
    G.layers_, G.heads = [], [4, 1]
    for k, v in options.items():
        setattr(G, k, v)
    return gat, G


def test_constructor_refusals_need_no_gpu(pkg):
    """fails on the code before the feature with TypeError: gat() takes no skip="""
    A = _tiny(pkg)
    with pytest.raises(ValueError, match="skip must be one of"):
        pkg.gat(A, [16, 32, 5], skip="sum")
    with pytest.raises(ValueError, match="skip must be one of"):
        pkg.gat(A, [16, 32, 5], skip=True, variant="dot")
    with pytest.raises(ValueError, match="norm must be one of"):
        pkg.gat(A, [16, 32, 5], norm="batch")
    with pytest.raises(ValueError, match="skip_weights needs skip"):
        pkg.gat(A, [16, 32, 5], skip_weights=[(None, None)] * 2)
    with pytest.raises(ValueError, match="skip_weights lists 1 layers"):
        pkg.gat(A, [16, 32, 5], skip="add", skip_weights=[(None, None)])
    with pytest.raises(ValueError, match=r'skip="add" takes \(W_r, b_r\)'):
        pkg.gat(A, [16, 32, 5], skip="add", skip_weights=[(None, None, None)] * 2)
    with pytest.raises(ValueError, match="w_gate"):
        pkg.gat(A, [16, 32, 5], skip="gate", skip_weights=[(None,)] * 2)
    gat = import_module(pkg.__name__ + ".gat")
    assert gat.SKIPS == (None, "add", "gate") and [gat.check_skip(s) for s in gat.SKIPS] == list(gat.SKIPS)
    assert "gated_skip" in pkg.__all__ and pkg.gated_skip is gat.gated_skip


def test_dist_gat_does_not_take_the_options(pkg):
    dist = import_module(pkg.__name__ + ".dist")
    for option in ("skip", "norm", "skip_weights"):
        with pytest.raises(TypeError, match=option):
            dist.dist_gat(None, None, None, [16, 32, 5], **{option: None})


@pytest.mark.parametrize("options", [dict(skip="add"), dict(skip="gate"), dict(norm="layer"), dict(skip="gate", norm="layer")])
def test_checkpoints_are_refused_and_create_no_file(pkg, tmp_path, options):
    """save, load and the selector's save_best raise ValueError naming the option with None in the place of the context;
    nothing is written, read or created"""
    _, G = _stand_in(pkg, **options)
    name = "skip" if "skip" in options else "norm"
    path = tmp_path / "model.ckpt"
    with pytest.raises(ValueError, match=name):
        G.save(None, str(path))
    with pytest.raises(ValueError, match=name):
        G.load(None, str(path))                            # refused before the (missing) file is opened
    with pytest.raises(ValueError, match=name):
        G._write_checkpoint(None, str(path), {}, False, 0)
    assert not path.exists() and not list(tmp_path.iterdir())


def test_stand_ins_without_the_options_behave_as_before(pkg, tmp_path):
    """an object built with __new__ has neither attribute: set_dropout works, and save gets past the refusals (to the
    context it was not given)"""
    _, G = _stand_in(pkg)
    G.set_dropout(0.5, seed=3, epoch=1)
    assert (G.dropout_p, G.dropout_seed, G.dropout_epoch) == (0.5, 3, 1)
    with pytest.raises(AttributeError):
        G.save(None, str(tmp_path / "model.ckpt"))
    assert not list(tmp_path.iterdir())


def test_parameter_names_of_a_stand_in_layer(pkg):
    """checkpoint.model_params names a full layer W0, b0, att0, res_W0, res_b0, gate0, gamma0, beta0, params() lists the
    owners in the same order, and a layer without the attributes is what it was"""
    gat = import_module(pkg.__name__ + ".gat")
    gcn = import_module(pkg.__name__ + ".gcn")
    checkpoint = import_module(pkg.__name__ + ".checkpoint")
    new = lambda cls: cls.__new__(cls)                      # the real owner classes carry the tables; none has a tensor
    layer = gat.gat_layer.__new__(gat.gat_layer)
    layer.lin, layer.attn = new(gcn.linear), new(gat.attention)
    assert layer.params() == [layer.lin, layer.attn]
    model = type("m", (), {"layers_": [layer]})()
    assert [name for name, *_ in checkpoint.model_params(model)] == ["W0", "b0", "att0"]
    layer.res_lin, layer.gate, layer.norm = new(gcn.linear), new(gat.gated_skip), new(gcn.layer_norm)
    assert layer.params() == [layer.lin, layer.attn, layer.res_lin, layer.gate, layer.norm]
    rows = checkpoint.model_params(model)
    assert [name for name, *_ in rows] == ["W0", "b0", "att0", "res_W0", "res_b0", "gate0", "gamma0", "beta0"]
    assert rows[5] == ("gate0", layer.gate, "w", "m", "v") and rows[3][1] is layer.res_lin and rows[6][1] is layer.norm
    layer.gate = None                                       # skip="add"
    assert [name for name, *_ in checkpoint.model_params(model)] == ["W0", "b0", "att0", "res_W0", "res_b0", "gamma0", "beta0"]
    dotl = gat.gatdot_layer.__new__(gat.gatdot_layer)
    dotl.lin, dotl.attn = new(gcn.linear), gat.attention_dot.__new__(gat.attention_dot)
    assert dotl.params() == [dotl.lin]
    dotl.res_lin, dotl.gate, dotl.norm = new(gcn.linear), new(gat.gated_skip), None
    assert dotl.params() == [dotl.lin, dotl.res_lin, dotl.gate]


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
    assert (ops.GATED_SKIP_GATE, ops.GATED_SKIP_LEAKY_RELU, ops.GATED_SKIP_MAX_WIDTH) == (1, 2, 1024)
    o, r, y, w, g = M(8, 32), M(8, 32), M(8, 32), M(3, 32), M(8, 1)
    with pytest.raises(ValueError, match="1 <= m <= 1024"):
        ops.gated_skip(None, M(8, 1025), M(8, 1025), None, M(8, 1025), None, 0)
    with pytest.raises(ValueError, match="unknown flags"):
        ops.gated_skip(None, o, r, None, y, None, 4)
    with pytest.raises(ValueError, match="r and y must have o's shape"):
        ops.gated_skip(None, o, M(8, 31), None, y, None, 0)
    with pytest.raises(ValueError, match="r and y must have o's shape"):
        ops.gated_skip(None, o, r, None, M(7, 32), None, 0)
    with pytest.raises(ValueError, match="y must not be o or r"):
        ops.gated_skip(None, o, r, None, o, None, 0)
    with pytest.raises(ValueError, match="y must not be o or r"):
        ops.gated_skip(None, o, r, w, r, g, ops.GATED_SKIP_GATE)
    with pytest.raises(ValueError, match="w must be 3 x 32"):
        ops.gated_skip(None, o, r, M(2, 32), y, g, ops.GATED_SKIP_GATE)
    with pytest.raises(ValueError, match="w must be 3 x 32"):
        ops.gated_skip(None, o, r, None, y, g, ops.GATED_SKIP_GATE)
    with pytest.raises(ValueError, match="gate must hold 8 floats"):
        ops.gated_skip(None, o, r, w, y, M(7, 1), ops.GATED_SKIP_GATE)
    with pytest.raises(ValueError, match="w and gate need GATED_SKIP_GATE"):
        ops.gated_skip(None, o, r, w, y, g, 0)
    G, act, G_o, G_r, G_w = M(8, 32), M(8, 32), M(8, 32), M(8, 32), M(3, 32)
    gate = ops.GATED_SKIP_GATE
    with pytest.raises(ValueError, match="G_o and G_r must have G's shape"):
        ops.gated_skip_backward(None, G, None, None, None, None, None, M(8, 31), G_r, None, 0)
    with pytest.raises(ValueError, match="act must have G's shape"):
        ops.gated_skip_backward(None, G, None, None, None, None, None, G_o, G_r, None, ops.GATED_SKIP_LEAKY_RELU)
    with pytest.raises(ValueError, match="G_w needs GATED_SKIP_GATE"):
        ops.gated_skip_backward(None, G, None, None, None, None, None, G_o, G_r, G_w, 0)
    with pytest.raises(ValueError, match="GATED_SKIP_GATE needs o"):
        ops.gated_skip_backward(None, G, None, None, r, w, g, G_o, G_r, G_w, gate)
    with pytest.raises(ValueError, match="o must have G's shape"):
        ops.gated_skip_backward(None, G, None, M(9, 32), M(9, 32), w, M(9, 1), G_o, G_r, G_w, gate)
    with pytest.raises(ValueError, match="G_w must be 3 x 32"):
        ops.gated_skip_backward(None, G, None, o, r, w, g, G_o, G_r, M(2, 32), gate)
    with pytest.raises(ValueError, match="G_r must be a matrix of its own"):
        ops.gated_skip_backward(None, G, None, o, r, w, g, G_o, G_o, G_w, gate)
    with pytest.raises(ValueError, match="G_r must be a matrix of its own"):
        ops.gated_skip_backward(None, G, None, o, r, w, g, G_o, G, G_w, gate)
    with pytest.raises(ValueError, match="G_o must not be o or r"):
        ops.gated_skip_backward(None, G, None, o, r, w, g, o, G_r, G_w, gate)


def test_no_instantiation_uses_scratch(tmp_path):
    """csrc/gated_skip.hip compiled for gfx950 to assembly: the resource metadata of every kernel in it reports a private
    segment of zero bytes and zero spilled vector registers -- the 52 instantiations of the pair (thirteen (V, L, K, R), with
    and without the gate) and the final pass of the column sums"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path / "gated_skip.s"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-S",
                        "--cuda-device-only", os.path.join(ROOT, "mg-gcn_amd", "csrc", "gated_skip.hip"), "-o", str(out)],
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
                 for k in ("private_segment_fixed_size", "vgpr_spill_count", "vgpr_count", "agpr_count", "group_segment_fixed_size")}
        seen[nm.group(1)] = field
        print(f"[gat-skip] {nm.group(1)}: {field}")
        assert field["private_segment_fixed_size"] == 0 and field["vgpr_spill_count"] == 0, (nm.group(1), field)
    for kernel in ("gated_skip_forward_kernel", "gated_skip_backward_kernel"):
        assert sum(kernel in k for k in seen) == 26, (kernel, sorted(seen))
    assert len(seen) == 53 and sum("colsum_final_kernel" in k for k in seen) == 1, sorted(seen)
