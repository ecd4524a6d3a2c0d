"""The host references of the dot-product attention tests, checked without a GPU: the fp64 restatement
(gatdot_ref.restate64) against torch's autograd in fp64, the fp32 twin against the restatement, the bar of every output by
the project's rule and what that bar must be able to tell apart, the two-destination known answer, the refusals of
gat(variant="dot") (which come before any device work), and the register report of csrc/gatdot.hip."""
import os
import re
import shutil
import subprocess
from importlib import import_module

import numpy as np
import pytest

import gat_ref as ref
import gatdot_ref as dot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _autograd(indptr, indices, Zq, Zk, Zv, K, G):
    import torch
    n, d = indptr.size - 1, Zq.shape[1]
    dh = d // K
    rows = torch.from_numpy(np.repeat(np.arange(n), np.diff(indptr.astype(np.int64))))
    cols = torch.from_numpy(indices.astype(np.int64))
    q, k, v = (torch.tensor(M, dtype=torch.float64, requires_grad=True) for M in (Zq, Zk, Zv))
    q3, k3, v3 = q.view(-1, K, dh), k.view(-1, K, dh), v.view(-1, K, dh)
    e = float(dot.default_scale(dh)) * (q3[rows] * k3[cols]).sum(-1)
    p = torch.exp(e)                                   # |score| <~ 6 on these inputs: no max to subtract
    alpha = p / torch.zeros(n, K, dtype=torch.float64).index_add(0, rows, p)[rows]
    out = torch.zeros(n, K, dh, dtype=torch.float64).index_add(0, rows, alpha[:, :, None] * v3[cols]).view(n, d)
    out.backward(torch.tensor(G, dtype=torch.float64))
    return out.detach().numpy(), q.grad.numpy(), k.grad.numpy(), v.grad.numpy()


@pytest.mark.parametrize("graph", ["long", "rect"])
@pytest.mark.parametrize("K,dh", dot.AUTOGRAD_SHAPES)
def test_restatement_matches_autograd(graph, K, dh):
    """out, G_Zq, G_Zk and G_Zv of the fp64 restatement against torch CPU autograd in fp64 on the long graph (empty rows, one
    entry, 63 .. 4097 entries, a duplicated column, an unreferenced column) and the 200 x 320 block: <= 1e-10"""
    c = dot.case(graph, K, dh)
    indptr, indices = c["indptr"], c["indices"]
    r = c["want"]
    out, G_Zq, G_Zk, G_Zv = _autograd(indptr, indices, c["Zq"], c["Zk"], c["Zv"], K, c["G"])
    for what, got, want in (("out", r["out"], out), ("G_Zq", r["G_Zq"], G_Zq), ("G_Zk", r["G_Zk"], G_Zk),
                            ("G_Zv", r["G_Zv"], G_Zv)):
        d = ref.relerr(got, want)
        print(f"[gatdot] restatement against autograd {graph} K={K} dh={dh} {what}: {d:.3e}")
        assert d <= 1e-10, (what, d)
    empty = np.flatnonzero(np.diff(indptr.astype(np.int64)) == 0)
    assert empty.size and not r["out"][empty].any() and not r["lse"][empty].any() and not r["G_Zq"][empty].any()
    assert not r["G_Zk"][ref.UNREFERENCED].any() and not r["G_Zv"][ref.UNREFERENCED].any()


def _worst_twin():
    worst = dict.fromkeys(dot.NAMES, (0.0, None))
    for name, K, dh in dot.cases():
        c = dot.case(name, K, dh)
        for what in dot.NAMES:
            row, d = ref.rowerr(c["twin"][what], c["want"][what], c["scale"][what])
            if d > worst[what][0]:
                worst[what] = (d, (name, K, dh, row))
    return worst


def test_the_bars_follow_the_rule():
    """per output: ROW_TOL where the fp32 twin's worst row-scaled distance from the exact restatement over every case the
    device runs stays within ROW_TOL / 8, eight times the twin's worst otherwise -- gatdot_ref.BAR, fixed here before any
    device run -- and the recorded twin figures are the ones measured"""
    worst = _worst_twin()
    print("[gatdot] worst row-scaled twin distance per output: " +
          ", ".join(f"{k} {d:.2e} at {where}" for k, (d, where) in worst.items()))
    for what, (d, where) in worst.items():
        assert np.isfinite(d), (what, where)                # an element without terms is exact in the twin too
        assert dot.BAR[what] == pytest.approx(dot.bar_rule(d), rel=0.05), (what, d, where)
        assert d == pytest.approx(dot.TWIN_MEASURED[what], rel=0.05), (what, d)


def test_the_bar_tells_a_wrong_formula_apart():
    """the three mutations of the restatement -- c left out, G_Zk accumulated from Zk instead of Zq, D left out of ds -- each
    exceed the bar of the output they spoil on at least one case"""
    for mutation, spoiled in dot.MUTATIONS.items():
        worst = 0.0
        for name, K, dh in [("long", 4, 32), ("long", 3, 7), ("rect", 2, 65)]:
            c = dot.case(name, K, dh)
            r = dot.restate64(c["indptr"], c["indices"], c["Zq"], c["Zk"], c["Zv"], K, G=c["G"], exact=True, mutate=mutation)
            worst = max(worst, ref.rowdist(r[spoiled], c["want"][spoiled], c["scale"][spoiled]).max() / dot.BAR[spoiled])
        print(f"[gatdot] mutation {mutation!r}: {spoiled} moves by {worst:.1f} bars")
        assert worst > 1, (mutation, spoiled, worst)


def test_two_destination_known_answer():
    """gatdot_ref.dynamic_probe(): exact scores (3, 1) and (1, 3), alpha = 1 / (1 + e^-2) for each destination's favourite,
    and the two destinations prefer different sources"""
    indptr, indices, Zq, Zk, Zv = dot.dynamic_probe()
    r = dot.restate64(indptr, indices, Zq, Zk, Zv, 1, exact=True)
    np.testing.assert_array_equal(r["e"].reshape(2, 2), [[3.0, 1.0], [1.0, 3.0]])
    alpha = r["alpha"].reshape(2, 2)
    hi = 1 / (1 + np.exp(-2.0))
    np.testing.assert_allclose(alpha, [[hi, 1 - hi], [1 - hi, hi]], rtol=1e-14)
    np.testing.assert_allclose(r["out"][:, :2], alpha, rtol=1e-14)
    np.testing.assert_allclose(r["lse"].reshape(-1), [3 + np.log1p(np.exp(-2.0))] * 2, rtol=1e-14)
    assert alpha.argmax(axis=1).tolist() == [0, 1]


def test_probe_and_stress_cases_are_what_they_claim():
    """forward_probe_case: exact scores of 0 and 40, lse = 40, out = the probed source's Zv row in fp32 almost everywhere;
    stress_case: every score exact (a multiple of c) with the largest |e| in [100, 256)"""
    for K, dh in ((4, 32), (3, 7)):
        for t in range(ref.PROBE_SLOTS):
            c = dot.forward_probe_case(t, K, dh)
            assert set(np.unique(c["want"]["e"]).tolist()) == {0.0, 40.0}
            assert np.abs(c["want"]["lse"] - 40).max() <= 1e-12
            assert (c["want"]["out"].astype(np.float32) == c["Zv"][c["hot"]]).mean() >= 0.99
    for K, dh in dot.STRESS_SHAPES:
        c = dot.stress_case(K, dh)
        e, cc = c["want"]["e"], float(dot.default_scale(dh))
        assert cc == 2.0 ** round(np.log2(cc)) and (e / cc == np.round(e / cc)).all()
        assert 100 <= np.abs(e).max() < 256, (c["a"], np.abs(e).max())
        assert c["a"] ** 2 * dh < 2 ** 24


def _tiny(pkg, n=8):
    return pkg.csr_matrix(np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32), np.ones(n, dtype=np.float32), n)


def _stand_in(pkg, variant="dot"):
    """a gat object without a device, as test_gatv2_cpu.py builds its own"""
    gat = import_module(pkg.__name__ + ".gat")
    G = gat.gat.__new__(gat.gat)
    G.variant, G._dropout_layers, G.attn_dropout_p, G._attn_dropout_params = variant, 2, 0.0, None
    G.dropout_p, G.dropout_seed, G.dropout_epoch = 0.0, 0, 0
    G.layers_, G.heads = [], [4, 1]
    return gat, G


def test_constructor_refusals_need_no_gpu(pkg):
    A = _tiny(pkg)
    with pytest.raises(ValueError, match="variant"):
        pkg.gat(A, [16, 32, 5], variant="dot2")
    with pytest.raises(ValueError, match=r'"dot".*attention dropout'):
        pkg.gat(A, [16, 32, 5], variant="dot", attn_dropout=0.25)
    with pytest.raises(ValueError, match="not divisible"):
        pkg.gat(A, [16, 30, 5], heads=4, variant="dot")
    big = type("shape_only", (), {"n": lambda self: 1 << 20, "m": lambda self: 1 << 20})()
    with pytest.raises(ValueError, match=r'"dot".*2\^31'):
        pkg.gat(big, [16, 1024, 5], heads=4, variant="dot")


def test_check_variant_keeps_v1_and_v2(pkg):
    gat = import_module(pkg.__name__ + ".gat")
    assert gat.VARIANTS == ("v1", "v2", "dot")
    assert gat.check_variant("v1") == "v1" and gat.check_variant("v1", 0.5) == "v1" and gat.check_variant("v2") == "v2"
    assert gat.check_variant("dot") == "dot"
    with pytest.raises(ValueError, match=r'gat\(variant="v2"\) has no attention dropout: attn_dropout must be 0'):
        gat.check_variant("v2", 0.5)
    with pytest.raises(ValueError, match="variant"):
        gat.check_variant(None)


def test_set_dropout_refuses_attention_dropout_on_dot(pkg):
    _, G = _stand_in(pkg)
    with pytest.raises(ValueError, match=r'"dot".*attention dropout'):
        G.set_dropout(0.5, seed=3, epoch=1, attn=0.1)
    assert (G.dropout_p, G.dropout_seed, G.dropout_epoch, G.attn_dropout_p) == (0.0, 0, 0, 0.0)
    G.set_dropout(0.5, seed=3, epoch=1)
    assert (G.dropout_p, G.dropout_seed, G.dropout_epoch, G.attn_dropout_p) == (0.5, 3, 1, 0.0)


def test_export_and_checkpoints_are_refused(pkg, tmp_path):
    """attention_weights, gat_layer.alpha, save, load and the selector's save_best raise ValueError naming dot with None in
    the place of the context; nothing is written, read or created"""
    gat, G = _stand_in(pkg)
    with pytest.raises(ValueError, match="dot"):
        G.attention_weights(None, None)
    layer = gat.gatdot_layer.__new__(gat.gatdot_layer)
    layer.name, layer.H = "0_", object()
    with pytest.raises(ValueError, match="dot"):
        layer.alpha(None)
    path = tmp_path / "model.ckpt"
    with pytest.raises(ValueError, match="dot"):
        G.save(None, str(path))
    with pytest.raises(ValueError, match="dot"):
        G.load(None, str(path))                            # refused before the (missing) file is opened
    with pytest.raises(ValueError, match="dot"):
        G._write_checkpoint(None, str(path), {}, False, 0)
    assert not path.exists() and not list(tmp_path.iterdir())


def test_dist_gat_refuses_dot(pkg):
    dist = import_module(pkg.__name__ + ".dist")
    with pytest.raises(ValueError, match="dot"):
        dist.dist_gat(None, None, None, [16, 32, 5], variant="dot")
    with pytest.raises(ValueError, match="variant"):
        dist.dist_gat(None, None, None, [16, 32, 5], variant="dot2")


def test_attention_dot_has_no_parameter(pkg):
    """a row of nobody's Adam table, and invisible to the generic parameter readers"""
    gat = import_module(pkg.__name__ + ".gat")
    a = gat.attention_dot.__new__(gat.attention_dot)
    assert a.adam_tensors(5e-4) == [] and a.adam_update(None, 1e-2, 0.9, 0.999, 5e-4, 1e-8) is None
    assert a.att is None and a.m is None
    layer = gat.gatdot_layer.__new__(gat.gatdot_layer)
    linear = import_module(pkg.__name__ + ".gcn").linear
    layer.lin, layer.attn = linear.__new__(linear), a         # the real owner class carries the table; it has no tensor
    assert layer.params() == [layer.lin]
    model = type("m", (), {"layers_": [layer]})()
    names = [name for name, *_ in import_module(pkg.__name__ + ".checkpoint").model_params(model)]
    assert names == ["W0", "b0"]
    assert pkg.ops.gatdot_scale(16) == 0.25 and pkg.ops.gatdot_scale(7) == float(np.float32(1 / np.sqrt(7)))


def test_ops_refuse_bad_shapes_before_the_library(pkg):
    """the wrappers raise ValueError on stand-ins that own no device memory"""
    class M:
        def __init__(self, n, m): self.N, self.Mm = n, m
        def n(self): return self.N
        def m(self): return self.Mm
        def shape(self): return (self.N, self.Mm)
        def buffer(self): raise AssertionError("the library must not be reached")
    ops = pkg.ops
    F = _tiny(pkg)
    with pytest.raises(ValueError, match="not divisible"):
        ops.gatdot_forward(None, F, M(8, 30), M(8, 30), M(8, 30), M(8, 30), M(8, 4), 4)
    with pytest.raises(ValueError, match="shape mismatch"):
        ops.gatdot_forward(None, F, M(8, 32), M(9, 32), M(8, 32), M(8, 32), M(8, 4), 4)
    with pytest.raises(ValueError, match="neither"):
        ops.gatdot_forward(None, F, M(8, 64), M(8, 32), M(8, 32), M(8, 32), M(8, 4), 4)
    with pytest.raises(ValueError, match="lse must be"):
        ops.gatdot_forward(None, F, M(8, 96), M(8, 96), M(8, 96), M(8, 32), M(8, 3), 4)
    with pytest.raises(ValueError, match="lse and D"):
        ops.gatdot_backward_dst(None, F, M(8, 96), M(8, 96), M(8, 96), M(8, 4), M(8, 32), M(8, 32), M(8, 3), M(8, 96), 4)
    with pytest.raises(ValueError, match="shape mismatch"):
        ops.gatdot_backward_src(None, F, M(8, 96), M(8, 96), M(8, 96), M(8, 4), M(8, 4), M(7, 32), M(8, 96), M(8, 96), 4)
    one = M(8, 32)
    with pytest.raises(ValueError, match="same"):
        ops.gatdot_backward_src(None, F, M(8, 96), M(8, 96), M(8, 96), M(8, 4), M(8, 4), M(8, 32), one, one, 4)
    with pytest.raises(ValueError, match="heads"):
        ops.gatdot_forward(None, F, M(8, 34), M(8, 34), M(8, 34), M(8, 34), M(8, 17), 17)


# per attention file: the prefix of its kernels' names and the instantiations of each templated kernel -- gat_dispatch's five
# (VEC, NT, U) x the flags (gat.hip: DROP on the three sparse kernels, REC on backward_src as well, KV = 4 / 1 on the export;
# gatv2.hip: REC on backward_src)
ATTENTION_KERNELS = {
    "gat.hip": ("gat_", dict(gat_forward_kernel=10, gat_backward_dst_kernel=10, gat_backward_src_kernel=20,
                             gat_alpha_kernel=2)),
    "gatv2.hip": ("gatv2_", dict(gatv2_forward_kernel=5, gatv2_backward_dst_kernel=5, gatv2_backward_src_kernel=10,
                                 gatv2_alpha_kernel=5)),
    "gatdot.hip": ("gatdot_", dict(gatdot_forward_kernel=5, gatdot_backward_dst_kernel=5, gatdot_backward_src_kernel=5)),
}


@pytest.mark.parametrize("source", sorted(ATTENTION_KERNELS))
def test_no_instantiation_uses_scratch(tmp_path, source):
    """csrc/gat.hip, gatv2.hip and gatdot.hip compiled for gfx950 to assembly: the resource metadata of every kernel whose
    name contains the file's prefix reports a private segment of zero bytes and zero spilled vector registers -- every
    instantiation of ATTENTION_KERNELS, and in gatdot.hip nothing else: all fifteen (three kernels x five (VEC, NT, U));
    its backward_src holds six head-row arrays per lane and is the one closest to the limit"""
    prefix, counts = ATTENTION_KERNELS[source]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path / (source + ".s")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-S",
                        "--cuda-device-only", os.path.join(ROOT, "mg-gcn_amd", "csrc", source), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels"):]
    seen = {}
    for b in re.split(r"\n\s*- \.agpr_count:", "\n" + meta)[1:]:
        blk = ".agpr_count:" + b
        nm = re.search(r"\.name:\s+(\S+)", blk)
        if not nm or prefix not in nm.group(1):
            continue
        field = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                 for k in ("private_segment_fixed_size", "vgpr_spill_count", "vgpr_count", "agpr_count")}
        seen[nm.group(1)] = field
        print(f"[{source}] {nm.group(1)}: {field}")
        assert field["private_segment_fixed_size"] == 0 and field["vgpr_spill_count"] == 0, (nm.group(1), field)
    if source == "gatdot.hip":
        assert len(seen) == 15, sorted(seen)
    for kernel, count in counts.items():
        assert sum(kernel in k for k in seen) == count, (kernel, sorted(seen))
