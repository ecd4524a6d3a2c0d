"""The host references of the GATv2 tests, checked without a GPU: the fp64 restatement (gatv2_ref.restate64) against
torch's autograd in fp64, the fp32 twin against the restatement, the bar of every output by the project's rule and what
that bar must be able to tell apart, the dynamic-attention probe, the refusals of the gat constructor (which come before
any device work) and which shape reaches which compiled variant."""
from importlib import import_module

import numpy as np
import pytest

import gat_ref as ref
import gatv2_ref as v2


def _autograd(indptr, indices, Zs, Zd, att, K, G, slope):
    import torch
    n, d = indptr.size - 1, Zs.shape[1]
    dh = d // K
    rows = torch.from_numpy(np.repeat(np.arange(n), np.diff(indptr.astype(np.int64))))
    cols = torch.from_numpy(indices.astype(np.int64))
    Zst = torch.tensor(Zs, dtype=torch.float64, requires_grad=True)
    Zdt = torch.tensor(Zd, dtype=torch.float64, requires_grad=True)
    at = torch.tensor(att, dtype=torch.float64, requires_grad=True)
    Zs3, Zd3, a3 = Zst.view(-1, K, dh), Zdt.view(-1, K, dh), at.view(1, K, dh)
    e = (torch.nn.functional.leaky_relu(Zd3[rows] + Zs3[cols], slope) * a3).sum(-1)
    p = torch.exp(e)                                   # |score| <~ 10 on these inputs: no max to subtract
    alpha = p / torch.zeros(n, K, dtype=torch.float64).index_add(0, rows, p)[rows]
    out = torch.zeros(n, K, dh, dtype=torch.float64).index_add(0, rows, alpha[:, :, None] * Zs3[cols]).view(n, d)
    out.backward(torch.tensor(G, dtype=torch.float64))
    return out.detach().numpy(), Zst.grad.numpy(), Zdt.grad.numpy(), at.grad.numpy()


@pytest.mark.parametrize("K,dh", v2.AUTOGRAD_SHAPES)
def test_restatement_matches_autograd(K, dh):
    """out, G_Zs, G_Zd and G_att of the fp64 restatement against torch CPU autograd in fp64 on kernel_graph_long() (empty
    rows, one entry, 63 .. 4097 entries, a duplicated column, an unreferenced column): <= 1e-12; and P adds up to G_att"""
    indptr, indices = ref.kernel_graph_long()
    Zs, Zd, G, att = v2.inputs(320, 320, K, dh)
    r = v2.restate64(indptr, indices, Zs, Zd, att, K, G=G, exact=True)
    out, G_Zs, G_Zd, G_att = _autograd(indptr, indices, Zs, Zd, att, K, G, ref.SLOPE)
    for what, got, want in (("out", r["out"], out), ("G_Zs", r["G_Zs"], G_Zs), ("G_Zd", r["G_Zd"], G_Zd),
                            ("G_att", r["G_att"], G_att)):
        d = ref.relerr(got, want)
        print(f"[gatv2] restatement against autograd K={K} dh={dh} {what}: {d:.3e}")
        assert d <= 1e-12, (what, d)
    assert ref.relerr(r["P"].sum(axis=0), r["G_att"][0]) <= 1e-12
    assert not r["G_Zs"][ref.UNREFERENCED].any() and not r["G_Zd"][[0, 319]].any() and not r["P"][[0, 319]].any()
    assert not r["out"][[0, 319]].any() and not r["lse"][[0, 319]].any()


def _worst_twin():
    worst = dict.fromkeys(v2.NAMES, (0.0, None))
    for name, K, dh in v2.cases():
        c = v2.case(name, K, dh)
        for what in v2.NAMES:
            row, d = ref.rowerr(c["twin"][what], c["want"][what], c["scale"][what])
            if d > worst[what][0]:
                worst[what] = (d, (name, K, dh, row))
    return worst


def test_the_bars_follow_the_rule():
    """per output: ROW_TOL where the fp32 twin's worst row-scaled distance from the exact restatement over every case the
    device runs stays within ROW_TOL / 8, eight times the twin's worst otherwise -- gatv2_ref.BAR, fixed here before any
    device run -- and the recorded twin figures are the ones measured"""
    worst = _worst_twin()
    print("[gatv2] worst row-scaled twin distance per output: " +
          ", ".join(f"{k} {d:.2e} at {where}" for k, (d, where) in worst.items()))
    for what, (d, where) in worst.items():
        assert np.isfinite(d), (what, where)                # an element without terms is exact in the twin too
        assert v2.BAR[what] == pytest.approx(v2.bar_rule(d), rel=0.05), (what, d, where)
        assert d == pytest.approx(v2.TWIN_MEASURED[what], rel=0.05), (what, d)


@pytest.mark.parametrize("K,dh", v2.SHAPES)
def test_the_bar_tells_a_wrong_kernel_apart(K, dh):
    """the sensitivity conditions: the restatement with the last entry of every row of 65 or more entries removed, with the
    first entry of its last chunk removed, and with lrelu' of Zs alone in v, is at least 4 bars away in one output"""
    c = v2.case("long", K, dh)
    indptr, indices = c["indptr"], c["indices"]
    args, kw = (c["Zs"], c["Zd"], c["att"], K), dict(G=c["G"], exact=True)
    long_rows, last = ref.long_row_positions(indptr, "last")
    assert long_rows.tolist() == [4, 5, 6, 7, 8, 9, 10, 11, 12]
    mutants = {"last": v2.restate64(*ref.without_entries(indptr, indices, last), *args, **kw),
               "chunk": v2.restate64(*ref.without_entries(indptr, indices, ref.long_row_positions(indptr, "chunk")[1]), *args, **kw),
               "lrelu' of Zs": v2.restate64(indptr, indices, *args, vprime="zs", **kw)}
    for what, r in mutants.items():
        moved = {nm: ref.rowdist(r[nm], c["want"][nm], c["scale"][nm]).max() / v2.BAR[nm] for nm in v2.NAMES}
        print(f"[gatv2] K={K} dh={dh} {what}: " + ", ".join(f"{nm} {v:.1f}" for nm, v in moved.items()) + " bars")
        assert max(moved.values()) >= 4, (what, moved)


def test_dynamic_attention_probe():
    """the two destinations of gatv2_ref.dynamic_probe() prefer different sources; a v1 score on ANY s_dst, s_src gives every
    destination the same favourite"""
    indptr, indices, Zs, Zd, att = v2.dynamic_probe()
    r = v2.restate64(indptr, indices, Zs, Zd, att, 1, exact=True)
    np.testing.assert_array_equal(r["e"].reshape(2, 2), [[3.2, 1.6], [-3.2, -1.6]])
    alpha = r["alpha"].reshape(2, 2)
    assert alpha.argmax(axis=1).tolist() == [0, 1]
    rng = np.random.default_rng(0)
    for _ in range(100):
        s_dst, s_src = rng.standard_normal((2, 1)), rng.standard_normal((2, 1))
        s_src[1] = s_src[0] + rng.choice([-1, 1]) * (0.1 + rng.random())        # no ties
        w = ref.restate64(indptr, indices, np.zeros((2, 2), dtype=np.float32), np.zeros((2, 2), dtype=np.float32), 1, exact=True,
                          s_dst=s_dst, s_src=s_src)["alpha"].reshape(2, 2)
        assert w[0].argmax() == w[1].argmax()


def test_forward_probe_is_what_it_claims():
    """gatv2_ref.forward_probe_case: exact scores of 0 and 40, out = the probed source's row to fp32's last bit in all but a
    handful of near-zero elements, lse = 40"""
    for K, dh in ((4, 32), (3, 7)):
        for t in range(ref.PROBE_SLOTS):
            c = v2.forward_probe_case(t, K, dh)
            assert set(np.unique(c["want"]["e"]).tolist()) == {0.0, 40.0}
            assert np.abs(c["want"]["lse"] - 40).max() <= 1e-12
            same = c["want"]["out"].astype(np.float32) == c["Zs"][c["hot"]]
            assert same.mean() >= 0.99


def test_stress_case_reaches_the_hundreds_with_exact_scores():
    """gatv2_ref.stress_case: every row's top score lies in (100, 256), every score is a multiple of 0.25 (exact in fp32 in
    any order of summation), and the fp32 rounding of the exact lse keeps the weights' sum within 1e-5 of one"""
    for K, dh in v2.STRESS_ATT:
        c = v2.stress_case(K, dh)
        e, ip = c["want"]["e"], c["indptr"].astype(np.int64)
        tops = [e[ip[r]:ip[r + 1]].max() for r in range(c["n"])]
        assert 100 < min(tops) and max(tops) < 256, tops
        assert (e * 4 == np.round(e * 4)).all() and np.abs(e).max() < 2 ** 11
        sums = v2.alpha_row_sums(c["indptr"], e, c["want"]["lse"].astype(np.float32))
        assert np.abs(sums - 1).max() <= 1e-5


def _tiny(pkg, n=8):
    return pkg.csr_matrix(np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32), np.ones(n, dtype=np.float32), n)


def test_constructor_refusals_need_no_gpu(pkg):
    A = _tiny(pkg)
    with pytest.raises(ValueError, match="variant"):
        pkg.gat(A, [16, 32, 5], variant="v3")
    with pytest.raises(ValueError, match="variant"):
        pkg.gat(A, [16, 32, 5], variant=None)
    with pytest.raises(ValueError, match="attention dropout"):
        pkg.gat(A, [16, 32, 5], variant="v2", attn_dropout=0.25)
    with pytest.raises(ValueError, match="not divisible"):
        pkg.gat(A, [16, 30, 5], heads=4, variant="v2")


def test_set_dropout_refuses_attention_dropout_on_v2(pkg):
    """on a stand-in without a device: set_dropout(attn > 0) raises before anything is stored; attn = 0 is accepted"""
    gat = import_module(pkg.__name__ + ".gat")
    G = gat.gat.__new__(gat.gat)
    G.variant, G._dropout_layers, G.attn_dropout_p, G._attn_dropout_params = "v2", 2, 0.0, None
    G.dropout_p, G.dropout_seed, G.dropout_epoch = 0.0, 0, 0
    with pytest.raises(ValueError, match="attention dropout"):
        G.set_dropout(0.5, seed=3, epoch=1, attn=0.1)
    assert (G.dropout_p, G.dropout_seed, G.dropout_epoch, G.attn_dropout_p) == (0.0, 0, 0, 0.0)
    G.set_dropout(0.5, seed=3, epoch=1)
    assert (G.dropout_p, G.dropout_seed, G.dropout_epoch, G.attn_dropout_p) == (0.5, 3, 1, 0.0)
    G.variant = "v1"
    G.set_dropout(0.5, seed=3, epoch=1, attn=0.1)
    assert G.attn_dropout_p == 0.1
    assert gat.check_variant("v1", 0.5) == "v1" and gat.check_variant("v2") == "v2"


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
    with pytest.raises(ValueError, match="att must be 1 x"):
        ops.gatv2_forward(None, F, M(8, 32), M(8, 32), M(2, 32), M(8, 32), M(8, 4), 4)
    with pytest.raises(ValueError, match="not divisible"):
        ops.gatv2_forward(None, F, M(8, 30), M(8, 30), M(1, 30), M(8, 30), M(8, 4), 4)
    with pytest.raises(ValueError, match="shape mismatch"):
        ops.gatv2_forward(None, F, M(9, 32), M(8, 32), M(1, 32), M(8, 32), M(8, 4), 4)
    with pytest.raises(ValueError, match="neither"):
        ops.gatv2_forward(None, F, M(8, 48), M(8, 32), M(1, 32), M(8, 32), M(8, 4), 4)
    with pytest.raises(ValueError, match="lse and D"):
        ops.gatv2_backward_dst(None, F, M(8, 64), M(8, 64), M(1, 32), M(8, 4), M(8, 32), M(8, 32), M(8, 3), M(8, 64), M(8, 32), 4)
    with pytest.raises(ValueError, match="shape mismatch"):
        ops.gatv2_backward_src(None, F, M(8, 64), M(8, 64), M(1, 32), M(8, 4), M(8, 4), M(7, 32), M(8, 64), 4)
    with pytest.raises(ValueError, match="G_att must be"):
        ops.gatv2_att_grad(None, M(8, 32), M(2, 32))
    with pytest.raises(ValueError, match="width"):
        ops.gatv2_att_grad(None, M(8, 1025), M(1, 1025))


def test_shape_list_reaches_every_variant():
    """csrc/gat_internal.h's head geometry and dispatch (gat_ref.head_geometry_for restates them; the GATv2 calls add att to
    the operands that must be aligned): the shapes select all five (VEC, NT, U) variants, each of them on the rectangular
    block too, mask lanes on both paths, and the misaligned run of (4, 32) lands on the element path"""
    geo = {(K, dh): ref.head_geometry_for(dh, dh % 4 == 0) for K, dh in v2.SHAPES}
    assert {v for v, _ in geo.values()} == {(4, 1, 4), (4, 4, 1), (1, 1, 4), (1, 4, 2), (1, 16, 1)}
    assert geo[(4, 32)] == ((4, 1, 4), 1) and geo[(16, 4)] == ((4, 1, 4), 1) and geo[(1, 260)] == ((4, 4, 1), 2)
    assert geo[(1, 1024)] == ((4, 4, 1), 4) and geo[(3, 7)] == ((1, 1, 4), 1) and geo[(2, 65)] == ((1, 4, 2), 2)
    assert geo[(1, 255)] == ((1, 4, 2), 4) and geo[(1, 257)] == ((1, 16, 1), 5)
    assert {ref.head_geometry_for(dh, dh % 4 == 0)[0] for _, dh in v2.RECT_SHAPES} == {v for v, _ in geo.values()}
    assert ref.head_geometry_for(32, False) == ((1, 1, 4), 1)
    assert all(K <= 16 and K * dh <= 1024 for K, dh in v2.SHAPES)
    assert set(v2.AUTOGRAD_SHAPES) <= set(v2.SHAPES)
