"""The host references of the GAT dropout tests, checked without a GPU: the fp64 restatement with attention dropout
(gat_dropout_ref.restate64) against torch's autograd in fp64 with the mask held fixed, the fp32 twin against the
restatement on every case the device tests use (which fixes the bar before any device run), four mutations of the mask and
of the formula that the bar must tell apart, the statistics of the mask, the count probe's own claim, and the option
checks of the gat constructor and set_dropout, which come before any device work."""
import numpy as np
import pytest

import dropout_ref
import gat_dropout_ref as dref
import gat_ref as ref


def _autograd(indptr, indices, Z, att, K, G, slope, keep, scale):
    import torch
    n, d = indptr.size - 1, Z.shape[1]
    dh = d // K
    rows = torch.from_numpy(np.repeat(np.arange(n), np.diff(indptr.astype(np.int64))))
    cols = torch.from_numpy(indices.astype(np.int64))
    q = torch.from_numpy(np.where(keep, float(scale), 0.0))                 # a constant: no gradient flows into the mask
    Zt = torch.tensor(Z, dtype=torch.float64, requires_grad=True)
    at = torch.tensor(att, dtype=torch.float64, requires_grad=True)
    Z3, a3 = Zt.view(-1, K, dh), at.view(2, K, dh)
    s_dst, s_src = (Z3 * a3[0]).sum(-1), (Z3 * a3[1]).sum(-1)
    e = torch.nn.functional.leaky_relu(s_dst[rows] + s_src[cols], slope)
    p = torch.exp(e)
    alpha = p / torch.zeros(n, K, dtype=torch.float64).index_add(0, rows, p)[rows]      # the sum takes EVERY entry
    out = torch.zeros(n, K, dh, dtype=torch.float64).index_add(0, rows, (alpha * q)[:, :, None] * Z3[cols]).view(n, d)
    out.backward(torch.tensor(G, dtype=torch.float64))
    return out.detach().numpy(), Zt.grad.numpy(), at.grad.numpy()


@pytest.mark.parametrize("p", [0.5, 0.9])
@pytest.mark.parametrize("K,dh", [(3, 7), (4, 8), (6, 5)])
def test_restatement_matches_autograd(K, dh, p):
    """out, G_Z and G_att of the fp64 restatement against torch CPU autograd in fp64 on the kernel-test graph, the mask a
    constant tensor: <= 1e-12.  D = G . out with the DROPPED out is what makes sum_j alpha (q dalpha) = D hold"""
    indptr, indices = ref.kernel_graph()
    Z, _, G, att = ref.tolerance_inputs(320, 320, K, dh)
    keep, scale = dref.keep_mask(indptr, indices, K, p, 7, 65), dropout_ref.params(p)[1]
    r = dref.restate64(indptr, indices, Z, att, K, keep, scale, G=G, exact=True)
    out, G_Z, G_att = _autograd(indptr, indices, Z, att, K, G, ref.SLOPE, keep, scale)
    for what, got, want in (("out", r["out"], out), ("G_Z", r["G_Z"], G_Z), ("G_att", r["G_att"], G_att)):
        d = ref.relerr(got, want)
        print(f"[gat-drop] restatement against autograd K={K} dh={dh} p={p} {what}: {d:.3e}")
        assert d <= 1e-12, (what, d)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_keeping_everything_is_the_plain_restatement(dtype):
    """keep = all, scale = 1: the bits of gat_ref.attention in every output, in both precisions"""
    indptr, indices = ref.kernel_graph()
    Z, _, G, att = ref.tolerance_inputs(320, 320, 4, 8)
    keep = np.ones((indices.size, 4), dtype=bool)
    with np.errstate(over="ignore"):
        a = dref.attention(indptr, indices, Z, att, 4, keep, np.float32(1), G=G, dtype=dtype)
        b = ref.attention(indptr, indices, Z, att, 4, G=G, dtype=dtype)
    for what in ref.NAMES + ("alpha",):
        np.testing.assert_array_equal(a[what].view(np.uint8), b[what].view(np.uint8), err_msg=what)


def test_twin_fixes_the_bar():
    """the fp32 twin against the exact restatement, row-scaled, on every case of test_gpu_gat_dropout.py (a), output by
    output: where its worst is within ROW_TOL / 8 the bar is gat_ref.ROW_TOL, where it is not the bar is eight times the
    twin's worst (rounded up, by less than a tenth) -- never the single widest bar for every output"""
    worst = dict.fromkeys(dref.DROP_NAMES, (0.0, None))
    for case in dref.drop_cases():
        c = dref.drop_case(*case)
        for what in dref.DROP_NAMES:
            d = ref.rowerr(c["twin"][what], c["want"][what], c["scale"][what])[1]
            assert np.isfinite(d), (case, what)
            worst[what] = max(worst[what], (d, case))
    print("[gat-drop] worst row-scaled twin distance per output: " + ", ".join(f"{k} {v[0]:.2e} {v[1]}" for k, v in worst.items()))
    for what, (d, case) in worst.items():
        assert d == pytest.approx(dref.TWIN_DROP_MEASURED[what], rel=0.05), (what, case)
        if d <= ref.ROW_TOL / 8:
            assert dref.DROP_TOL[what] == ref.ROW_TOL, what
        else:
            assert 8 * d <= dref.DROP_TOL[what] <= 8.8 * d, what
    assert [k for k, v in dref.DROP_TOL.items() if v == ref.ROW_TOL] == ["out", "lse", "D"]


@pytest.mark.parametrize("K,dh", dref.DROP_SHAPES)
def test_a_wrong_mask_or_a_renormalised_softmax_is_four_bars_away(K, dh):
    """the conditions on the bar, at p = 0.5 on kernel_graph_long with dst0 = 1000 and src0 = 70000: the restatement with i and
    j swapped in the counter, with head 0's word for every head, with dst0 / src0 ignored, and with the dropped entries
    taken out of the softmax sum as well, is at least 4 of its own bars away in one of out, ds_src, G_Z.  A one-head shape has no
    second head to confuse: there "head0" must change nothing at all"""
    indptr, indices, _ = ref.edge_graphs()["long"]
    c = dref.drop_case("long", K, dh, 0.5)
    off = (dref.RECT_DST0, dref.RECT_SRC0)
    scale = dropout_ref.params(0.5)[1]
    args = (indptr, indices, c["Z"], c["att"], K)

    def run(keep, **kw):
        return dref.restate64(*args, keep, scale, G=c["G"], exact=True, **kw)
    mask = lambda *o, **mut: dref.keep_mask(indptr, indices, K, 0.5, dref.SEED, dref.STREAM, *o, **mut)
    want = run(mask(*off), scales=True)
    mutants = {"swap": run(mask(*off, swap=True)), "head0": run(mask(*off, head0=True)), "offsets": run(mask(0, 0)),
               "renormalised": run(mask(*off), softmax_over_kept=True)}
    for what, r in mutants.items():
        moved = {nm: ref.rowdist(r[nm], want[nm], want["scale"][nm]).max() / dref.DROP_TOL[nm] for nm in ("out", "ds_src", "G_Z")}
        print(f"[gat-drop] K={K} dh={dh} {what}: " + ", ".join(f"{nm} {v:.1f}" for nm, v in moved.items()) + " bars")
        if what == "head0" and K == 1:
            assert max(moved.values()) == 0.0
        else:
            assert max(moved.values()) >= 4, (what, moved)


@pytest.mark.parametrize("p", [0.1, 0.5, 0.6, 0.9])
def test_kept_fraction(p):
    """over 10^6 draws (1000 destinations x 250 sources x 4 heads) the kept fraction is within 4 sigma of 1 - p"""
    i, j = np.repeat(np.arange(1000), 250), np.tile(np.arange(250), 1000)
    kept = (dref.words(i, j, 4, 12345, 77) >= np.uint32(dropout_ref.params(p)[0])).mean()
    sigma = (p * (1 - p) / 1e6) ** 0.5
    print(f"[gat-drop] p={p}: kept {kept:.6f}, expected {1 - p:.6f} +- {sigma:.1e}")
    assert abs(kept - (1 - p)) <= 4 * sigma


def test_no_word_is_shared_with_the_matrix_dropout():
    """rows, columns < 512 at one (seed, stream): the words mggcn_dropout_f32 draws (third counter word = row >> 32 = 0) and
    the ones the attention draws for destinations, sources < 512 and sixteen heads (third word 2^31 | k >> 2) come from
    disjoint counters.  Philox is a bijection of the counter for a fixed key, so disjoint counters cannot give the same four
    words: checked on the 128-bit blocks, not on single words, which collide by chance among 2^20 draws of 32 bits"""
    seed, stream = 99, 5
    blocks = dropout_ref.words(512, 2048, 0, seed, stream).reshape(512 * 512, 4)           # one block per 4 columns
    i, j = np.repeat(np.arange(512), 512), np.tile(np.arange(512), 512)
    mine = dref.words(i, j, 16, seed, stream).reshape(512 * 512 * 4, 4)
    as_key = lambda a: {bytes(x) for x in np.ascontiguousarray(a)}
    a, b = as_key(blocks), as_key(mine)
    assert len(a) == blocks.shape[0] and len(b) == mine.shape[0]                           # all distinct within each
    assert not (a & b)


def test_duplicate_entries_share_one_bit_and_the_mask_ignores_the_walk():
    """the duplicated column of kernel_graph_long's row 13 has one bit; the mask of F^T's entries, drawn with the roles
    swapped as backward_src does, is the mask of F's entries reordered; rows [5, 13) with dst0 = 5 draw the whole call's"""
    indptr, indices = ref.kernel_graph_long()
    keep = dref.keep_mask(indptr, indices, 6, 0.5, dref.SEED, dref.STREAM)
    b = int(indptr[ref.LONG_DUPLICATE_ROW])
    assert indices[b] == indices[b + 1] and (keep[b] == keep[b + 1]).all()
    t_indptr, t_indices = ref.transpose_pattern(indptr, indices, 320)
    t_rows = np.repeat(np.arange(320), np.diff(t_indptr.astype(np.int64)))
    t_keep = dref.words(t_indices, t_rows, 6, dref.SEED, dref.STREAM) >= np.uint32(dropout_ref.params(0.5)[0])
    np.testing.assert_array_equal(t_keep, keep[np.argsort(indices, kind="stable")])
    a, e = int(indptr[5]), int(indptr[13])
    part = dref.keep_mask(indptr[5:14] - indptr[5], indices[a:e], 6, 0.5, dref.SEED, dref.STREAM, dst0=5)
    np.testing.assert_array_equal(part, keep[a:e])


@pytest.mark.parametrize("K,dh", [(4, 64), (16, 4)])
def test_count_probe_counts(K, dh):
    """the count probe's own claim, as F and as F^T: with att = 0 the restatement's out[i, k, c] L / 2 (G_Z[j, k, c] L / 2 with
    lse = log L supplied) is the number of kept entries of that bucket to 1e-9, every bucket of the 4097-entry row sees both
    kept and dropped entries, and one miscounted entry is a hundred times the device test's 1e-5"""
    att = np.zeros((2, K * dh), dtype=np.float32)
    c = dref.count_probe(K, dh)
    r = dref.restate64(c["indptr"], c["indices"], c["hot"], att, K, c["keep"], np.float32(2), exact=True)
    got = r["out"].reshape(5, K, dh) * c["L"][:, None, None] / 2
    assert np.abs(got - c["counts"]).max() <= 1e-9
    per_bucket = -(-4097 // dh)
    assert 0 < c["counts"][4].min() and c["counts"][4].max() < per_bucket
    assert c["counts"].sum() == c["keep"].sum()
    assert 1.0 / c["counts"].max() >= 100 * 1e-5
    t = dref.count_probe(K, dh, transposed=True)
    assert (t["keep"] != c["keep"]).any()                      # another mask: the roles of row and entry are swapped
    indptr, indices = ref.transpose_pattern(t["indptr"], t["indices"], t["n_ent"])          # F: 4548 destinations x 5 sources
    keepF = np.empty_like(t["keep"])
    keepF[t["indices"].astype(np.int64)] = t["keep"]           # destination i has exactly one entry: F's entry order is i
    zeros = np.zeros((t["n_ent"], K))
    r = dref.restate64(indptr, indices, np.zeros((5, K * dh), dtype=np.float32), att, K, keepF, np.float32(2), G=t["hot"],
                       Z_dst=np.zeros((t["n_ent"], K * dh), dtype=np.float32), s_dst=zeros, lse=t["lse"], D=zeros, exact=True)
    got = r["G_Z"].reshape(5, K, dh) * t["L"][:, None, None] / 2
    assert np.abs(got - t["counts"]).max() <= 1e-5 * max(1, t["counts"].max())       # lse is log L rounded to fp32
    assert t["counts"].sum() == t["keep"].sum()


def test_all_dropped_seed_drops_every_head():
    seed = dref.all_dropped_seed(1, 7, 4, 0.9, dref.STREAM)
    assert not dref.keep_mask(np.array([0, 0, 1], dtype=np.uint32), np.array([7], dtype=np.uint32), 4, 0.9, seed, dref.STREAM).any()


# ---- the model's options -----------------------------------------------------------------------------------------------------------
def _tiny(pkg, n=8):
    return pkg.csr_matrix(np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32), np.ones(n, dtype=np.float32), n)


@pytest.mark.parametrize("kw", [dict(dropout=1.0), dict(dropout=-0.1), dict(attn_dropout=1.0), dict(attn_dropout=float("nan")),
                                dict(dropout="0.5"), dict(attn_dropout=None)])
def test_constructor_refuses_a_bad_probability_without_a_gpu(pkg, kw):
    with pytest.raises(ValueError, match="dropout"):
        pkg.gat(_tiny(pkg), [16, 32, 5], **kw)


@pytest.mark.parametrize("kw", [dict(dropout=0.5), dict(attn_dropout=0.5)])
def test_constructor_refuses_more_than_64_layers_without_a_gpu(pkg, kw):
    with pytest.raises(ValueError, match="64 layers"):
        pkg.gat(_tiny(pkg), [4] * 66 + [2], heads=1, **kw)


def test_ops_refuse_a_bad_drop_tuple_before_the_library(pkg):
    """the checks of ops.gat_forward(drop=) need no context: a tuple of the wrong length, a threshold beyond 32 bits and
    an index range beyond 2^32 raise ValueError (the library would print and exit)"""
    class shape_only:
        def __init__(self, n, m):
            self._s = (n, m)
        def n(self): return self._s[0]
        def m(self): return self._s[1]
        def shape(self): return self._s
    F = shape_only(8, 8)
    Z, s, out = shape_only(8, 16), shape_only(8, 4), shape_only(8, 16)
    for drop in ((1, 2.0, 0, 0), (1 << 32, 2.0, 0, 0, 0, 0), (1, 2.0, 0, 0, (1 << 32) - 7, 0), (1, 2.0, 0, 0, 0, -1)):
        with pytest.raises(ValueError, match="gat forward"):
            pkg.ops.gat_forward(None, F, Z, s, s, out, s, 4, drop=drop)
