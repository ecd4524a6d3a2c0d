"""The host references of the GAT tests, checked without a GPU: the fp64 restatement (gat_ref.restate64) against torch's
autograd in fp64, the fp32 twin against the restatement on the inputs the device tests use, the option checks of the
gat constructor, which come before any device work, and the helpers of test_gpu_gat_edges.py: injected intermediates,
the long graph, the shape list, the row-scaled bar against the twin and against three off-by-one mutations."""
import numpy as np
import pytest

import gat_ref as ref


@pytest.fixture(scope="module")
def graph():
    return ref.kernel_graph()


def _autograd(indptr, indices, Z, att, K, G, slope):
    import torch
    n, d = indptr.size - 1, Z.shape[1]
    dh = d // K
    rows = torch.from_numpy(np.repeat(np.arange(n), np.diff(indptr.astype(np.int64))))
    cols = torch.from_numpy(indices.astype(np.int64))
    Zt = torch.tensor(Z, dtype=torch.float64, requires_grad=True)
    at = torch.tensor(att, dtype=torch.float64, requires_grad=True)
    Z3, a3 = Zt.view(-1, K, dh), at.view(2, K, dh)
    s_dst, s_src = (Z3 * a3[0]).sum(-1), (Z3 * a3[1]).sum(-1)
    e = torch.nn.functional.leaky_relu(s_dst[rows] + s_src[cols], slope)
    p = torch.exp(e)                                   # |score| <~ 10 on these inputs: no max to subtract
    alpha = p / torch.zeros(n, K, dtype=torch.float64).index_add(0, rows, p)[rows]
    out = torch.zeros(n, K, dh, dtype=torch.float64).index_add(0, rows, alpha[:, :, None] * Z3[cols]).view(n, d)
    out.backward(torch.tensor(G, dtype=torch.float64))
    return out.detach().numpy(), Zt.grad.numpy(), at.grad.numpy()


@pytest.mark.parametrize("K,dh", [(3, 7), (4, 8), (1, 5)])
def test_restatement_matches_autograd(graph, K, dh):
    """out, G_Z and G_att of the fp64 restatement against torch CPU autograd in fp64, on the kernel-test graph (empty rows,
    one entry, 64 / 65 / 1000 / 4097 entries, a duplicated column, an unreferenced column): <= 1e-12"""
    indptr, indices = graph
    Z, _, G, att = ref.tolerance_inputs(320, 320, K, dh)
    r = ref.restate64(indptr, indices, Z, att, K, G=G, exact=True)
    out, G_Z, G_att = _autograd(indptr, indices, Z, att, K, G, ref.SLOPE)
    for what, got, want in (("out", r["out"], out), ("G_Z", r["G_Z"], G_Z), ("G_att", r["G_att"], G_att)):
        d = ref.relerr(got, want)
        print(f"[gat] restatement against autograd K={K} dh={dh} {what}: {d:.3e}")
        assert d <= 1e-12, (what, d)


@pytest.mark.parametrize("K,dh", [(1, 1), (5, 1), (3, 7), (1, 41), (4, 32), (2, 65), (1, 128), (8, 32), (16, 64)])
def test_twin_is_close_to_the_restatement(graph, K, dh):
    """on the tolerance inputs the fp32 twin is within 1e-5 of the restatement in every output; if it is not, the input is
    at fault, not a kernel"""
    indptr, indices = graph
    Z, _, G, att = ref.tolerance_inputs(320, 320, K, dh)
    want = ref.restate64(indptr, indices, Z, att, K, G=G)
    twin = ref.twin32(indptr, indices, Z, att, K, G=G)
    for what in ref.NAMES:
        d = ref.relerr(twin[what], want[what])
        print(f"[gat] twin against restatement K={K} dh={dh} {what}: {d:.3e}")
        assert d <= 1e-5, ("the input is ill-conditioned for the device tests' bar", what, d)


def test_rectangular_restatement_leaves_the_destination_term_out():
    """200 destinations x 320 sources: G_Z has one row per source and no ds_dst term; G_att[0] sums over destinations"""
    indptr, indices = ref.kernel_graph(200, 320)
    Z, Z_dst, G, att = ref.tolerance_inputs(200, 320, 4, 32)
    r = ref.restate64(indptr, indices, Z, att, 4, G=G, Z_dst=Z_dst, exact=True)
    assert r["G_Z"].shape == (320, 128) and r["ds_dst"].shape == (200, 4) and r["ds_src"].shape == (320, 4)
    want = (r["ds_src"][ref.UNREFERENCED][:, None] * att.astype(np.float64).reshape(2, 4, 32)[1]).reshape(-1)
    np.testing.assert_array_equal(r["G_Z"][ref.UNREFERENCED], want)          # ds_src of an unreferenced column is 0
    assert not r["G_Z"][ref.UNREFERENCED].any()


def test_attention_with_zero_att_is_the_row_mean(graph):
    indptr, indices = graph
    Z, _, _, att = ref.tolerance_inputs(320, 320, 4, 8)
    r = ref.restate64(indptr, indices, Z, np.zeros_like(att), 4, exact=True)
    assert ref.relerr(r["out"], ref.row_mean(indptr, indices, Z)) <= 1e-14


# ---- the helpers of test_gpu_gat_edges.py ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("K,dh", [(3, 7), (4, 32), (1, 41), (2, 65)])
def test_injected_intermediates_leave_the_plain_path_alone(graph, K, dh, dtype):
    """attention() fed its own s_dst, s_src, lse and D, or asked for the row scales, gives the bits it gives without: the
    injectable scalars replace the intermediates and touch nothing else, square and rectangular"""
    for (indptr, indices), n in ((graph, 320), (ref.kernel_graph(200, 320), 200)):
        Z, Z_dst, G, att = ref.tolerance_inputs(n, 320, K, dh)
        kw = dict(G=G, Z_dst=None if n == 320 else Z_dst, dtype=dtype)
        with np.errstate(over="ignore"):
            plain = ref.attention(indptr, indices, Z, att, K, **kw)
            fed = ref.attention(indptr, indices, Z, att, K, s_dst=plain["s_dst"], s_src=plain["s_src"], lse=plain["lse"],
                                D=plain["D"], score_cols=indices, scales=dtype is np.float64, **kw)
        for what in ref.NAMES + ("alpha",):
            assert plain[what].dtype == fed[what].dtype == dtype
            np.testing.assert_array_equal(plain[what].view(np.uint8), fed[what].view(np.uint8), err_msg=what)


def test_injected_intermediates_are_used():
    """each injected array reaches what is computed from it: lse + log 2 halves alpha and with it out, D = 0 leaves
    ds = alpha dalpha lrelu', s_src = 0 with s_dst = 0 makes every row the plain mean"""
    indptr, indices = ref.kernel_graph()
    Z, _, G, att = ref.tolerance_inputs(320, 320, 4, 8)
    r = ref.restate64(indptr, indices, Z, att, 4, G=G, exact=True)
    half = ref.restate64(indptr, indices, Z, att, 4, G=G, exact=True, lse=r["lse"] + np.log(2.0))
    assert ref.relerr(2 * half["out"], r["out"]) <= 1e-14
    noD = ref.restate64(indptr, indices, Z, att, 4, G=G, exact=True, D=np.zeros((320, 4)))
    rows = np.repeat(np.arange(320), np.diff(indptr.astype(np.int64)))
    assert ref.relerr(noD["ds_dst"] - r["ds_dst"], r["D"] * ref._segsum(r["alpha"] * np.where(
        r["s_dst"][rows] + r["s_src"][indices] > 0, 1.0, ref.SLOPE), indptr)) <= 1e-12
    flat = ref.restate64(indptr, indices, Z, att, 4, exact=True, s_dst=np.zeros((320, 4)), s_src=np.zeros((320, 4)))
    assert ref.relerr(flat["out"], ref.row_mean(indptr, indices, Z)) <= 1e-14


def test_rowdist_scales_and_exact_zeros():
    want = np.array([[1.0, -1.0], [0.0, 0.0], [1e-3, 0.0]])
    scale = np.array([[10.0, 10.0], [0.0, 0.0], [1e-3, 0.0]])
    got = want + np.array([[1e-3, 0.0], [0.0, 0.0], [1e-6, 0.0]])
    np.testing.assert_allclose(ref.rowdist(got, want, scale), [1e-4, 0.0, 1e-3], rtol=1e-9)
    assert ref.rowerr(got, want, scale) == (2, pytest.approx(1e-3))
    got[1, 1] = 1e-30                                     # nothing adds up to this element: it must be exact
    assert ref.rowerr(got, want, scale) == (1, np.inf)
    assert ref.rowerr(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3))) == (-1, 0.0)


def test_long_graph_has_its_long_rows_on_either_side():
    """kernel_graph_long: the rows on either side of one, two and three chunks are in F, through the transpose in F^T, and
    the other side of either orientation stays short; one duplicated column, one unreferenced column, an empty last row"""
    indptr, indices = ref.kernel_graph_long()
    special = [0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 1000, 4097]
    deg = np.diff(indptr.astype(np.int64))
    assert indptr.size - 1 == 320 and int(indptr[-1]) < 10_000
    assert deg[:13].tolist() == special and deg[13] == 3 and deg[319] == 0 and 1 <= deg[14:319].min() and deg[14:319].max() <= 8
    b = int(indptr[ref.LONG_DUPLICATE_ROW])
    assert indices[b] == indices[b + 1]
    t_indptr, t_indices = ref.transpose_pattern(indptr, indices, 320)
    tdeg = np.diff(t_indptr.astype(np.int64))
    assert tdeg[ref.UNREFERENCED] == 0 and (np.delete(tdeg, ref.UNREFERENCED) > 0).all() and tdeg.max() < 64
    assert tdeg.tolist() == np.bincount(indices, minlength=320).tolist()
    # the other orientation, as the tests build it: F = the transpose, F^T = the graph itself, rows in increasing order
    g = ref.edge_graphs()["longT"]
    np.testing.assert_array_equal(g[0], t_indptr)
    np.testing.assert_array_equal(g[1], t_indices)
    back_indptr, back_indices = ref.transpose_pattern(g[0], g[1], 320)
    assert np.diff(back_indptr.astype(np.int64)).tolist() == deg.tolist()
    for r in range(320):                                    # the same entries, sorted within the row
        assert back_indices[back_indptr[r]:back_indptr[r + 1]].tolist() == sorted(indices[indptr[r]:indptr[r + 1]].tolist())


def test_probe_block_lists_every_source_once():
    indptr, indices, n_src = ref.probe_block()
    assert np.diff(indptr.astype(np.int64)).tolist() == [64, 65, 129, 193, 4097] and n_src == 4548
    assert sorted(indices.tolist()) == list(range(n_src)) and (np.diff(indices[:64].astype(np.int64)) < 0).any()
    assert [ref.probe_positions(L) for L in (64, 65, 4097)] == [[0, 62, 63], [0, 63, 64], [0, 63, 64, 127, 128, 4095, 4096]]
    seen = {(r, p) for t in range(ref.PROBE_SLOTS) for r, p in enumerate(ref.probe_hot(t)[0])}
    assert seen == {(r, p) for r, L in enumerate(ref.PROBE_ROWS) for p in ref.probe_positions(L)}


def test_shape_list_reaches_every_variant():
    """head_geometry_for and MGGCN_GAT_DISPATCH of csrc/gat.hip recomputed: the aligned shapes and the misaligned runs of
    test_gpu_gat_edges.py select all five (VEC, NT, U) variants, use every tile count from 1 to 5 and 16, and mask lanes
    on the float4 path"""
    runs = [(dh, dh % 4 == 0) for _, dh in ref.EDGE_SHAPES] + [(dh, False) for _, dh in ref.EDGE_MISALIGNED]
    geo = [ref.head_geometry_for(dh, vec) for dh, vec in runs]
    assert {v for v, _ in geo} == {(4, 1, 4), (4, 4, 1), (1, 1, 4), (1, 4, 2), (1, 16, 1)}
    assert {nt for _, nt in geo} >= {1, 2, 3, 4, 5, 16}
    assert {nt for v, nt in geo if v == (1, 4, 2)} == {2, 3, 4} and {nt for v, nt in geo if v == (4, 4, 1)} >= {2, 4}
    assert all(nt <= v[1] for v, nt in geo)
    assert any(vec and (dh // 4) & (dh // 4 - 1) for dh, vec in runs if dh <= 256)      # float4 lanes beyond dh masked
    assert {ref.head_geometry_for(dh, dh % 4 == 0)[0] for _, dh in ref.EDGE_RECT} == {v for v, _ in geo}
    assert all(K <= 16 and K * dh <= 1024 for K, dh in ref.EDGE_SHAPES)
    for dh, vec, want in ((1, False, ((1, 1, 4), 1)), (64, False, ((1, 1, 4), 1)), (65, False, ((1, 4, 2), 2)),
                          (256, True, ((4, 1, 4), 1)), (260, True, ((4, 4, 1), 2)), (1024, True, ((4, 4, 1), 4)),
                          (1024, False, ((1, 16, 1), 16)), (257, False, ((1, 16, 1), 5))):
        assert ref.head_geometry_for(dh, vec) == want, dh


def test_row_bar_is_eight_times_the_twin():
    """ROW_TOL against what it was derived from: over every case of the variant test the fp32 twin's worst row-scaled
    distance from the exact restatement is within an eighth of the bar, and the bar is no looser than sixteen times it"""
    worst = dict.fromkeys(ref.NAMES, 0.0)
    for name, K, dh in ref.edge_cases():
        c = ref.edge_case(name, K, dh)
        for what in ref.NAMES:
            assert ref.relerr(c["twin"][what], c["want"][what]) <= 1e-4 / 3
            worst[what] = max(worst[what], ref.rowerr(c["twin"][what], c["want"][what], c["scale"][what])[1])
    print("[gat] worst row-scaled twin distance per output: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert ref.ROW_TOL / 16 <= max(worst.values()) <= ref.ROW_TOL / 8, worst
    assert max(worst.values()) == pytest.approx(ref.TWIN_ROW_MEASURED, rel=0.05)


@pytest.mark.parametrize("K,dh", ref.EDGE_SHAPES)
def test_an_off_by_one_in_a_long_row_is_four_bars_away(K, dh):
    """the condition on ROW_TOL: the restatement with the last entry of every row of 65 or more entries removed, with the
    first entry of its last chunk removed, and with the scores at positions 63 and 64 swapped, is at least 4 x ROW_TOL away
    in one of out, lse, ds_dst, ds_src, G_Z on the row-scaled measure.  The two removals are asked for more: every one of
    the nine long rows, the 4097-entry one included, is that far away in its own out, lse or ds_dst"""
    indptr, indices, _ = ref.edge_graphs()["long"]
    c = ref.edge_case("long", K, dh)
    args, kw = (c["Z"], c["att"], K), dict(G=c["G"], exact=True)
    long_rows, last = ref.long_row_positions(indptr, "last")
    assert long_rows.tolist() == [4, 5, 6, 7, 8, 9, 10, 11, 12]
    mutants = {"last": ref.restate64(*ref.without_entries(indptr, indices, last), *args, **kw),
               "chunk": ref.restate64(*ref.without_entries(indptr, indices, ref.long_row_positions(indptr, "chunk")[1]), *args, **kw),
               "swap": ref.restate64(indptr, indices, *args, score_cols=ref.swapped_scores(indptr, indices), **kw)}
    for what, r in mutants.items():
        moved = {nm: ref.rowdist(r[nm], c["want"][nm], c["scale"][nm]) for nm in ("out", "lse", "ds_dst", "ds_src", "G_Z")}
        per_row = np.max([moved[nm][long_rows] for nm in ("out", "lse", "ds_dst")], axis=0)
        print(f"[gat] K={K} dh={dh} {what}: " + ", ".join(f"{nm} {v.max() / ref.ROW_TOL:.1f}" for nm, v in moved.items())
              + f" bars; long rows {np.round(per_row / ref.ROW_TOL, 1).tolist()}")
        assert max(v.max() for v in moved.values()) >= 4 * ref.ROW_TOL, what
        if what != "swap":
            assert (per_row >= 4 * ref.ROW_TOL).all(), (what, per_row)


@pytest.mark.parametrize("K,dh", [(4, 32), (3, 7)])
def test_probes_and_stress_cases_are_well_conditioned(K, dh):
    """the crafted-scalar cases of test_gpu_gat_edges.py: the restatement says what the probes claim (out = one row of Z,
    lse = 40; G_Z = one row of G, ds_src = slope G_p . Z_j), and the twin is within an eighth of the bar wherever the
    device test asks for that -- everywhere but ds_src and G_Z of the stress cases, whose sources have one entry each (a
    single term relative to |dalpha| + |D|, which the dot product's own rounding can exceed by more) and stay within the bar"""
    def twin(c, nm):
        return ref.rowerr(c["twin"][nm], c["want"][nm], c["want"]["scale"][nm])[1]
    for t in range(ref.PROBE_SLOTS):
        c = ref.forward_probe_case(t, K, dh)
        assert ref.rowerr(c["want"]["out"], c["Z"][c["hot"]], c["want"]["scale"]["out"])[1] <= 1e-9
        assert np.abs(c["want"]["lse"] - 40).max() <= 1e-12
        assert max(twin(c, "out"), twin(c, "lse")) <= ref.ROW_TOL / 8
        c = ref.backward_src_probe_case(t, K, dh)
        assert ref.rowerr(c["want"]["G_Z"], c["G"][c["hot"]], c["want"]["scale"]["G_Z"])[1] <= 1e-9
        assert ref.rowerr(c["want"]["ds_src"], c["dots"], c["want"]["scale"]["ds_src"])[1] <= 1e-9
        assert max(twin(c, "G_Z"), twin(c, "ds_src")) <= ref.ROW_TOL / 8
    for kind in ref.STRESS_KINDS:
        c = ref.stress_case(kind, K, dh)
        d = {nm: twin(c, nm) for nm in ("out", "lse", "D", "ds_dst", "ds_src", "G_Z")}
        print(f"[gat] stress {kind} K={K} dh={dh}: twin " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()))
        assert max(d[nm] for nm in ("out", "lse", "D", "ds_dst")) <= ref.ROW_TOL / 8 and max(d.values()) <= ref.ROW_TOL, d
        assert np.abs(ref.alpha_row_sums(c["indptr"], c["indices"], c["s_src"], c["want"]["lse"]) - 1).max() <= 1e-12
        x = c["s_src"][c["indices"][-4097:], 0]                       # the scores along the longest row
        assert x.min() == (7.5 if kind == "constant" else -80.0) and x.max() == (7.5 if kind == "constant" else 80.0)
        assert {"ascending": (np.diff(x) > 0).all(), "descending": (np.diff(x) < 0).all(), "constant": True,
                "late peak": x[-1] == 80.0 and (x[:-1] == -80.0).all()}[kind]


@pytest.mark.parametrize("sizes,heads,what", [
    ([16, 30, 5], 4, "not divisible"),             # 30 columns into 4 heads
    ([16, 32, 6], [4, 4], "not divisible"),        # the last layer's 6 into 4
    ([16, 34, 5], 17, "heads"),                    # more than 16 heads
    ([16, 32, 5], 0, "heads"),
    ([16, 2048, 5], 8, "1024"),                    # wider than the kernels take
    ([16, 32, 5], [4], "lists"),                   # one entry for two layers
    ([16, 32, 5], 2.5, "heads"),
])
def test_constructor_refusals_need_no_gpu(pkg, sizes, heads, what):
    n = 8
    A = pkg.csr_matrix(np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32), np.ones(n, dtype=np.float32), n)
    with pytest.raises(ValueError, match=what):
        pkg.gat(A, sizes, heads=heads)


def test_constructor_refuses_an_unknown_loss_and_a_rectangular_matrix(pkg):
    n = 8
    A = pkg.csr_matrix(np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32), np.ones(n, dtype=np.float32), n)
    with pytest.raises(ValueError, match="loss"):
        pkg.gat(A, [16, 32, 5], loss="hinge")
    R = pkg.csr_matrix(np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32), np.ones(n, dtype=np.float32), n + 3)
    with pytest.raises(ValueError, match="square"):
        pkg.gat(R, [16, 32, 5])


def test_heads_default_gives_the_last_layer_one_head(pkg):
    from importlib import import_module
    gat = import_module(pkg.__name__ + ".gat")
    assert gat.check_heads([16, 32, 32, 7], 4) == [4, 4, 1]
    assert gat.check_heads([16, 32, 32, 8], [2, 4, 8]) == [2, 4, 8]
