"""The host side of the attention layout tests, checked without a GPU: the graph has the rows it promises, the layout table
gives the operands that meet in one call different leading dimensions and reaches every kernel variant and both forms of
every entry point that has two, the guards are sized by the rule, the checks (a)-(d) catch every named addressing mistake
on a numpy model of the addressing, and the fp32 twins stay under the families' bars on the new graph."""
import numpy as np
import pytest

import gat_alpha_ref as ar
import gat_layout_ref as lr
import gat_ref as ref
import gatv2_ref as v2
from guarded import IN_NAN32, OUT_NAN32, Guarded

CASES = [(f, K, dh) for f in lr.FAMILIES for K, dh in lr.SHAPES[f]]


# ---- the graph -------------------------------------------------------------------------------------------------------------------------
def test_graph_has_the_rows_it_promises():
    indptr, indices = lr.layout_graph()
    a, b = lr.layout_graph()
    np.testing.assert_array_equal(a, indptr), np.testing.assert_array_equal(b, indices)      # a fixed seed
    n, lens = indptr.size - 1, np.diff(indptr.astype(np.int64))
    assert (n, lr.N_SRC) == (37, 53) and n % 4 == 1 and lr.N_SRC % 4 == 1
    assert {0, 1, 2, 63, 64, 65, 129, 200} <= set(lens.tolist())
    assert 0 in lens[-4:] and 200 in lens[-4:] and lens[-1] == 200       # the one row of the last workgroup is the longest
    row = indices[int(indptr[lr.DUPLICATE_ROW]):int(indptr[lr.DUPLICATE_ROW + 1])]
    assert row.size == 3 and row[0] == row[1]
    assert indices.max() < lr.N_SRC and 300 <= indices.size <= 999      # a few hundred entries
    t_indptr, _ = ref.transpose_pattern(indptr, indices, lr.N_SRC)
    t_lens = np.diff(t_indptr.astype(np.int64))
    assert t_lens[lr.UNREFERENCED] == 0 and (np.delete(t_lens, lr.UNREFERENCED) > 0).all() and t_lens[-1] > 0


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
def test_shapes_come_from_the_families_lists():
    assert lr.SHAPES["gat"] == ref.EDGE_RECT + [(16, 4)] and lr.SHAPES["gatv2"] == v2.RECT_SHAPES + [(16, 4)]
    assert lr.SHAPES["gat-drop"] == lr.SHAPES["gat"] and lr.ONE_PADDED_SHAPE in lr.SHAPES["gat"] + lr.SHAPES["gatv2"]


def test_the_rows_of_the_table_follow_their_rules():
    L = lr.LAYOUTS
    assert all(v == (0, 0) for v in L["contiguous"].values())
    vp = L["vec-padded"]
    pads = [vp[k][0] for k in lr.DENSE if k != "alpha"]
    offs = [vp[k][1] for k in lr.DENSE + ("att", "G_att")]
    assert len(set(pads)) == len(pads) and all(x and x % 4 == 0 for x in pads)
    assert len(set(offs)) == len(offs) and all(x % 4 == 0 for x in offs) and all(v[1] % 4 == 0 for v in vp.values())
    od = L["odd-ld"]
    pads = [od[k][0] for k in lr.DENSE if k != "alpha"]
    assert len(set(pads)) == len(pads) and all(x % 2 == 1 for x in pads) and od["alpha"][0] % 2 == 1
    assert all(v[1] == 0 for v in od.values())
    ob = L["off-base"]
    pads = [ob[k][0] for k in lr.DENSE if k != "alpha"]
    assert len(set(pads)) == len(pads)
    assert all(ob[k][1] in (1, 2, 3) for k in lr.DENSE + lr.FLAT if k != "rec") and ob["rec"][1] == "rec"
    for x in lr.DENSE:
        row = L[f"one-padded[{x}]"]
        assert row[x] == (4, 0) and all(v == (0, 0) for k, v in row.items() if k != x)


@pytest.mark.parametrize("family,K,dh", CASES)
def test_leading_dimensions_that_meet_in_a_call_differ(family, K, dh):
    """in every layout row but "contiguous" and "one-padded"; in "halves" the two halves of one buffer share theirs and every
    other pair differs.  rec keeps its alignment and, in "vec-padded", lda % 4 == 0"""
    nnz = lr.case(family, K, dh)["nnz"]
    for layout in ("vec-padded", "odd-ld", "off-base") + (("halves",) if family == "gatv2" else ()):
        p = lr.plan(family, K, dh, layout, nnz)
        for call, (lds, _, _, _, _) in lr.CALLS[family].items():
            for i, x in enumerate(lds):
                for y in lds[i + 1:]:
                    shared = layout == "halves" and {x, y} <= {"Zs", "Zd", "G_Zs", "G_Zd", "G_Zs_r"}       # ld = 2 K dh
                    assert (p[x].ld == p[y].ld) == shared, (layout, call, x, y, p[x].ld)
        assert p["rec"].off % lr.rec_offset(family) == 0
    assert lr.plan(family, K, dh, "vec-padded", nnz)["alpha"].ld % 4 == 0
    assert lr.plan(family, K, dh, "vec-padded", nnz)["alpha"].ld > K
    q = lr.plan(family, K, dh, "off-base", nnz)["rec"]
    assert q.off and (q.off * 4) % (8 if family == "gatv2" else 16) == 0
    if family == "gatv2":
        assert (q.off * 4) % 16 != 0                     # 8-byte aligned and no more: all the ABI asks for


@pytest.mark.parametrize("family", lr.FAMILIES)
def test_the_table_reaches_every_variant_and_both_forms(family):
    """rows16, head_geometry_for and gat_dispatch restated (gat_layout_ref.classify): over (layout, shape) every sparse entry
    point reaches all five (VEC, NT, U) variants -- so its float4 and its element form --, mggcn_gat_alpha_f32 both store
    forms and mggcn_gatv2_alpha_f32 all five variants; every float4 shape also runs on the element path by leading
    dimension alone ("odd-ld") and by base alone ("off-base"), and on the float4 path with padded rows ("vec-padded")"""
    reached = {}
    for K, dh in lr.SHAPES[family]:
        nnz = lr.case(family, K, dh)["nnz"]
        p0 = lr.plan(family, K, dh, "contiguous", nnz)
        for layout in lr.layouts_for(family, K, dh):
            p = lr.plan(family, K, dh, layout, nnz)
            for call in lr.CALLS[family]:
                form = lr.classify(family, call, K, dh, p)
                reached.setdefault(call, set()).add(form)
                base = lr.classify(family, call, K, dh, p0)
                if call in lr.SPARSE or (family == "gatv2" and call == "alpha"):
                    assert form in lr.VARIANTS
                    if dh % 4 == 0:
                        assert base[0] == 4
                        assert form[0] == (1 if layout in ("odd-ld", "off-base") else 4), (layout, call, K, dh)
                    else:
                        assert form == base and form[0] == 1
                if family != "gatv2" and call == "alpha" and K % 4 == 0:
                    assert form == ("KV", 1 if layout in ("odd-ld", "off-base") else 4), (layout, K)
            same = lr.same_bits_as_contiguous(family, K, dh, p, p0)
            assert all(same.values()) == (dh % 4 != 0 or layout not in ("odd-ld", "off-base")), (layout, K, dh)
    for call in lr.SPARSE:
        assert reached[call] == set(lr.VARIANTS), (call, reached[call])
    if family == "gatv2":
        assert reached["alpha"] == set(lr.VARIANTS)
    else:
        assert reached["alpha"] == {("KV", 4), ("KV", 1)}
    for call, (_, deciders, _, _, _) in lr.CALLS[family].items():
        if deciders == "one":
            assert reached[call] == {"one"}


def test_the_restated_geometry_is_the_sources():
    """the variant of every shape on aligned operands, as the comments of gat_ref.EDGE_RECT / gatv2_ref.RECT_SHAPES list them"""
    want = {(4, 32): (4, 1, 4), (1, 260): (4, 4, 1), (3, 7): (1, 1, 4), (1, 130): (1, 4, 2), (2, 65): (1, 4, 2), (1, 257): (1, 16, 1),
            (16, 4): (4, 1, 4)}
    for family in lr.FAMILIES:
        for K, dh in lr.SHAPES[family]:
            p0 = lr.plan(family, K, dh, "contiguous", 10)
            assert lr.classify(family, "forward", K, dh, p0) == want[(K, dh)]


# ---- the guards ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,K,dh", CASES)
def test_guards_follow_the_sizing_rule(family, K, dh):
    """with ANY leading dimension of the plan used on ANY operand all its rows stay inside the allocation: the guard behind
    is at least rows x (largest ld - own ld) plus one row; the front guard is Guarded's own"""
    c = lr.case(family, K, dh)
    for layout in lr.layouts_for(family, K, dh) + (["halves"] if family == "gatv2" else []):
        p = lr.plan(family, K, dh, layout, c["nnz"])
        top = lr.largest_ld(p)
        for name, q in p.items():
            if q.view is not None:
                continue
            assert q.tail_rows * q.ld >= q.rows * (top - q.ld) + q.ld, (layout, name)
            assert q.tail_rows * q.ld >= lr.guard_need(p, name, c["nnz"])
    p = lr.plan(family, K, dh, "vec-padded", c["nnz"])
    q = p["out"]
    g = Guarded(q.rows, q.cols, q.ld, q.off, output=True, tail_rows=q.tail_rows, host=True)
    assert g.host.size - (g.start + q.rows * q.ld) >= q.tail_rows * q.ld and g.start == g.head + q.off
    assert g.start + (q.rows - 1) * lr.largest_ld(p) + q.cols <= g.host.size


def test_guarded_without_a_tail_is_what_it_was():
    """tail_rows=None: one front-guard's worth behind, the sizes and the fill of before"""
    g = Guarded(5, 7, 9, 2, logical=np.arange(35, dtype=np.float32).reshape(5, 7), host=True)
    assert g.head == 64 and g.start == 66 and g.host.size == 66 + 45 + 64 and g.mask.sum() == 35
    assert (g.host[~g.mask] == IN_NAN32).all()
    np.testing.assert_array_equal(g.values(), np.arange(35, dtype=np.float32).reshape(5, 7))
    g = Guarded(5, 7, 9, 2, output=True, tail_rows=20, host=True)
    assert g.host.size == 66 + 45 + 180 and (g.host == OUT_NAN32).all()
    assert Guarded(5, 7, 9, 2, output=True, tail_rows=1, host=True).host.size == 66 + 45 + 64


# ---- the checks have teeth -------------------------------------------------------------------------------------------------------------------
MODEL_SHAPES = [("gat", 4, 32), ("gat", 3, 7), ("gat-drop", 4, 32), ("gatv2", 4, 32), ("gatv2", 3, 7)]


@pytest.mark.parametrize("family,K,dh", MODEL_SHAPES)
def test_the_model_without_a_mutation_passes_every_check(family, K, dh):
    for layout in lr.layouts_for(family, K, dh):
        b, p = lr.run_model(family, K, dh, layout)
        assert lr.violations(b, p) == [], layout
        c = lr.case(family, K, dh)
        for name in lr.compared(family):
            rn = lr.result_name(family, name)
            np.testing.assert_array_equal(b[name].values(), c["want"][rn].astype(np.float32).reshape(p[name].rows, -1))


@pytest.mark.parametrize("family,K,dh", MODEL_SHAPES)
@pytest.mark.parametrize("mutation", lr.MUTATIONS)
def test_every_mutation_trips_a_check(family, K, dh, mutation):
    """each named addressing mistake fails at least one of (a)-(d) in every row of the table where the mistake is one (with
    equal leading dimensions a swap of two is none), never leaves the allocation, and a one-padded row names the operand"""
    swap = mutation in lr.MUTATIONS[:2]
    for layout in ("vec-padded", "odd-ld", "off-base") + (() if swap else ("contiguous",)):
        b, p = lr.run_model(family, K, dh, layout, mutation)
        found = lr.violations(b, p)
        print(f"[gat-layouts] {family} K={K} dh={dh} {layout} '{mutation}': {sorted({(v[0], v[1]) for v in found})}")
        assert found and {v[0] for v in found} <= set("abcd"), (layout, mutation)
    if (K, dh) == lr.ONE_PADDED_SHAPE and swap:
        x, y = ("G", "Zs") if mutation == lr.MUTATIONS[0] else ("out", "Zs")
        for padded in (x, y):
            b, p = lr.run_model(family, K, dh, f"one-padded[{padded}]", mutation)
            assert lr.violations(b, p), (padded, mutation)
        others = [z for z in lr.dense_operands(family) if z not in (x, y)]
        b, p = lr.run_model(family, K, dh, f"one-padded[{others[0]}]", mutation)
        assert lr.violations(b, p) == []                 # the two leading dimensions are equal there: no mistake to see


# ---- the twins on the new graph ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", lr.FAMILIES)
def test_twins_stay_under_the_bars_on_this_graph(family):
    """the fp32 twin of every family against its exact restatement on the 37 x 53 graph: within an eighth of the family's
    bar for every output (gatv2_ref.bar_rule leaves the bar where it is then), and what TWIN_MEASURED records"""
    worst = {}
    for K, dh in lr.SHAPES[family]:
        for name, (d, bar) in lr.twin_errors(family, K, dh).items():
            print(f"[gat-layouts] {family} twin K={K} dh={dh} {name}: {d:.3e} (bar {bar:.1e})")
            assert d <= bar / 8, (family, K, dh, name, d, bar)
            if bar == ref.ROW_TOL:
                assert v2.bar_rule(d) == ref.ROW_TOL
            worst[name] = max(worst.get(name, 0.0), d)
    print(f"[gat-layouts] {family} twin worst: " + ", ".join(f"{k}={v:.2e}" for k, v in worst.items()))
    rec = lr.TWIN_MEASURED[family]
    assert set(rec) == set(worst)
    for name, d in worst.items():
        assert 0.9 * rec[name] <= d <= 1.02 * rec[name], (family, name, d, rec[name])
    assert ar.BAR <= ref.ROW_TOL
