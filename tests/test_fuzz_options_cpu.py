"""The option fuzz without a GPU: which cases of fuzz_ref.py the device may be held to (admission), what the admitted set
covers, and the refusals no device test may trigger.

Admission is the suite's own rule (test_gpu_gat_edges.py: "the input is ill-conditioned for this bar"), decided with the
reference alone: the reference runs its two epochs at both of its precisions from identical state -- oracle.Gcn(f64acc=True)
against f64acc=False for gcn, the fp64 restatement of the attention against its fp32 twin for gat --, the loss must be
finite, and every line of fuzz_ref.distances(), the measure of test_gpu_fuzz_options.py, must stay within a third of its bar.
A third run takes every activation that lies within 8 x (fuzz_ref.SIGN_FACTOR) of zero -- 8 x its largest difference between the
held run, the other precision from the same state, and the other precision running free, which reaches the second epoch by its
own Adam step as the device does -- on the other side of zero in the backward pass and is held to the same third: leaky_relu'
jumps by 0.99 there, and one such element is enough to move a gradient by 4e-3.  For gat a fourth run is the twin with D = G . out
summed in another order than dalpha (gat_ref.oracle_gat._D), held to the same third.  The second epoch is held twice: from the held
run's own Adam step and from the free-running other precision's.
A seed that fails is mended in the generator or listed in fuzz_ref.EXCLUDED, at most fuzz_ref.MAX_EXCLUDED per family; an excluded
seed is run all the same and must fail, so the list cannot hold a seed that the reference alone does not refuse."""
import numpy as np
import pytest

import fuzz_ref as fz
import gat_ref

CASES = {"gcn": fz.gcn_case, "gat": fz.gat_case}
TOL_LOSS = fz.TOL
_made = {}


def _case(family, seed):
    if (family, seed) not in _made:
        _made[(family, seed)] = CASES[family](seed)
    return _made[(family, seed)]


def _admitted(family):
    return [_case(family, s) for s in fz.admitted(family)]


def _as_got(case, epoch, res):
    after = bool(case["opt"]["step"]) and epoch == 1
    got = dict(loss=res["loss"], score=res["score"], grads=res["grads_after"] if after else res["grads"], params=res["params"],
               per=res.get("per"))
    if case["opt"]["loss"] == "bce":
        got["conf"] = res["per"]["train"][2]
    return got


def admission(case, oracle):
    """every line of the measure with its epoch, the second epoch started once from the held run's own Adam step and once from
    the free-running other precision's: the device arrives there by a third, and which activations lie next to zero then
    depends on the last bits of that state"""
    lines = _admission(case, oracle, False)
    return lines + [(e, name + " (second epoch from the other precision's step)") + tuple(rest)
                    for e, name, *rest in _admission(case, oracle, True) if e == 1]


def _admission(case, oracle, from_free):
    held, other, signs = fz.reference(case, oracle), fz.reference(case, oracle, other=True), fz.reference(case, oracle)
    free = fz.reference(case, oracle, other=True)               # never re-synchronised: it reaches epoch 2 by its own Adam step
    order = fz.reference(case, oracle, reorder=True) if case["family"] == "gat" else None
    lines = []
    for epoch in range(2):
        if from_free and epoch == 1:
            held.set_state(free.get_state())
        state = held.get_state()
        other.set_state(state)
        signs.set_state(state)
        if order is not None:
            order.set_state(state)
        with fz.recorded_signs(oracle) as a:
            want = held.epoch()
        with fz.recorded_signs(oracle) as b:
            twin = other.epoch()
        with fz.recorded_signs(oracle) as c:
            free.epoch()
        with fz.flipped_signs(oracle, fz.sign_margins(a, b, c)) as f:
            flip = signs.epoch()
        if not (np.isfinite(want["loss"]) and np.isfinite(twin["loss"])):
            return lines + [(epoch, "loss is not finite", float("inf"), TOL_LOSS, False)]
        lines += [(epoch,) + ln for ln in fz.distances(case, epoch, _as_got(case, epoch, twin), want)]
        if order is not None:
            lines += [(epoch, f"{ln[0]} with D summed in another order") + ln[1:]
                      for ln in fz.distances(case, epoch, _as_got(case, epoch, order.epoch()), want)]
        if f.flipped:
            lines += [(epoch, f"{ln[0]} with {f.flipped} sign(s) flipped") + ln[1:] for ln in fz.distances(case, epoch, _as_got(case, epoch, flip), want)]
    return lines


@pytest.mark.parametrize("seed", range(fz.SEEDS))
@pytest.mark.parametrize("family", ["gcn", "gat"])
def test_admission(oracle, family, seed):
    case = _case(family, seed)
    lines = admission(case, oracle)
    bad = [(e, name, value, bar) for e, name, value, bar, scalable in lines if not value <= (bar / 3 if scalable else bar)]
    if seed in fz.EXCLUDED[family]:                              # only a seed that the reference alone refuses may be excluded
        assert fz.EXCLUDED[family][seed] and bad, (fz.describe(case), "is excluded but passes admission")
        return
    for key, (q, value, bar) in sorted(fz.worst([ln[1:] for ln in lines]).items()):
        print(f"[fuzz admission] {family} seed {seed} {key}: {value:.3e} (bar {bar:g})")
    assert not bad, (fz.describe(case), bad)


@pytest.mark.parametrize("family", ["gcn", "gat"])
def test_exclusions_stay_under_the_cap(family):
    assert len(fz.EXCLUDED[family]) <= fz.MAX_EXCLUDED
    assert all(0 <= s < fz.SEEDS and isinstance(r, str) and r for s, r in fz.EXCLUDED[family].items())
    assert len(fz.admitted(family)) == fz.SEEDS - len(fz.EXCLUDED[family]) >= fz.SEEDS - fz.MAX_EXCLUDED


@pytest.mark.parametrize("family", ["gcn", "gat"])
def test_cases_depend_on_the_seed_alone(family):
    for seed in (0, 7, 23):
        a, b = CASES[family](seed), CASES[family](seed)
        assert fz.describe(a) == fz.describe(b)
        for k in ("ip", "ix", "X", "Y"):
            assert np.array_equal(a[k], b[k])


# ---- coverage ------------------------------------------------------------------------------------------------------------------------------
def _count(cases, name, value):
    return sum(1 for c in cases if c["opt"][name] == value)


def test_every_value_of_every_gcn_option_occurs_and_every_pair_meets():
    cases = _admitted("gcn")
    names = sorted(fz.GCN_OPTIONS)
    for name in names:
        for value in fz.GCN_OPTIONS[name]:
            assert _count(cases, name, value) >= 3, (name, value)
    illegal = {("agg_dtype", "bf16", "hoist_first_aggregation", True)}
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            for va in fz.GCN_OPTIONS[a]:
                for vb in fz.GCN_OPTIONS[b]:
                    if (a, va, b, vb) in illegal:
                        assert not any(c["opt"][a] == va and c["opt"][b] == vb for c in cases)
                        continue
                    assert any(c["opt"][a] == va and c["opt"][b] == vb for c in cases), (a, va, b, vb)
    for n in fz.NS:
        assert sum(1 for c in cases if c["n"] == n) >= 3, n
    depths = [len(c["sizes"]) - 1 for c in cases]
    assert all(depths.count(d) >= 3 for d in (1, 2, 3, 4)), depths
    hidden = {w for c in cases for w in c["sizes"][1:-1]}
    assert {1, 2, 5, 33, 200} <= hidden, hidden


def test_gcn_corners():
    cases = _admitted("gcn")
    width1 = [c for c in cases if c["opt"]["norm"] == "layer" and 1 in c["sizes"][1:-1]]
    assert len(width1) >= 2, "a width-1 hidden layer under norm='layer'"
    assert sum(1 for c in cases if fz.hoist_effective(c)) >= 3, "hoisting that the model really switches on"
    assert any(c["opt"]["hoist_first_aggregation"] and c["facts"]["empty_F_rows"] for c in cases), "hoisting asked for on a graph that refuses it"
    assert any(fz.hoist_effective(c) and c["opt"]["dropout"] for c in cases)
    assert any(fz.hoist_effective(c) and c["opt"]["norm"] for c in cases)
    assert any(c["opt"]["loss"] == "bce" and c["sizes"][-1] == 2 for c in cases), "two-class bce"
    assert any(c["opt"]["agg_dtype"] == "bf16" and c["opt"]["norm"] and c["opt"]["dropout"] and c["opt"]["residual_layer"]
               for c in cases), "bf16 with norm, dropout and a residual branch"
    # both layer orders next to a norm, a residual branch and bf16
    for what in (lambda c: c["opt"]["norm"], lambda c: c["opt"]["residual_layer"], lambda c: c["opt"]["agg_dtype"] == "bf16"):
        orders = {o for c in cases if what(c) for o in fz.gemm_first(c)[:-1] + fz.gemm_first(c)[-1:]}
        assert orders == {True, False}, orders


@pytest.mark.parametrize("family", ["gcn", "gat"])
def test_every_graph_law_occurs(family):
    cases = _admitted(family)
    for law in fz.GRAPH_LAWS:
        assert sum(1 for c in cases if c["law"] == law) >= 3, law
    assert any(c["n"] == 8 for c in cases)
    assert sum(1 for c in cases if c["facts"]["empty_F_rows"]) >= 3
    assert sum(1 for c in cases if c["facts"]["never_gathered"]) >= 3


def test_gat_options_and_kernel_variants():
    cases = _admitted("gat")
    for name, values in fz.GAT_OPTIONS.items():
        for value in values:
            assert _count(cases, name, value) >= 3, (name, value)
    assert all(c["opt"]["attn_dropout"] == 0.0 for c in cases if c["opt"]["variant"] == "v2")
    for d in (1, 2, 3):
        assert sum(1 for c in cases if len(c["layers"]) == d) >= 3, d
    reached = {(c["opt"]["variant"], fz.layer_variant(dh)) for c in cases for _, dh in c["layers"]}
    assert reached == {(v, k) for v in ("v1", "v2") for k in fz.KERNEL_VARIANTS}, sorted(reached)
    for c in cases:                                              # the targeted variant is where the case says, and as the kernels pick it
        assert c["target"] in {fz.layer_variant(dh) for _, dh in c["layers"]}
        assert all(k * dh == w for (k, dh), w in zip(c["layers"], c["sizes"][1:]))
        assert all(dh < 257 for _, dh in c["layers"]) or c["n"] <= 520
    assert fz.layer_variant(260) == (4, 4, 1) and fz.layer_variant(257) == (1, 16, 1) and fz.layer_variant(256) == (4, 1, 4)
    assert fz.layer_variant(255) == (1, 4, 2) and fz.layer_variant(65) == (1, 4, 2) and fz.layer_variant(63) == (1, 1, 4)
    assert sum(1 for c in cases if c["facts"]["empty_F_rows"]) >= 3, "GAT cases with an empty row of F"
    lists = [c for c in cases if isinstance(c["heads"], list)]
    assert sum(1 for c in lists if c["heads"][-1] > 1) >= 3, "head lists whose last entry is above 1"
    assert any(16 in c["per_layer_heads"] for c in cases) and any(dh == 1 and k > 1 for c in cases for k, dh in c["layers"])
    v2_out = [w for c in cases if c["opt"]["variant"] == "v2" for w in c["sizes"][1:]]
    assert sum(1 for w in v2_out if w % 4 == 2) >= 2 and sum(1 for w in v2_out if w % 2) >= 2, v2_out
    assert sum(1 for c in cases if c["dup"]) >= 3


# ---- duplicates ------------------------------------------------------------------------------------------------------------------------------
def test_the_transposes_and_the_reference_keep_duplicates(oracle):
    """a duplicated entry of A is two entries of F = A^T in oracle.transpose and in gat_ref.transpose_pattern, and the
    reference model counts it twice: its logits differ from those on the same graph with the copy removed"""
    case = next(c for c in _admitted("gat") if c["dup"])
    r, col = case["dup"]
    ip, ix, n = case["ip"], case["ix"], case["n"]
    F = oracle.transpose(oracle.Csr(ip, ix, case["dv"], n))
    assert F.nnz == ix.size
    assert int((F.indices[int(F.indptr[col]):int(F.indptr[col + 1])] == r).sum()) == 2
    tip, tix = gat_ref.transpose_pattern(ip, ix, n)
    assert np.array_equal(tip, F.indptr) and np.array_equal(tix, F.indices)
    with_dup = fz.reference(case, oracle)
    single = dict(case)
    e = int(np.flatnonzero(ix[int(ip[r]):int(ip[r + 1])] == col)[0]) + int(ip[r])
    single["ix"] = np.delete(ix, e)
    single["ip"] = ip.astype(np.int64).copy()
    single["ip"][r + 1:] -= 1
    single["ip"] = single["ip"].astype(np.uint32)
    single["dv"] = case["dv"][:-1]
    without = fz.reference(single, oracle)
    a, b = with_dup.O.forward(case["X"]), without.O.forward(case["X"])
    assert np.abs(a[col] - b[col]).max() > 100 * fz.TOL * np.abs(a[col]).max(), (a[col], b[col])


# ---- refusals: ValueErrors before any device work, which the device file therefore never passes ---------------------------------------
def test_refusals(pkg):
    with pytest.raises(ValueError, match="attention dropout"):
        pkg.gat(None, [8, 8, 3], heads=[2, 1], variant="v2", attn_dropout=0.3)
    with pytest.raises(ValueError, match="heads lists 3 layers"):
        pkg.gat(None, [8, 8, 3], heads=[2, 1, 1])
    with pytest.raises(ValueError, match="not divisible"):
        pkg.gat(None, [8, 10, 3], heads=[4, 1])
    with pytest.raises(ValueError, match="not divisible"):
        pkg.gat(None, [8, 8, 3], heads=[2, 2], variant="v2")
    with pytest.raises(ValueError, match="hoist_first_aggregation"):
        pkg.gcn(None, [16, 8, 4], agg_dtype="bf16", hoist_first_aggregation=True)


def test_no_case_is_one_the_library_refuses(pkg):
    import sys
    G = sys.modules[pkg.gat.__module__]
    for c in _admitted("gat"):
        assert G.check_heads(c["sizes"], c["heads"]) == c["per_layer_heads"]
        G.check_variant(c["opt"]["variant"], c["opt"]["attn_dropout"])
    for c in _admitted("gcn"):
        assert not (c["opt"]["hoist_first_aggregation"] and c["opt"]["agg_dtype"] == "bf16")
        assert int((c["S"] == 0).sum()) >= 1 if c["S"] is not None else True
