"""Randomised parity of every model option and of the attention models (-m gpu): the cases of fuzz_ref.py that
test_fuzz_options_cpu.py admits, two epochs each against the composed reference from identical state every epoch (the
reference takes over the device's parameters and Adam moments), the second epoch through train_step where the case says so --
its gradients are then compared after the Adam step, as test_gpu_bce.py does.  test_gpu_fuzz_model.py draws a graph, a plain
layer stack and ``fused``; this draws everything merged since: residual_layer, hoist_first_aggregation, agg_dtype, dropout,
norm, loss, splits and train_step on gcn, and variant, per-layer head lists, both dropouts, loss, splits and train_step on gat,
on graphs with empty rows of F, vertices nobody gathers, eight vertices, one giant row and rows that hold only their self-loop.

The bars are the project's own, through fuzz_ref.distances() -- the measure admission used on the CPU: loss 1e-4 relative;
accuracy within 3 / rows; with bce every confusion count within 3 and micro-F1 equal to micro_f1 of the device's own counts;
with splits the same per split through split_metrics(), the row counts exact; every gradient (G_W, G_b, the residual branch's,
G_gamma, G_beta, G_att) within 1e-4 of max(|want|.max(), 1e-2 x the model's largest gradient), test_gpu_fuzz_model.py's rule;
bf16 cases at GRAD_BAR / GRAD_BAR_REST / W_SOLID_BAR of test_gpu_agg_bf16.py on the same denominator; the parameters of gat
(and of bf16 gcn) after Adam never more than a sign flip (2.05 lr) away and at 1e-4 in the well-conditioned entries,
test_gat_epochs_match_the_reference's rule; every device number finite.

On every fourth seed, without a reference: evaluate() with dropout switched on equals a plain forward, which equals the forward
with dropout off bit for bit, and leaves dropout_epoch alone; and for gat the same case with ``fused`` flipped gives the same
bits in every parameter, gradient and moment.  gcn makes no such promise at the model's level -- fused=True swaps in the one-pass
loss and the column sums of G_b, which round differently from the chains they replace, and everything downstream inherits that --
so there the same case with ``fused`` flipped is held to the reference once more, at the same bars.

For gat the reference also runs at its other precision from the state each epoch starts from, and where the two cannot tell the
sign of an activation (fuzz_ref.undetermined_signs: within 8 x their difference of zero, admission's margin) its leaky_relu' takes
the device's sign, which a gat layer keeps in ``out``.  That state is the device's own Adam step, which admission cannot visit; the
rule is admission's, decided by the reference alone, and the count of such signs is printed (gcn overwrites its sign source in the
backward pass and rests on admission only).

No case is skipped: the parametrisation is fuzz_ref.admitted(), and no invalid shape or option reaches the library.

Measured on an MI355X, the worst value over the admitted seeds and both epochs / its bar (accuracy and confusion in rows):
  gcn (36 seeds, 9 of them once more with ``fused`` flipped)   loss 1.4e-6 / 1e-4; accuracy 0 rows / 3; confusion 0 / 3; split row
                   counts exact; fp32 cases: G_W 7.1e-6, G_b 1.0e-5, the residual branch's 3.3e-6 and 2.6e-6, G_gamma 3.6e-6,
                   G_beta 3.1e-6 / 1e-4; bf16 cases: first layer's G_W 1.7e-7 / 1e-2, every other G_W 3.9e-5, G_b 2.98e-4 (seed 4 with
                   ``fused`` flipped; 3.7e-7 as drawn, 4.4e-5 the next worst), the residual branch's 1.2e-4 and 9.9e-5, G_gamma 1.5e-5,
                   G_beta 8.1e-5 / 3e-4; W and b a sign flip at most (worst 2.3e-3 of 2.05 lr), their well-conditioned entries
                   2.7e-6 / 1e-4 (first layer 8.4e-8 / 1e-2)
  gat (37 seeds)   loss 2.6e-7 / 1e-4; accuracy 0 rows / 3; confusion 0 / 3; split row counts exact; G_W 7.7e-6, G_b 7.3e-6,
                   G_att 3.0e-5 / 1e-4; W and att a sign flip at most (0.07 and 0.44 of 2.05 lr), their well-conditioned entries
                   1.1e-5 and 1.2e-5 / 1e-4; signs the reference took from the device: one, in seed 35 (layer 1's out[148, 18]:
                   +2.0e-8 in the twin, -2.4e-8 in the restatement, -1.2e-7 on the device)
  seconds per case (two epochs)   gcn: device median 0.004, worst 0.034; reference median 0.003, worst 0.10; gat: device median
                   0.002, worst 0.005; reference (both precisions) median 0.012, worst 0.43 (a 512-column v1 layer on 40 vertices);
                   the whole file, model construction included: 5.4 s for 74 tests.
One deliberate break, never committed (_arm_dropout handing layer l the dropout stream of layer l + 1, results only): 39 of the 73
cases turn red -- every gcn and gat case that drops anything, and no other.
"""
import time

import numpy as np
import pytest

import bce_ref
import fuzz_ref as fz

pytestmark = pytest.mark.gpu

GCN_SEEDS, GAT_SEEDS = fz.admitted("gcn"), fz.admitted("gat")


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


def test_the_parametrisation_is_the_admitted_set():
    for family, seeds in (("gcn", GCN_SEEDS), ("gat", GAT_SEEDS)):
        assert len(seeds) == fz.SEEDS - len(fz.EXCLUDED[family]) >= fz.SEEDS - fz.MAX_EXCLUDED
        assert not set(seeds) & set(fz.EXCLUDED[family])


def _model(pkg, case, fused=None):
    o = case["opt"]
    A = pkg.csr_matrix(case["ip"].copy(), case["ix"].copy(), case["dv"].copy(), case["n"])
    kw = fz.gcn_kwargs(case) if case["family"] == "gcn" else fz.gat_kwargs(case)
    if fused is not None:
        kw["fused"] = fused
    G = (pkg.gcn if case["family"] == "gcn" else pkg.gat)(A, case["sizes"], **kw)
    if o["dropout"] or o.get("attn_dropout"):
        G.set_dropout(o["dropout"], seed=o["dropout_seed"])
    if case["S"] is not None:
        G.set_splits(case["S"])
    return G


def _init_from(G, initial):
    for layer, init in zip(G.layers(), initial):
        if init["norm"] is not None:
            layer.norm.init(*init["norm"])
        if init["att"] is not None:
            layer.attn.init(init["att"])


def _finite(what, tree):
    for li, row in enumerate(tree):
        for name, v in row.items():
            assert np.isfinite(v).all(), (what, li, name)


def _device_epoch(G, ctx, case, Xd, Yd, epoch):
    """one epoch on the device in fuzz_ref.distances()'s ``got`` form"""
    o = case["opt"]
    if o["step"] and epoch == 1:
        loss, score = G.train_step(ctx, Xd, Yd, *fz.ADAM)
        grads = fz.device_grads(G)
    else:
        loss, score = G.train_forward(ctx, Xd, Yd)
        G.backward(ctx)
        ctx.sync()
        grads = fz.device_grads(G)
        G.adam_update(ctx, *fz.ADAM)
        ctx.sync()
    got = dict(loss=loss, score=score, grads=grads, params=fz.device_params(G))
    assert np.isfinite(loss), (fz.describe(case), epoch, loss)
    _finite("gradient", grads)
    _finite("parameter", got["params"])
    if o["loss"] == "bce":
        got["conf"] = G.loss_layer.confusion()
        assert np.isfinite(got["conf"]).all()
        own = bce_ref.micro_f1(*got["conf"])
        assert score == own or (np.isnan(score) and np.isnan(own)), (epoch, score, got["conf"])
    else:
        assert np.isfinite(score)
    if case["S"] is not None:
        m = G.split_metrics()
        assert m["train"] == (loss, score) or np.isnan(score), (epoch, m["train"], loss, score)
        got["per"] = {name: (m[name][0], m[name][1], m.get("confusion", {}).get(name), m["counts"][name]) for name in fz.SPLIT_NAMES}
        for name in fz.SPLIT_NAMES:
            assert np.isfinite(m[name][0]) == (m["counts"][name] > 0), (epoch, name, m[name], m["counts"])
    return got


def _run(pkg, ctx, oracle, case, monkeypatch, folded):
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    what = fz.describe(case)
    R = fz.reference(case, oracle)
    gat = case["family"] == "gat"
    other = fz.reference(case, oracle, other=True) if gat else None
    G = _model(pkg, case)
    _init_from(G, R.initial())
    Xd, Yd = pkg.dn_matrix.from_numpy(case["X"]), pkg.dn_matrix.from_numpy(case["Y"])
    t_dev = t_ref = 0.0
    bad = []
    taken = 0
    for epoch in range(2):
        state = fz.device_state(G)
        R.set_state(state)
        t0 = time.perf_counter()
        got = _device_epoch(G, ctx, case, Xd, Yd, epoch)
        t1 = time.perf_counter()
        if gat:
            # a gat layer keeps its sign source (``out``) through the backward pass: where the reference's two precisions cannot
            # tell an activation's sign at THIS state, leaky_relu' of the reference takes the device's (fuzz_ref.undetermined_signs)
            other.set_state(state)
            with fz.recorded_signs(oracle) as rec:
                other.epoch()
            outs = [l.out.numpy().copy() for l in reversed(G.layers()) if l.activation]
            with fz.undetermined_signs(oracle, rec, outs) as u:
                want = R.epoch()
            taken += u.taken
        else:
            want = R.epoch()
        t2 = time.perf_counter()
        t_dev, t_ref = t_dev + t1 - t0, t_ref + t2 - t1
        lines = fz.distances(case, epoch, got, want)
        for key, (q, value, bar) in fz.worst(lines).items():
            if key not in folded or q > folded[key][0]:
                folded[key] = (q, value, bar)
        bad += [(epoch, name, value, bar) for name, value, bar, _ in lines if not value <= bar]
    for key, (q, value, bar) in sorted(folded.items()):
        print(f"[fuzz] {case['family']} seed {case['seed']} {key}: {value:.3e} (bar {bar:g})")
    print(f"[fuzz] {case['family']} seed {case['seed']} seconds: device {t_dev:.3f} reference {t_ref:.3f}; signs taken from the device: {taken}")
    assert not bad, (what, bad)
    return G, Xd, Yd


def _state_bits(G):
    out = []
    for tree in (fz.device_state(G), fz.device_grads(G)):
        for row in tree:
            for key in sorted(row):
                v = row[key]
                for name in (sorted(v) if isinstance(v, dict) else [None]):
                    a = v[name] if name is not None else v
                    out.append((key, name, np.asarray(a).view(np.uint32).copy() if isinstance(a, np.ndarray) else a))
    return out


def _free_run(pkg, ctx, case, initial, fused):
    G = _model(pkg, case, fused=fused)
    _init_from(G, initial)
    Xd, Yd = pkg.dn_matrix.from_numpy(case["X"]), pkg.dn_matrix.from_numpy(case["Y"])
    res = [_device_epoch(G, ctx, case, Xd, Yd, epoch) for epoch in range(2)]
    return [(r["loss"], r["score"]) for r in res], _state_bits(G)


def _evaluate_never_drops(pkg, ctx, case, G, Xd, Yd):
    """dropout switched on at the epoch the model has reached: evaluate() is a plain forward, a plain forward is the forward
    with dropout off, bit for bit, and neither moves dropout_epoch"""
    e, seed = G.dropout_epoch, case["opt"]["dropout_seed"]
    v1 = case["family"] == "gat" and case["opt"]["variant"] == "v1"
    G.set_dropout(0.5, seed=seed, epoch=e, **(dict(attn=0.3) if v1 else {}))
    Z = G(ctx, Xd)
    ctx.sync()
    Z = Z.numpy().copy()
    Sd = None if case["S"] is None else pkg.dn_matrix.from_numpy(case["S"].reshape(-1, 1))
    ev = G.evaluate(ctx, Xd, Yd, Sd)
    assert G.dropout_epoch == e
    rows = [("all", np.ones(case["n"], dtype=bool))] + ([] if Sd is None else [(nm, case["S"] == k) for k, nm in enumerate(("train", "val", "test"))])
    for name, r in rows:
        if case["opt"]["loss"] == "bce":
            want = bce_ref.micro_f1(*bce_ref.counts(Z[r], case["Y"][r])[0])
        else:
            want = float((Z[r].argmax(axis=1) == case["Y"].reshape(-1)[r]).mean()) if r.any() else float("nan")
        assert ev[name] == want or (np.isnan(ev[name]) and np.isnan(want)), (name, ev[name], want)
    G.set_dropout(0.0, seed=seed, epoch=e, **(dict(attn=0.0) if v1 else {}))
    Z0 = G(ctx, Xd)
    ctx.sync()
    assert np.array_equal(Z0.numpy().view(np.uint32), Z.view(np.uint32)), "a plain forward with dropout on is not the forward with dropout off"
    assert G.dropout_epoch == e


@pytest.mark.parametrize("seed", GCN_SEEDS)
def test_gcn_options_match_the_reference(pkg, oracle, ctx, monkeypatch, seed):
    case = fz.gcn_case(seed)
    G, Xd, Yd = _run(pkg, ctx, oracle, case, monkeypatch, {})
    assert G.layers()[0].hoist_input == fz.hoist_effective(case)
    assert [l.gemm_first() for l in G.layers()] == fz.gemm_first(case)
    if seed % 4 == 0:
        _evaluate_never_drops(pkg, ctx, case, G, Xd, Yd)
        flipped = dict(case, opt=dict(case["opt"], fused=not case["opt"]["fused"]))
        _run(pkg, ctx, oracle, flipped, monkeypatch, {})


@pytest.mark.parametrize("seed", GAT_SEEDS)
def test_gat_options_match_the_reference(pkg, oracle, ctx, monkeypatch, seed):
    case = fz.gat_case(seed)
    G, Xd, Yd = _run(pkg, ctx, oracle, case, monkeypatch, {})
    assert G.heads == case["per_layer_heads"]
    if seed % 4 == 0:
        _evaluate_never_drops(pkg, ctx, case, G, Xd, Yd)
        initial = fz.reference(case, oracle).initial()
        a, b = (_free_run(pkg, ctx, case, initial, fused) for fused in (False, True))
        assert a[0] == b[0] or all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a[0], b[0])), (a[0], b[0])
        assert len(a[1]) == len(b[1])
        for (ka, na, va), (kb, nb, vb) in zip(a[1], b[1]):
            assert (ka, na) == (kb, nb) and np.array_equal(va, vb), ("fused flipped", ka, na)
