"""model.roc_auc and model_selector(metric="roc_auc") on tiny multi-label models: the integers of the device against the numpy
restatement (tests/auc_ref.py) on the model's own logits, a run that is bit for bit the run without the metric, and the
selector's history, best epoch and restore."""
import math

import numpy as np
import pytest

import auc_ref as ref

pytestmark = pytest.mark.gpu

N, SIZES = 300, [24, 16, 5]
ADAM = (1e-2, 0.9, 0.999, 5e-4, 1e-8)
KINDS = ("gcn", "gat", "sage")


@pytest.fixture()
def ctx(pkg):
    return pkg.context(0)           # a context per test: its timers are this test's


_data = {}


def _problem(pkg):
    if not _data:
        ip, ix, dv = pkg.datasets.synth_powerlaw_csr(N, 3000, 80, seed=5)
        rng = np.random.default_rng(8)
        centres = rng.standard_normal((SIZES[-1], SIZES[0]))
        Y = (rng.random((N, SIZES[-1])) < 0.3).astype(np.int32)
        X = (Y @ centres + 0.7 * rng.standard_normal((N, SIZES[0]))).astype(np.float32)
        S = rng.choice(np.array([0, 1, 2, 7], dtype=np.int32), size=(N, 1), p=[0.5, 0.2, 0.2, 0.1])
        _data.update(csr=(ip, ix, dv), X=X, Y=Y, S=S)
    return _data


def _make(pkg, kind, loss="bce"):
    d = _problem(pkg)
    ip, ix, dv = d["csr"]
    A = pkg.csr_matrix(ip.copy(), ix.copy(), dv.copy(), N)
    if kind == "gcn":
        model = pkg.gcn(A, SIZES, loss=loss)
    elif kind == "gat":
        model = pkg.gat(A, SIZES, heads=[2, 1], loss=loss, dropout=0.5, fanout=4)
    else:
        model = pkg.sage(A, SIZES, aggr="max", loss=loss)
    return model, pkg.dn_matrix.from_numpy(d["X"].copy()), pkg.dn_matrix.from_numpy(d["Y"].copy())


def _param_bits(pkg, model):
    return [getattr(owner, p).numpy().view(np.uint32).copy() for _, owner, p, _, _ in pkg.checkpoint.model_params(model)]


def _same(got, want, what):
    assert got["stats"] == want, what
    summary = ref.summary(want)
    np.testing.assert_array_equal(got["per_class"], summary["per_class"], err_msg=what)
    for name in ref.VIEWS:
        assert got[name] == summary[name] or (math.isnan(got[name]) and math.isnan(summary[name])), (what, name)


@pytest.mark.parametrize("kind", KINDS)
def test_roc_auc_equals_the_restatement_on_the_models_logits(pkg, ctx, kind):
    d = _problem(pkg)
    model, X, Y = _make(pkg, kind)
    S = pkg.dn_matrix.from_numpy(d["S"])
    model.train_step(ctx, X, Y, *ADAM)                              # away from the initial weights
    logits = model(ctx, X)
    ctx.sync()
    logits = logits.numpy().copy()
    _same(model.roc_auc(ctx, X, Y, S), ref.stats(logits, d["Y"], d["S"]), f"{kind}: S given")
    _same(model.roc_auc(ctx, X, Y, d["S"].reshape(-1)), ref.stats(logits, d["Y"], d["S"]), f"{kind}: S as host integers")
    _same(model.roc_auc(ctx, X, Y), ref.stats(logits, d["Y"], None), f"{kind}: no sets")
    model.set_splits(d["S"])
    _same(model.roc_auc(ctx, X, Y), ref.stats(logits, d["Y"], d["S"]), f"{kind}: the sets of set_splits")
    assert model._roc_auc_evaluator is not None and model._roc_auc_evaluator.group == SIZES[-1]
    for name in ("roc-auc-keys", "roc-auc-sort", "roc-auc-stats"):
        assert name in ctx.timers


@pytest.mark.parametrize("kind", KINDS)
def test_a_roc_auc_call_changes_no_bit_of_the_run(pkg, ctx, kind):
    d = _problem(pkg)
    runs = []
    for with_metric in (False, True):
        model, X, Y = _make(pkg, kind)
        model.set_splits(d["S"])
        losses = [model.train_step(ctx, X, Y, *ADAM)]
        if with_metric:
            before = (model.dropout_epoch, getattr(model, "sample_epoch", 0))
            model.roc_auc(ctx, X, Y)
            assert (model.dropout_epoch, getattr(model, "sample_epoch", 0)) == before
        losses.append(model.train_step(ctx, X, Y, *ADAM))
        runs.append((losses, _param_bits(pkg, model), model.dropout_epoch, getattr(model, "sample_epoch", 0)))
    assert runs[0][0] == runs[1][0] and runs[0][2:] == runs[1][2:]
    assert len(runs[0][1]) == len(runs[1][1]) > 0
    for a, b in zip(runs[0][1], runs[1][1]):
        np.testing.assert_array_equal(a, b)


def test_a_run_without_the_metric_has_no_timer_and_no_evaluator(pkg, ctx):
    model, X, Y = _make(pkg, "gcn")
    model.train_step(ctx, X, Y, *ADAM)
    assert model._roc_auc_evaluator is None
    assert not [name for name in ctx.timers if name.startswith("roc-auc")]


@pytest.mark.parametrize("kind", ["gcn", "gat"])
def test_selector_on_roc_auc(pkg, ctx, kind):
    d = _problem(pkg)
    model, X, Y = _make(pkg, kind)
    model.set_splits(d["S"])
    sel = pkg.model_selector(model, split="val", metric="roc_auc")
    assert sel.clean
    want, params = [], []
    for _ in range(8):
        sel.step(ctx, X, Y, *ADAM)
        logits = model(ctx, X)
        ctx.sync()
        want.append(ref.summary(ref.stats(logits.numpy(), d["Y"], d["S"]))["val"])
        params.append(_param_bits(pkg, model))
    assert sel.history == want
    assert len(set(want)) > 1 and not any(math.isnan(v) for v in want)
    assert sel.best_epoch == int(np.argmax(want)) and sel.best_value == max(want)
    sel.restore(ctx)
    for a, b in zip(_param_bits(pkg, model), params[sel.best_epoch]):
        np.testing.assert_array_equal(a, b)


def test_refusals(pkg, ctx):
    d = _problem(pkg)
    soft, X, _ = _make(pkg, "gcn", loss="softmax")
    soft.set_splits(d["S"])
    labels = pkg.dn_matrix.from_numpy(np.zeros((N, 1), dtype=np.int32))
    with pytest.raises(ValueError, match="loss"):
        soft.roc_auc(ctx, X, labels)
    with pytest.raises(ValueError, match="loss"):
        pkg.model_selector(soft, metric="roc_auc")
    model, X, Y = _make(pkg, "gcn")
    model.set_splits(d["S"])
    with pytest.raises(ValueError, match="clean"):
        pkg.model_selector(model, metric="roc_auc", clean=False)
    with pytest.raises(ValueError, match="metric"):
        pkg.model_selector(model, metric="auc")
    with pytest.raises(ValueError, match="targets"):
        model.roc_auc(ctx, X, labels)                               # n x 1 labels are not n x C targets
    with pytest.raises(ValueError, match="^S: "):
        model.roc_auc(ctx, X, Y, np.zeros(N - 1, dtype=np.int32))
    assert model._roc_auc_evaluator is None and not [name for name in ctx.timers if name.startswith("roc-auc")]
