"""ROC-AUC on the device (metrics.roc_auc_evaluator over ops.roc_auc_keys / radix_sort_pairs / roc_auc_stats) against the
numpy restatement tests/auc_ref.py: every (2U, P, N) integer for integer, per class and view."""
import math

import numpy as np
import pytest

import auc_ref as ref

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (257, 3), (5_000, 41), (3_001, 112), (70_001, 2))
LOGITS = ("normal", "quantised", "equal-class", "inf")
TARGETS = ("bernoulli", "single-label")
PAD_FRONT, PAD_BACK = 3, 2          # the operands are column windows [3, 3 + C) of matrices C + 5 wide


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


def _torch():
    import torch
    return torch


def _logits(kind, n, C, rng):
    x = rng.standard_normal((n, C)).astype(np.float32)
    if kind == "quantised":                                         # four values, both zeros among them: heavy ties everywhere
        x = rng.choice(np.array([-1.0, -0.0, 0.0, 0.5], dtype=np.float32), size=(n, C))
    elif kind == "equal-class":
        x[:, C // 2] = np.float32(0.25)
    elif kind == "inf":
        x[rng.random((n, C)) < 0.05] = np.inf
        x[rng.random((n, C)) < 0.05] = -np.inf
    return np.ascontiguousarray(x)


def _targets(kind, n, C, rng):
    y = (rng.random((n, C)) < 0.3).astype(np.int32) * rng.integers(1, 9, size=(n, C)).astype(np.int32)    # non-zero = positive
    if kind == "single-label":
        y[:, 0] = 1                                                 # one class all positive
        y[:, C - 1] = 0 if C > 1 else 1                             # one class all negative
    return np.ascontiguousarray(y)


def _window(a):
    """`a` as the column window of a wider device matrix whose other columns hold values that would change the answer"""
    torch = _torch()
    wide = np.full((a.shape[0], a.shape[1] + PAD_FRONT + PAD_BACK), 7, dtype=a.dtype)
    wide[:, PAD_FRONT:PAD_FRONT + a.shape[1]] = a
    return torch.from_numpy(wide).cuda()[:, PAD_FRONT:PAD_FRONT + a.shape[1]]


def _check(got, x, y, s, what):
    want = ref.stats(x, y, s)
    assert got["stats"] == want, what
    summary = ref.summary(want)
    np.testing.assert_array_equal(got["per_class"], summary["per_class"], err_msg=what)
    for name in ref.VIEWS:
        assert got[name] == summary[name] or (math.isnan(got[name]) and math.isnan(summary[name])), (what, name)
    return want


@pytest.mark.parametrize("with_sets", [True, False], ids=["sets", "no-sets"])
@pytest.mark.parametrize("kind", LOGITS)
@pytest.mark.parametrize("n,C", SHAPES)
def test_stats_equal_the_restatement(pkg, ctx, n, C, kind, with_sets):
    rng = np.random.default_rng(n + 31 * C + len(kind))
    ev = pkg.roc_auc_evaluator(n, C)
    x = _logits(kind, n, C, rng)
    s = rng.choice(np.array([0, 1, 2, 7], dtype=np.int32), size=(n, 1)) if with_sets else None
    S = pkg.dn_matrix.from_numpy(s) if with_sets else None
    for targets in TARGETS:
        y = _targets(targets, n, C, rng)
        what = f"{n} x {C}, {kind} logits, {targets} targets, sets {with_sets}"
        want = _check(ev(ctx, _window(x), _window(y), S), x, y, s, what)
        if targets == "single-label":                               # both single-label classes: P N == 0, nan, skipped by the mean
            for c in {0, C - 1}:
                assert all(p * q == 0 for _, p, q in want[c])
    for name in ("roc-auc-keys", "roc-auc-sort", "roc-auc-stats"):
        assert name in ctx.timers


def test_single_label_classes_are_nan_and_the_mean_skips_them(pkg, ctx):
    rng = np.random.default_rng(2)
    n, C = 5_000, 41
    x, y = _logits("normal", n, C, rng), _targets("single-label", n, C, rng)
    got = pkg.roc_auc_evaluator(n, C)(ctx, pkg.dn_matrix.from_numpy(x), pkg.dn_matrix.from_numpy(y))
    assert np.isnan(got["per_class"][:, [0, C - 1]]).all()
    assert not np.isnan(got["per_class"][[0, 4], 1:C - 1]).any()    # without sets: slot "train" and "all" hold every row
    assert np.isnan(got["per_class"][1:4]).all() and math.isnan(got["val"])
    assert got["all"] == got["train"] == math.fsum(got["per_class"][4, 1:C - 1].tolist()) / (C - 2)
    _check(got, x, y, None, "dn_matrix operands")


@pytest.mark.parametrize("n,C", [(1, 1), (257, 3), (5_000, 41)])
def test_the_result_does_not_depend_on_the_group_size(pkg, ctx, n, C):
    rng = np.random.default_rng(5 + n)
    x, y = _logits("quantised", n, C, rng), _targets("bernoulli", n, C, rng)
    x[:, 0] = rng.standard_normal(n).astype(np.float32)
    s = rng.choice(np.array([0, 1, 2, 7], dtype=np.int32), size=(n, 1))
    X, Y, S = pkg.dn_matrix.from_numpy(x), pkg.dn_matrix.from_numpy(y), pkg.dn_matrix.from_numpy(s)
    results = []
    for cap, g in ((1, 1), (32 * n, min(2, C)), (16 * n * C, C)):   # below one class (the cap is exceeded), two classes, all
        ev = pkg.roc_auc_evaluator(n, C, max_workspace_bytes=cap)
        assert ev.group == g
        results.append(ev(ctx, X, Y, S))
    want = ref.stats(x, y, s)
    for r in results:
        assert r["stats"] == want


def test_two_calls_give_the_same_result(pkg, ctx):
    rng = np.random.default_rng(9)
    n, C = 3_001, 112
    x, y = _logits("quantised", n, C, rng), _targets("bernoulli", n, C, rng)
    s = rng.choice(np.array([0, 1, 2, 7], dtype=np.int32), size=(n, 1))
    X, Y, S = pkg.dn_matrix.from_numpy(x), pkg.dn_matrix.from_numpy(y), pkg.dn_matrix.from_numpy(s)
    ev = pkg.roc_auc_evaluator(n, C)
    first, second = ev(ctx, X, Y, S), ev(ctx, X, Y, S)
    assert first["stats"] == second["stats"] == ref.stats(x, y, s)
    np.testing.assert_array_equal(first["per_class"], second["per_class"])
    other = _logits("normal", n, C, rng)                            # and the kept buffers carry nothing over
    assert ev(ctx, pkg.dn_matrix.from_numpy(other), Y, S)["stats"] == ref.stats(other, y, s)


def test_keys_and_values_equal_the_restatement(pkg, ctx):
    """ops.roc_auc_keys on a column window, class-major, with sentinels around the outputs"""
    torch = _torch()
    rng = np.random.default_rng(4)
    n, C, c0, nc = 1_000, 70, 3, 66                                 # two column tiles, the second partial
    x = rng.choice(np.array([-np.inf, -1.5, -0.0, 0.0, 1e-30, 2.0, np.inf], dtype=np.float32), size=(n, C))
    y = _targets("bernoulli", n, C, rng)
    s = rng.choice(np.array([0, 1, 2, 7, -1], dtype=np.int32), size=(n, 1))
    pad = 128
    outs = [torch.full((n * nc + 2 * pad,), 0x5EA1DEAD, dtype=torch.int32, device="cuda") for _ in range(2)]
    for sets in (s, None):
        for o in outs:
            o.fill_(0x5EA1DEAD)
        pkg.ops.roc_auc_keys(ctx, _window(x), _window(y), None if sets is None else pkg.dn_matrix.from_numpy(sets), c0, nc,
                             outs[0][pad:pad + n * nc], outs[1][pad:pad + n * nc])
        ctx.sync()
        for o, want in zip(outs, (ref.keys_of(x[:, c0:c0 + nc]), ref.vals_of(y[:, c0:c0 + nc], sets))):
            w = o.cpu().numpy().view(np.uint32)
            np.testing.assert_array_equal(w[pad:pad + n * nc].reshape(nc, n), want.T)
            assert (w[:pad] == 0x5EA1DEAD).all() and (w[pad + n * nc:] == 0x5EA1DEAD).all()
