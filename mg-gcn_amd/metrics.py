"""Ranking metrics on the device (opt-in; the reference has none): ROC-AUC of a multi-label model, per class and split, as
exact integers.  The logits never leave the device: ops.roc_auc_keys makes sortable keys class by class, ops.radix_sort_pairs
sorts every class, ops.roc_auc_stats counts.  A program that never calls any of this allocates, launches and registers nothing.
"""
from __future__ import annotations

import math
import numbers
from typing import Optional

import numpy as np

from . import ops
from .matrix import context, dn_matrix

VIEWS = ops.ROC_AUC_VIEWS           # ("train", "val", "test", "other", "all"): the rows of "per_class", the k of "stats"


def _torch():
    import torch
    return torch


def auc_of(two_u: int, pos: int, neg: int) -> float:
    """2U / (2 P N): numerator and denominator as Python integers, one division in float64; nan where P N == 0"""
    den = 2 * int(pos) * int(neg)
    return int(two_u) / den if den else float("nan")


def summarize(stats) -> dict:
    """what roc_auc_evaluator returns, from stats[c][k] = (2U, P, N) as Python integers: the mean per view over the classes
    whose AUC is defined there (an exactly rounded sum over their count; nan if none), "per_class" and "stats" """
    per_class = np.array([[auc_of(*stats[c][k]) for c in range(len(stats))] for k in range(len(VIEWS))],
                         dtype=np.float64).reshape(len(VIEWS), len(stats))
    out = {}
    for k, name in enumerate(VIEWS):
        known = [v for v in per_class[k].tolist() if not math.isnan(v)]
        out[name] = math.fsum(known) / len(known) if known else float("nan")
    out["per_class"] = per_class
    out["stats"] = stats
    return out


def check_rows(n, what: str = "n") -> int:
    if not isinstance(n, numbers.Integral) or isinstance(n, bool) or n < 0:
        raise ValueError(f"{what} must be a non-negative integer, not {n!r}")
    if n >= 1 << 31:
        raise ValueError(f"{what} must be below 2^31 (a class is one sort segment), got {n}")
    return int(n)


class roc_auc_evaluator:
    """roc_auc_evaluator(n, n_classes, max_workspace_bytes=256 << 20): ROC-AUC of n rows x n_classes logits against int32
    targets, per class and per split.

    ev(ctx, logits, Y, S=None) enqueues everything on the compute stream and synchronises once.  logits (fp32) and Y (int32,
    non-zero = positive) are dn_matrix objects or 2-D device tensors with unit column stride (a column window of a wider
    matrix), n x n_classes both; S is the int32 n x 1 dn_matrix of sets or None (every row is in slot "train").  Returns
        {"train" | "val" | "test" | "other" | "all": the mean AUC over the classes whose AUC is defined in that view (nan if
         none; a class without a positive or without a negative there is skipped, as OGB's evaluator skips it),
         "per_class": float64 [5 x n_classes], rows in that order, nan where P N == 0,
         "stats": [n_classes][5][3] Python integers (2U, P, N)}
    with AUC = 2U / (2 P N) -- ties count one half -- formed from Python integers and divided once in float64.  "all" is
    every row, whatever its slot.  A NaN logit is ranked where the key map of ops.roc_auc_keys puts its bit pattern.

    The classes are processed in groups of g = clamp(floor(max_workspace_bytes / (16 n)), 1, n_classes) columns: the four
    sort arrays (keys, values and their scratch twins, 16 n g bytes, allocated with the first call and kept) never exceed the
    cap -- except with g = 1, where one class is the least a sort can take and 16 n bytes may be more than the cap.  The
    histogram and count tables come on top (about 1/8 of that).  The integers do not depend on g.

    Timers roc-auc-keys, roc-auc-sort and roc-auc-stats (of the last group) exist once it has been called."""

    def __init__(self, n: int, n_classes: int, max_workspace_bytes: int = 256 << 20):
        self.n = check_rows(n)
        if not isinstance(n_classes, numbers.Integral) or isinstance(n_classes, bool) or n_classes < 1:
            raise ValueError(f"n_classes must be a positive integer, not {n_classes!r}")
        if (not isinstance(max_workspace_bytes, numbers.Integral) or isinstance(max_workspace_bytes, bool)
                or max_workspace_bytes < 1):
            raise ValueError(f"max_workspace_bytes must be a positive integer, not {max_workspace_bytes!r}")
        self.n_classes = int(n_classes)
        g = self.n_classes if self.n == 0 else int(max_workspace_bytes) // (16 * self.n)
        if self.n:
            g = min(g, ((1 << 31) - 1) // self.n)                   # one sort call stays below 2^31 pairs
        self.group = max(1, min(g, self.n_classes))
        self._arrays = None

    def workspace_bytes(self) -> int:
        """the device bytes the evaluator holds after its first call"""
        return (16 * self.n * self.group + ops.radix_sort_work_bytes(self.group, self.n)
                + ops.roc_auc_stats_work_bytes(self.n, self.group) + 120 * self.n_classes)

    def _allocate(self, ctx: context):
        torch = _torch()
        pairs = max(self.n * self.group, 1)
        four = [torch.empty(pairs, dtype=torch.int32, device=ctx.device) for _ in range(4)]
        work = torch.empty(max(ops.radix_sort_work_bytes(self.group, self.n),
                               ops.roc_auc_stats_work_bytes(self.n, self.group), 8) // 8 + 1, dtype=torch.int64,
                           device=ctx.device)                       # the sort is done with it before the statistic starts
        stats = torch.empty(self.n_classes * len(VIEWS) * 3, dtype=torch.int64, device=ctx.device)
        self._arrays = (four, work, stats)

    def _check(self, logits, Y, S) -> None:
        shape = (self.n, self.n_classes)
        for name, M in (("logits", logits), ("Y", Y)):
            t = M.t if isinstance(M, dn_matrix) else M
            if not hasattr(t, "shape") or tuple(t.shape) != shape:
                got = tuple(t.shape) if hasattr(t, "shape") else type(M).__name__
                raise ValueError(f"{name} must be {shape[0]} x {shape[1]}, got {got}")
        if S is not None and (not isinstance(S, dn_matrix) or S.t.dtype != _torch().int32 or S.shape() != (self.n, 1)):
            got = f"{S.t.dtype} of {S.shape()}" if isinstance(S, dn_matrix) else type(S).__name__
            raise ValueError(f"S must be an int32 dn_matrix of {self.n} x 1 or None, got {got}")

    def __call__(self, ctx: context, logits, Y, S: Optional[dn_matrix] = None) -> dict:
        self._check(logits, Y, S)
        if self._arrays is None:
            self._allocate(ctx)
        (keys, vals, keys_alt, vals_alt), work, stats = self._arrays
        n = self.n
        for c0 in range(0, self.n_classes, self.group):
            nc = min(self.group, self.n_classes - c0)
            ops.roc_auc_keys(ctx, logits, Y, S, c0, nc, keys, vals, timer="roc-auc-keys")
            ops.radix_sort_pairs(ctx, nc, n, keys, vals, keys_alt, vals_alt, work, timer="roc-auc-sort")
            ops.roc_auc_stats(ctx, keys, vals, n, nc, stats[c0 * 15:], work, timer="roc-auc-stats")
        ctx.sync()
        host = stats.cpu().numpy().reshape(self.n_classes, len(VIEWS), 3)
        return summarize([[tuple(int(x) for x in host[c, k]) for k in range(len(VIEWS))] for c in range(self.n_classes)])


def model_roc_auc_checks(model, Y, S, targets: bool = True):
    """the refusals of model.roc_auc / model_selector(metric="roc_auc") (which has no targets yet: ``targets`` False), before
    any device work; returns the sets to use"""
    from .gcn import check_sets, check_targets
    if getattr(model, "loss", None) != "bce":
        raise ValueError(f"roc_auc needs a model with loss='bce' (one binary task per logit), this one has "
                         f"loss={getattr(model, 'loss', None)!r}")
    n = check_rows(model.A.n(), "n (the number of vertices)")
    if targets:
        check_targets(model.loss, Y, n, model._out_width)
    if S is None:
        loss_layer = getattr(model.loss_layer, "inner", model.loss_layer)
        return loss_layer.S
    try:
        host = check_sets(S, n, 0)
    except ValueError as e:
        raise ValueError(f"S: {e}") from None
    return S if isinstance(S, dn_matrix) else dn_matrix.from_numpy(host)
