"""Model selection on a split's loss or score: keep the best epoch's parameters, stop early, restore, save (opt-in; the
reference reports over all vertices and keeps nothing).  Host bookkeeping around train_step for gcn, dist.dist_gcn, gat.gat
and dist_gat.dist_gat; the only device work it adds is dn_matrix.copy_to of the parameters (and, with ``clean``, one plain
forward and one loss-layer call per epoch).  A model without a selector launches and allocates nothing new.
"""
from __future__ import annotations

import math
from typing import List, Optional

from . import ops
from .checkpoint import model_params, raw_context, reset_adam

METRICS = ("loss", "score")                 # the pair split_metrics() reports per split
RANKING_METRICS = ("roc_auc",)              # computed by a pass of their own (model.roc_auc); always a clean pass


class model_selector:
    """model_selector(model, split="val", metric="loss" | "score" | "roc_auc", patience=None, clean=None)

    step(ctx, X, Y, lr, beta1, beta2, weight_decay, eps) runs one train_step and returns what it returns.

    clean=False monitors the training forward's own split metric, which is free.  That number describes the parameters
    BEFORE the epoch's update and is read after it, so every step first copies the parameters into a candidate buffer
    (stream-ordered copy_to, parameters only) and promotes the candidate when the number read afterwards improved:
    ``history[e]`` and ``best_epoch = e`` speak of the parameters epoch e started from.

    clean=True runs one extra plain forward and one loss-layer call after the update (no backward) and monitors that:
    ``history[e]`` speaks of the parameters epoch e ended with, snapshotted when the number improved.  The extra forward
    is not a training forward: it draws no mask and spends no dropout epoch.  split_metrics() of the model then reports
    the clean pass.  The default is clean = (dropout_p > 0 or attn_dropout_p > 0 or edge sampling on): with a dropout on, the
    training forward's validation numbers are the dropped forward's, with edge sampling (set_sampling) they are the sampled
    graph's, and a model must not be selected on either: the clean pass runs on the full graph.

    metric="roc_auc" (models with loss="bce": gcn, gat, sage) monitors model.roc_auc(ctx, X, Y)[split], the mean ROC-AUC
    over the classes that have both labels in the split, on the device.  It is always a clean pass -- one extra plain
    forward after the update, then keys, sort and count; no loss-layer call, so split_metrics() keeps the training forward's
    numbers --, hence clean=False together with it is refused.

    "Improved" is strict -- lower loss, higher score or roc_auc; the first best epoch wins a tie; a NaN never improves.
    ``stop`` turns true once ``patience`` epochs have passed without improvement."""

    def __init__(self, model, split: str = "val", metric: str = "loss", patience: Optional[int] = None,
                 clean: Optional[bool] = None):
        if metric not in METRICS + RANKING_METRICS:
            raise ValueError(f"metric must be one of {METRICS + RANKING_METRICS}, not {metric!r}")
        if split not in ops.SPLIT_NAMES[:3]:
            raise ValueError(f"split must be one of {ops.SPLIT_NAMES[:3]}, not {split!r}")
        if patience is not None and (int(patience) != patience or patience < 1):
            raise ValueError(f"patience must be a positive integer or None, not {patience!r}")
        loss_layer = getattr(model.loss_layer, "inner", model.loss_layer)
        if loss_layer.S is None:
            raise ValueError("model_selector needs set_splits(...) on the model first")
        if not loss_layer.counts[ops.SPLIT_NAMES.index(split)]:
            raise ValueError(f"no vertex belongs to the {split} split: nothing to select on")
        if metric in RANKING_METRICS:
            if clean is not None and not clean:
                raise ValueError(f"clean=False does not go with metric={metric!r}: the ranking metric is a pass of its own "
                                 "after the update (a clean pass), the training forward does not produce it")
            if not callable(getattr(model, "roc_auc", None)):
                raise ValueError(f"metric={metric!r} needs a model with roc_auc (gcn, gat, sage), not {type(model).__name__}")
            from .metrics import model_roc_auc_checks
            model_roc_auc_checks(model, None, None, targets=False)               # loss="bce", n < 2^31: before any device work
            clean = True
        self.model, self.split, self.metric = model, split, metric
        self.patience = None if patience is None else int(patience)
        dropping = (model.dropout_p > 0.0 or getattr(model, "attn_dropout_p", 0.0) > 0.0
                    or getattr(model, "sampler", None) is not None)         # edge sampling: validate on the full graph
        self.clean = bool(dropping) if clean is None else bool(clean)
        self.history: List[float] = []
        self.best_epoch: Optional[int] = None
        self.best_value: Optional[float] = None
        self.stop = False
        self._best = self._candidate = None                     # name -> dn_matrix, allocated with the first step

    def _params(self):
        return [(name, getattr(owner, p)) for name, owner, p, _, _ in model_params(self.model)]

    def _snapshot(self, ctx, into) -> dict:
        rc = raw_context(ctx)
        if into is None:
            into = {name: t.copy(rc) for name, t in self._params()}
        else:
            for name, t in self._params():
                t.copy_to(rc, into[name])
        return into

    def _improved(self, value: float) -> bool:
        if math.isnan(value):
            return False
        if self.best_value is None:
            return True
        return value < self.best_value if self.metric == "loss" else value > self.best_value

    def step(self, ctx, X, Y, lr, beta1, beta2, weight_decay, eps):
        if not self.clean:
            self._candidate = self._snapshot(ctx, self._candidate)          # the parameters this epoch's metric describes
        result = self.model.train_step(ctx, X, Y, lr, beta1, beta2, weight_decay, eps)
        if self.metric in RANKING_METRICS:
            value = float(self.model.roc_auc(ctx, X, Y)[self.split])        # plain forward, keys, sort, count; synchronises
        else:
            if self.clean:
                self.model.loss_layer(ctx, self.model(ctx, X), Y)           # plain forward, no mask; synchronises
            value = float(self.model.split_metrics()[self.split][METRICS.index(self.metric)])
        epoch = len(self.history)
        self.history.append(value)
        if self._improved(value):
            self.best_epoch, self.best_value = epoch, value
            if self.clean:
                self._best = self._snapshot(ctx, self._best)
            else:
                self._best, self._candidate = self._candidate, self._best
        last = -1 if self.best_epoch is None else self.best_epoch
        self.stop = self.patience is not None and epoch - last >= self.patience
        return result

    def _need_best(self) -> dict:
        if self._best is None:
            raise ValueError("no epoch has improved yet: there is no best model")
        return self._best

    def restore(self, ctx) -> None:
        """puts the best parameters back into the model (in place) and resets Adam: zero moments, step 0"""
        best, rc = self._need_best(), raw_context(ctx)
        for name, t in self._params():
            best[name].copy_to(rc, t)
        reset_adam(self.model, ctx)
        ctx.sync()

    def save_best(self, ctx, path: str) -> None:
        """writes the best parameters as a checkpoint without the optimiser section (dist_gcn: every rank calls)"""
        best = self._need_best()
        ctx.sync()
        self.model._write_checkpoint(ctx, path, {name: t.numpy() for name, t in best.items()}, False, 0)
