"""Correct and Smooth (Huang et al. 2021, "Combining Label Propagation and Simple Models Out-performs Graph Neural
Networks"; PyG's ``CorrectAndSmooth``): post-processing of the logits of any trained model by two short label-propagation
loops over the graph.  Nothing is trained.  No reference counterpart.

With Â the caller's ``csr_matrix`` (values as given; ``datasets.sym_normalize`` gives D^-1/2 A D^-1/2), T the number of
training rows (``S == train_set``) and every product the sweep SpMM's (``ops.matmul`` with the plan cached on the matrix):

  1. P = softmax(logits) row-wise                                                               ops.cs_residual
  2. E0 = onehot(y) - P on the training rows, +0.0 elsewhere;  sigma = sum |E0| / T              (the same kernel)
  3. correct:  E <- E0, then L1 times  E <- post(a1 (Â E) + (1 - a1) E0)                          matmul + ops.cs_step
       autoscale:  post = clamp(-1, 1);   otherwise post writes E0's rows back over the training rows and does not clamp
  4. Z = P + s_i E:  s_i = sigma / sum_c |E[i, c]|, 1 where that is not finite or above 1000      ops.cs_correct
       (autoscale; a row with E = 0 is P's row), otherwise s_i = scale
  5. smooth:  G0 = Z with onehot(y) over the training rows;  G <- G0, then L2 times  G <- clamp(a2 (Â G) + (1 - a2) G0, 0, 1)
  6. the prediction is the row argmax of G, the first maximum winning (ops.max_row_indices)

The iteration counts are fixed: no convergence test and no synchronisation inside a loop -- everything is enqueued on the
compute stream and the caller synchronises once.  sigma stays on the device.  The factors reach the kernels as
fp32(alpha) and fp32(1 - alpha), the subtraction in double.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import ops
from .gcn import check_sets
from .matrix import context, csr_matrix, dn_matrix

INF = float("inf")


def _check_alpha(name: str, alpha) -> float:
    try:
        a = float(alpha)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number in (0, 1], got {alpha!r}")
    if not (0.0 < a <= 1.0):
        raise ValueError(f"{name} must lie in (0, 1], got {alpha!r}")
    return a


def _check_layers(name: str, layers) -> int:
    if isinstance(layers, bool) or not isinstance(layers, (int, np.integer)) or layers < 0:
        raise ValueError(f"{name} must be a non-negative integer, got {layers!r}")
    return int(layers)


class correct_and_smooth:
    """``cs = correct_and_smooth(A, n_classes, num_correction_layers, correction_alpha, num_smoothing_layers,
    smoothing_alpha, autoscale=True, scale=1.0)`` (PyG's argument names), then

        Z  = cs.correct(ctx, logits, Y, S, train_set=0)     step 4, [n x C]
        G  = cs.smooth(ctx, Z, Y, S, train_set=0)           step 5
        G  = cs(ctx, logits, Y, S, train_set=0)             both: the correct kernel writes G0 directly
        yp = cs.predict(ctx, model, X, Y, S, train_set=0)   host int32 [n x 1]: model(ctx, X) -> cs -> argmax, one sync

    ``logits``: an [n x C] fp32 dn_matrix, only read.  ``Y`` / ``S``: the class and the set of every vertex, numpy arrays of
    n integers or int32 dn_matrix of n rows, as set_splits takes them; only the labels of the training rows are looked at.
    They are checked on the host and uploaded when the (Y, S, train_set) OBJECTS differ from the previous call's: after
    editing an array in place pass a copy.  The results are the object's own buffers (five [n x C] matrices and one
    float, allocated on first use and kept): a later call overwrites them.  A layer count of zero is valid: L1 = 0 gives
    E = E0 and L2 = 0 gives G = G0.  Every check raises ValueError naming the argument before any device work.

    Timers: cs-residual, cs-correct (the first loop), cs-scale (step 4), cs-smooth (the second loop), and cs-spmm /
    cs-step: the product and the step of the last iteration that ran."""

    def __init__(self, A: csr_matrix, n_classes: int, num_correction_layers: int, correction_alpha: float,
                 num_smoothing_layers: int, smoothing_alpha: float, autoscale: bool = True, scale: float = 1.0):
        if not isinstance(A, csr_matrix):
            raise ValueError(f"A must be a csr_matrix, got {type(A).__name__}")
        if A.n() != A.m():
            raise ValueError(f"A must be square, got {A.n()} x {A.m()}")
        if isinstance(n_classes, bool) or not isinstance(n_classes, (int, np.integer)) or not 1 <= n_classes <= ops.CS_MAX_WIDTH:
            raise ValueError(f"n_classes must be an integer in [1, {ops.CS_MAX_WIDTH}], got {n_classes!r}")
        self.A, self.n_classes = A, int(n_classes)
        self.num_correction_layers = _check_layers("num_correction_layers", num_correction_layers)
        self.num_smoothing_layers = _check_layers("num_smoothing_layers", num_smoothing_layers)
        self.correction_alpha = _check_alpha("correction_alpha", correction_alpha)
        self.smoothing_alpha = _check_alpha("smoothing_alpha", smoothing_alpha)
        self.autoscale = bool(autoscale)
        try:
            self.scale = float(scale)
        except (TypeError, ValueError):
            raise ValueError(f"scale must be a finite number, got {scale!r}")
        if not np.isfinite(self.scale):
            raise ValueError(f"scale must be a finite number, got {scale!r}")
        self._rank = None           # the device the buffers live on
        self._labels = None         # (Y object, S object, train_set, Y on the device, S on the device, training rows)

    # -- checks (host only) ---------------------------------------------------------------------------------------------
    def _check_dense(self, name: str, M) -> None:
        n, C = self.A.n(), self.n_classes
        if not hasattr(M, "n") or (M.n(), M.m()) != (n, C):
            got = f"{M.n()} x {M.m()}" if hasattr(M, "n") else type(M).__name__
            raise ValueError(f"{name} must be a {n} x {C} dn_matrix, got {got}")

    def _check_labels(self, Y, S, train_set: int):
        """(labels, sets) as host int32 [n x 1] arrays and the number of training rows"""
        n = self.A.n()
        try:
            sets = check_sets(S, n, train_set)
        except ValueError as e:
            raise ValueError(f"S / train_set: {e}")
        if isinstance(Y, dn_matrix):
            if Y.t.dtype != __import__("torch").int32 or Y.shape() != (n, 1):
                raise ValueError(f"Y must be an int32 dn_matrix of {n} x 1, got {Y.t.dtype} of {Y.shape()}")
            labels = Y.numpy()
        else:
            labels = np.asarray(Y)
            if labels.dtype.kind not in "iu" or labels.size != n or labels.ndim > 2 or (labels.ndim == 2 and labels.shape[1] != 1):
                raise ValueError(f"Y must be {n} integers, got {labels.dtype} of shape {labels.shape}")
            labels = np.ascontiguousarray(labels.reshape(n, 1).astype(np.int64))
        train = sets.reshape(-1) == train_set
        count = int(train.sum())
        if count == 0:
            raise ValueError(f"S: no vertex belongs to set {train_set}: there is no training row to propagate from")
        y = labels.reshape(-1)[train]
        if y.min() < 0 or y.max() >= self.n_classes:
            bad = y[(y < 0) | (y >= self.n_classes)][0]
            raise ValueError(f"Y: the label {int(bad)} of a training row is outside [0, {self.n_classes})")
        return labels.astype(np.int32), sets, count

    # -- device state --------------------------------------------------------------------------------------------------------
    def _buffers(self, ctx: context) -> None:
        if self._rank == ctx.rank:
            return
        torch = __import__("torch")
        ctx.set()
        n, C = self.A.n(), self.n_classes
        self.P, self.E0, self.X1, self.X2, self.G0 = (dn_matrix(n, C, device=ctx.device) for _ in range(5))
        self.sums = torch.zeros(1, dtype=torch.float32, device=ctx.device)
        self.pred = None
        self._labels = None
        self._rank = ctx.rank

    def _device_labels(self, ctx: Optional[context], Y, S, train_set: int):
        """(Y, S) on the device and the number of training rows; checked and uploaded once per (Y, S, train_set)"""
        have = self._labels
        if have is not None and have[0] is Y and have[1] is S and have[2] == train_set:
            return have[3:]
        labels, sets, count = self._check_labels(Y, S, train_set)
        self._buffers(ctx)
        Yd = Y if isinstance(Y, dn_matrix) else dn_matrix.from_numpy(labels, device=ctx.device)
        Sd = S if isinstance(S, dn_matrix) else dn_matrix.from_numpy(sets, device=ctx.device)
        self._labels = (Y, S, train_set, Yd, Sd, count)
        return Yd, Sd, count

    def _propagate(self, ctx: context, R: dn_matrix, layers: int, alpha: float, lo: float, hi: float, Sd, train_set: int,
                   flags: int, timer: str) -> dn_matrix:
        """X <- R, then ``layers`` times X <- post(alpha (Â X) + (1 - alpha) R); the product goes to the buffer the state
        is not in (the SpMM's C must not be its B) and the step runs in place on it"""
        plan = ops.spmm_plan_for(ctx, self.A, self.n_classes, self.n_classes)
        beta = 1.0 - alpha
        X = R
        ctx.record("0_" + timer, 0)
        for i in range(layers):
            last = i == layers - 1
            T = (self.X1, self.X2)[i % 2]
            if last:
                ctx.record("0_cs-spmm", 0)
            ops.matmul(ctx, self.A, X, T, plan, 1.0, 0.0)
            if last:
                ctx.record("1_cs-spmm", 0)
            ops.cs_step(ctx, T, R, Sd, alpha, beta, lo, hi, train_set, flags)
            if last:
                ctx.record("1_cs-step", 0)
                ctx.register_timer("cs-spmm", "0_cs-spmm", "1_cs-spmm")
                ctx.register_timer("cs-step", "1_cs-spmm", "1_cs-step")
            X = T
        ctx.record("1_" + timer, 0)
        ctx.register_timer(timer, "0_" + timer, "1_" + timer)
        return X

    def _correct(self, ctx: context, logits: dn_matrix, Yd, Sd, count: int, train_set: int, set_labels: bool) -> dn_matrix:
        ctx.record("0_cs-residual", 0)
        ops.cs_residual(ctx, logits, Yd, Sd, train_set, self.P, self.E0, self.sums)
        ctx.record("1_cs-residual", 0)
        ctx.register_timer("cs-residual", "0_cs-residual", "1_cs-residual")
        if self.autoscale:
            E = self._propagate(ctx, self.E0, self.num_correction_layers, self.correction_alpha, -1.0, 1.0, None, train_set,
                                0, "cs-correct")
        else:
            E = self._propagate(ctx, self.E0, self.num_correction_layers, self.correction_alpha, -INF, INF, Sd, train_set,
                                ops.CS_FIX_TRAIN, "cs-correct")
        flags = (ops.CS_AUTOSCALE if self.autoscale else 0) | (ops.CS_SET_LABELS if set_labels else 0)
        ctx.record("0_cs-scale", 0)
        ops.cs_correct(ctx, self.P, E, Yd, Sd, train_set, self.sums, float(np.float32(1.0 / count)), self.scale, flags,
                       out=self.G0)
        ctx.record("1_cs-scale", 0)
        ctx.register_timer("cs-scale", "0_cs-scale", "1_cs-scale")
        return self.G0

    def _smooth(self, ctx: context) -> dn_matrix:
        return self._propagate(ctx, self.G0, self.num_smoothing_layers, self.smoothing_alpha, 0.0, 1.0, None, 0, 0,
                               "cs-smooth")

    # -- the public calls ----------------------------------------------------------------------------------------------------
    def correct(self, ctx: context, logits: dn_matrix, Y, S, train_set: int = 0) -> dn_matrix:
        """steps 1-4: Z = softmax(logits) + the propagated, scaled training residual"""
        self._check_dense("logits", logits)
        Yd, Sd, count = self._device_labels(ctx, Y, S, train_set)
        self._buffers(ctx)
        return self._correct(ctx, logits, Yd, Sd, count, train_set, set_labels=False)

    def smooth(self, ctx: context, Z: dn_matrix, Y, S, train_set: int = 0) -> dn_matrix:
        """step 5 on any [n x C] Z (correct()'s, or class probabilities from elsewhere; only read unless it is
        correct()'s own buffer)"""
        self._check_dense("Z", Z)
        Yd, Sd, _ = self._device_labels(ctx, Y, S, train_set)
        self._buffers(ctx)
        # G0 = Z with the labels written in: the correct kernel at scale 0 over a zeroed E (z + 0 * 0)
        self.X1.zero(ctx)
        ops.cs_correct(ctx, Z, self.X1, Yd, Sd, train_set, None, 0.0, 0.0, ops.CS_SET_LABELS, out=self.G0)
        return self._smooth(ctx)

    def __call__(self, ctx: context, logits: dn_matrix, Y, S, train_set: int = 0) -> dn_matrix:
        """steps 1-5; the same bits as smooth(correct(...))"""
        self._check_dense("logits", logits)
        Yd, Sd, count = self._device_labels(ctx, Y, S, train_set)
        self._buffers(ctx)
        self._correct(ctx, logits, Yd, Sd, count, train_set, set_labels=True)
        return self._smooth(ctx)

    def predict(self, ctx: context, model, X: dn_matrix, Y, S, train_set: int = 0) -> np.ndarray:
        """the classes after Correct and Smooth of ``model`` (a gcn or gat with the softmax loss and n_classes outputs;
        its plain forward: no dropout, no label input) as a host int32 [n x 1] array; one synchronisation"""
        if getattr(model, "loss", "softmax") == "bce":
            raise ValueError('model: correct_and_smooth needs one class per vertex, the model has loss="bce" (multi-label)')
        width = getattr(model, "_out_width", self.n_classes)
        if width != self.n_classes:
            raise ValueError(f"model: its logits have {width} columns, n_classes is {self.n_classes}")
        Yd, Sd, count = self._device_labels(ctx, Y, S, train_set)
        self._buffers(ctx)
        logits = model(ctx, X)
        self._check_dense("model(ctx, X)", logits)
        self._correct(ctx, logits, Yd, Sd, count, train_set, set_labels=True)
        G = self._smooth(ctx)
        if self.pred is None:
            self.pred = dn_matrix(self.A.n(), 1, dtype=np.int32, device=ctx.device)
        ops.max_row_indices(ctx, G, self.pred)
        ctx.sync()
        return self.pred.numpy()
