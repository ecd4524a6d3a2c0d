"""GraphSAGE on one GPU (opt-in; the reference has no such model): ``sage(A, sizes, aggr="mean" | "max")``.

A layer computes ``Y = agg(H) W_l + 1 b_l^T + H W_r + 1 b_r^T`` and then the activation: the ROOT branch ``H W_r`` joins
BEFORE the activation, which is what tells the model from ``gcn(residual_layer=True)`` (that one adds ``H W_res`` after it).
``layer.lin`` is (W_l, b_l), ``layer.res_lin`` (W_r, b_r); both have a bias, as the skip of the attention models has.  The
order is always aggregate, then the two GEMMs, the second with ``discard=False`` on top of the first.

``aggr="mean"`` aggregates with gcn's operator: ``sparse_linear`` on ``A.normalize(True)`` -- the sweep SpMM forward over
``A.transpose()`` and backward over A.  ``aggr="max"`` takes the element-wise maximum over a vertex's neighbours
(``max_aggregate``: ops.agg_max_forward / ops.agg_max_backward, csrc/agg_max.hip) over the PATTERN of ``A.transpose()``; the
values of A are not read and not changed.  The forward remembers which neighbour it selected per element (``arg``), and the
backward routes a gradient element to exactly that source over the row-sorted pattern of A, without atomics.

Layer 0's aggregate is loop-invariant (the features are never dropped): ``agg(X)`` is computed on the first forward and kept,
keyed on (buffer, shape, matrix version) as gcn's hoisted product is; ``reset_input_cache()`` drops it (the way to pick up an
in-place change of X).  Layer 0 stores no ``arg`` and computes no input gradient.  A layer l >= 1 keeps ``M = agg(H)``
[n x in] -- and for max ``arg`` [n x in] -- from forward to backward.

``norm="layer"`` normalises every layer but the last between the GEMMs and the activation (gcn.layer_norm; the activation
rides in its kernel); ``dropout=p`` / set_dropout drop the input of every layer but the first in place with the counter-based
mask, so both branches see the dropped H, and the gradient returned; ``loss="bce"`` composes; ``fused`` picks how Adam is
launched (one launch for the model or one per tensor: the same bits).  set_splits, split_metrics, train_step, evaluate,
predict, model_selector's in-memory restore and smoothing.correct_and_smooth.predict are model_base's.

``fanout=k`` / ``edge_keep=q`` with ``aggr="max"`` (None and 1.0 by default: nothing new is allocated, launched or registered)
train every epoch on a fresh sample of the edges drawn on the device (edge_sample.py; set_sampling(fanout, keep, seed, epoch),
``sample_fanout`` / ``sample_keep`` / ``sample_seed`` / ``sample_epoch``, as on gat): a training forward aggregates, forward and
backward, over the pair of the epoch; every other forward runs on the full graph.  A sampled training forward neither reads
nor writes layer 0's kept ``agg(X)``: it aggregates X over the sample into a buffer of its own every epoch (``_M_sampled``),
and stores no ``arg`` there either -- layer 0 has no input gradient and its weight gradient reads M alone.  The sample keeps
the entry order of the row-sorted pattern and duplicates share their bit, so equal indices of a sampled row stay adjacent,
which the max backward needs.  ``aggr="mean"`` is a weighted sum and samples only when told how the kept values are rescaled:
``edge_rescale="row"`` (the mean over the sampled neighbours -- the published GraphSAGE recipe) or ``"inverse"``
(set_sampling(..., rescale=)); with ``edge_rescale`` None (the default) any setting that is on is refused by the argument's
name.  Its training forward multiplies by the pair of the epoch through the row-split SpMM on a plan built on the device
(sparse_linear.sample, ops.spmm_dev), layer 0 again into ``_M_sampled``.  ``aggr="max"`` reads no values and refuses
``edge_rescale``.

Refused with ValueError naming the argument, before any device work: an unknown ``aggr``, a matrix that is not square, and
gcn's own errors for ``norm``, ``loss`` and ``dropout``; save / load / model_selector.save_best (no version of the checkpoint
file stores a sage: nothing is read, written or created).  The row partition is dist_sage.dist_sage (a sage_layer per rank
over dist_row_linear, with dist_max_aggregate or dist_sparse_linear).  Not built: sum / min / the pooling MLP, the GEMM-first
order for mean when out < in, bf16 gathers (on one GPU, on the wire and in the packed max-backward record), the halo and
rounds schedules for max, hiding the forward gather under the root GEMM, one all-reduce for both linears of a layer,
checkpoints for any sage, the C++ layer and CLI, and a planned (non-row-walk) form for rows of many thousand entries.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np

from . import ops
from .edge_sample import refuse_sampling, rescaled_sampling_option
from .gcn import (check_loss, check_norm, layer_norm, layer_params, linear, model_base, sigmoid_bce_loss,
                  softmax_cross_entropy_loss, sparse_linear)
from .matrix import context, csr_matrix, dn_matrix

AGGREGATORS = ("mean", "max")


def check_aggr(aggr: str) -> str:
    """option checking of aggr=, before any device work"""
    if aggr not in AGGREGATORS:
        raise ValueError(f"aggr must be one of {AGGREGATORS}, not {aggr!r}")
    return aggr


def refuse_checkpoint(member: str) -> None:
    raise ValueError(f"sage: {member} has no version that stores a sage model yet")


class max_aggregate:
    """The max aggregator with sparse_linear's call shape: agg(ctx, B, M) is M[i, c] = max over the entries j of row i of F of
    B[j, c], agg.backward(ctx, G_M, G_B, discard) routes G_M[i, c] to the source the forward selected, over the rows of
    ``F_T`` -- whose equal indices must be adjacent (ops.agg_max_backward); csr_matrix.transpose() returns such rows.
    ``keep_arg=False`` (a layer without an input gradient) stores no selection and has no backward.  ``arg`` [rows x width],
    uint32 bits in an int32 dn_matrix, is made with the first call; ``launches`` counts the forward calls."""

    sample = None               # (F, F_T) of this forward where the model drew an edge sample (edge_sample.py); None: the full graph

    def __init__(self, name: str, F: csr_matrix, F_T: Optional[csr_matrix], keep_arg: bool = True):
        self.name, self.F, self.F_T, self.keep_arg = name, F, F_T, bool(keep_arg)
        self.arg: Optional[dn_matrix] = None
        self.launches = 0

    def _matrices(self):
        """(F, F_T) the most recent forward walked and its backward walks.  A sample keeps the entry order of the matrix it was
        drawn from and duplicates share their bit, so equal indices of a sampled row of F_T stay adjacent."""
        return self.sample if self.sample is not None else (self.F, self.F_T)

    def __call__(self, ctx: context, B: dn_matrix, M: dn_matrix, discard: bool = True, flags: int = 0) -> None:
        if not discard or flags:
            raise ValueError("max_aggregate: the forward overwrites its output and has no epilogue")
        if self.keep_arg and (self.arg is None or self.arg.shape() != M.shape()):
            self.arg = dn_matrix(M.n(), M.m(), dtype=np.int32, device=ctx.device)
        ops.agg_max_forward(ctx, self._matrices()[0], B, M, self.arg if self.keep_arg else None, timer=self.name + "0_agg-max")
        self.launches += 1

    def backward(self, ctx: context, G_M: dn_matrix, G_B: dn_matrix, discard: bool = True) -> None:
        if self.arg is None:
            raise ValueError("max_aggregate: no forward has stored a selection (keep_arg=False, or none has run)")
        ops.agg_max_backward(ctx, self._matrices()[1], self.arg, G_M, G_B, accumulate=not discard, timer=self.name + "1_agg-max")


class counted_sparse_linear(sparse_linear):
    """gcn's mean aggregator, counting its forward calls as max_aggregate does"""

    launches = 0

    def __call__(self, ctx: context, B: dn_matrix, C: dn_matrix, discard: bool = True, flags: int = 0) -> None:
        sparse_linear.__call__(self, ctx, B, C, discard, flags)
        self.launches += 1


class sage_layer(layer_params):
    """One GraphSAGE layer over a square matrix: Y = agg(H) W_l + 1 b_l^T + H W_r + 1 b_r^T, then the layer norm (with the
    activation in its kernel) or the leaky ReLU, in place in ``Y``.  ``agg``: the aggregation operator, agg(ctx, B, M) and
    agg.backward(ctx, G_M, G_H, discard) -- sparse_linear or max_aggregate.  ``first``: layer 0, whose aggregate is kept
    across forwards (``reset_input_cache``) and which has no input gradient.  ``G_M`` aliases the model-wide buffer."""

    def __init__(self, name: str, agg, rows: int, in_: int, out: int, activation: bool, first: bool, G_M_buffer=None,
                 norm=None, lin=None, res_lin=None, norm_layer=None):
        """``lin`` / ``res_lin`` / ``norm_layer``: the layer's two linears and its norm where the caller builds them (the row
        partition: dist_sage.dist_sage_layer); None builds the single-GPU ones"""
        check_norm(norm)
        self.name, self.agg, self.first, self.activation = name, agg, bool(first), bool(activation)
        # the linears' own fused kernels in every mode, as in the attention models: sage(fused=...) only picks how Adam is
        # launched
        self.lin = linear(name, in_, out, not first, True) if lin is None else lin
        self.res_lin = linear(name + "root_", in_, out, not first, True) if res_lin is None else res_lin
        if norm_layer is not None:
            self.norm = norm_layer
        else:
            self.norm = layer_norm(name, rows, out, True, adam_fused=True) if norm == "layer" and activation else None
        self.Y = dn_matrix(rows, out)
        self.M: Optional[dn_matrix] = None if first else dn_matrix(rows, in_)
        self._M_key = None
        self._M_sampled: Optional[dn_matrix] = None     # layer 0's aggregate over an edge sample: never the kept agg(X)
        self._M_used: Optional[dn_matrix] = None        # what the most recent forward handed to lin, for its backward
        self.G_M = None if first else dn_matrix(rows, in_, G_M_buffer)
        self.G_out = None if first else dn_matrix(rows, in_)
        self.H: Optional[dn_matrix] = None
        self.dropout = None             # (threshold, scale, seed, stream) of ops.dropout_raw, set by the model per forward
        self.row0 = 0

    def _drop(self, ctx: context, M: dn_matrix, tag: str) -> None:
        """M = dropout(M) in place with this forward's mask: H on the way up ("0"), G_out on the way down ("1")"""
        n = self.name
        threshold, scale, seed, stream = self.dropout
        ctx.record(n + tag + "_0_dropout", 0)
        ops.dropout_raw(ctx, M, M, threshold, scale, seed, stream, self.row0)
        ctx.record(n + tag + "_1_dropout", 0)
        ctx.register_timer(n + tag + "_dropout", n + tag + "_0_dropout", n + tag + "_1_dropout")

    def reset_input_cache(self) -> None:
        if self.first:
            self.M = self._M_key = None

    def _matrix_version(self) -> int:
        return getattr(getattr(self.agg, "F", None) or self.agg.A, "_version", 0)

    def __call__(self, ctx: context, H: dn_matrix) -> dn_matrix:
        n = self.name
        if self.dropout is not None:
            # In place in the Y buffer of the layer below, as in gcn: its backward reads that buffer for the SIGN of its
            # activation only, which a positive scale keeps, and a dropped element carries a zero gradient either way.
            self._drop(ctx, H, "0")
        self.H = H
        if self.first and getattr(self.agg, "sample", None) is not None:
            # a sampled training forward: the aggregate is this epoch's, in a buffer of its own -- the kept agg(X) of the full
            # graph is neither read nor written.  No arg: layer 0 has no input gradient, its backward reads M alone.
            if self._M_sampled is None or self._M_sampled.shape() != (self.Y.n(), H.m()):
                self._M_sampled = dn_matrix(self.Y.n(), H.m())
            self.agg(ctx, H, self._M_sampled)
            self._M_used = self._M_sampled
        elif self.first:
            # loop-invariant: the features are never dropped.  An IN-PLACE change of X is not visible in the key:
            # reset_input_cache() drops the product.
            key = (H.buffer(), H.n(), H.m(), self._matrix_version())
            if self.M is None or self._M_key != key:
                self.M = dn_matrix(self.Y.n(), H.m())
                self.agg(ctx, H, self.M)
                self._M_key = key
            self._M_used = self.M
        else:
            self.agg(ctx, H, self.M)
            self._M_used = self.M
        self.lin(ctx, self._M_used, self.Y)
        self.res_lin(ctx, H, self.Y, False)
        if self.norm is not None:
            self.norm(ctx, self.Y, True)
        elif self.activation:
            ctx.record(n + "0_0_activation", 0)
            ops.leaky_relu_forward(ctx, self.Y, self.Y)
            ctx.record(n + "0_1_activation", 0)
            ctx.register_timer(n + "0_activation", n + "0_0_activation", n + "0_1_activation")
        return self.Y

    def backward(self, ctx: context, G: dn_matrix) -> Optional[dn_matrix]:
        n = self.name
        T = G
        if self.norm is not None:
            self.norm.backward(ctx, G, self.Y, self.Y)      # leaky_relu'(Y as the forward left it), then the norm's backward
            T = self.Y
        elif self.activation:
            ctx.record(n + "1_0_activation", 0)
            ops.leaky_relu_backward(ctx, self.Y, G, self.Y)
            ctx.record(n + "1_1_activation", 0)
            ctx.register_timer(n + "1_activation", n + "1_0_activation", n + "1_1_activation")
            T = self.Y
        self.lin.setX(self._M_used)
        self.lin.backward(ctx, T, self.G_M)
        if not self.first and hasattr(self.agg, "start_backward"):
            # an aggregator that exchanges G_M (dist_sage.dist_max_aggregate): the collective runs under the GEMMs below
            self.agg.start_backward(ctx, self.G_M)
        self.res_lin.setX(self.H)
        self.res_lin.backward(ctx, T, self.G_out)
        if self.first:
            return None
        self.agg.backward(ctx, self.G_M, self.G_out, False)
        if self.dropout is not None:
            self._drop(ctx, self.G_out, "1")
        return self.G_out

    def linears(self):
        return [self.lin, self.res_lin]

    def owners(self):
        return [(prefix, o) for prefix, o in (("", self.lin), ("res_", self.res_lin), ("", self.norm)) if o is not None]

    def W_root(self): return self.res_lin.get_W()
    def b_root(self): return self.res_lin.get_b()


class sage(rescaled_sampling_option, model_base):
    """sage(A, sizes, aggr="mean", loss="softmax", fused=True, weights=None, dropout=0.0, norm=None, fanout=None, edge_keep=1.0,
    edge_rescale=None): see the module's text.
    ``A`` is taken as gcn takes it (the forward aggregates over the rows of A.transpose()); ``weights``: (W_l, b_l, W_r, b_r)
    per layer."""

    def __init__(self, A: csr_matrix, sizes: Sequence[int], aggr: str = "mean", loss: str = "softmax", fused: bool = True,
                 weights=None, dropout: float = 0.0, norm=None, fanout=None, edge_keep: float = 1.0, edge_rescale=None):
        self.aggr = check_aggr(aggr)                         # option checks come before any device work
        self._init_sampling(fanout, edge_keep, edge_rescale)  # aggr="mean": on only with a rescale; aggr="max": no rescale
        if A.n() != A.m():
            raise ValueError(f"A must be square, got {A.n()} x {A.m()}")
        self._init_dropout(dropout, len(sizes) - 1)
        self.norm = check_norm(norm)
        self.loss = check_loss(loss)
        self.sizes = [int(s) for s in sizes]
        self._out_width = self.sizes[-1]
        self.fused = bool(fused)
        import torch
        loss_class = sigmoid_bce_loss if self.loss == "bce" else softmax_cross_entropy_loss
        self.loss_layer = loss_class(f"{len(sizes) - 1}_", True, True)
        n, n_layers = A.n(), len(self.sizes) - 1
        self._plan_wants = []
        if self.aggr == "mean":
            A.normalize(True)
            A_T = A.transpose()
            self.A, self.A_T = A, A_T
            for l in range(n_layers):
                w = self.sizes[l]
                self._plan_wants.append((A_T, max(w, 128), w))
                if l:
                    self._plan_wants.append((A, max(w, 128), w))
        else:
            # F = A.transpose(), and F.transpose(): the row-sorted pattern of A, whose equal indices are adjacent (the
            # generators emit unsorted rows with duplicates); built once on the host, A itself stays as it is
            self.A, self.A_T = A, A.transpose()
            self._A_sorted = self.A_T.transpose()
        widest = max(self.sizes[1:-1], default=1)
        self.G_M_buffer = torch.empty(n * widest, dtype=torch.float32, device="cuda") if n_layers > 1 else None
        self.layers_: List[sage_layer] = []
        for l in range(n_layers):
            name = f"{l}_"
            if self.aggr == "mean":
                agg = counted_sparse_linear(name, self.A_T, self.A)
            else:
                agg = max_aggregate(name, self.A_T, self._A_sorted if l else None, keep_arg=l > 0)
            self.layers_.append(sage_layer(name, agg, n, self.sizes[l], self.sizes[l + 1], l + 1 < n_layers, l == 0,
                                           self.G_M_buffer, self.norm))
        self._adam = None
        self._sample_max_d = max(self.sizes[:-1])
        if self.aggr == "max":
            self._make_sampler(self.A_T, self._A_sorted)         # nothing unless sampling is on
        else:
            self._make_sampler(self.A_T, self.A)                 # with values: the forward matrix and the matrix it came from
        if weights is not None:
            if len(weights) != n_layers or any(len(w) != 4 for w in weights):
                raise ValueError(f"weights must be (W_l, b_l, W_r, b_r) for each of the {n_layers} layers")
            for layer, (W_l, b_l, W_r, b_r) in zip(self.layers_, weights):
                layer.lin.W.init(np.asarray(W_l, dtype=np.float32))
                layer.lin.b.init(np.asarray(b_l, dtype=np.float32))
                layer.res_lin.W.init(np.asarray(W_r, dtype=np.float32))
                layer.res_lin.b.init(np.asarray(b_r, dtype=np.float32))

    def __call__(self, ctx: context, H: dn_matrix, training: bool = False) -> dn_matrix:
        if self._plan_wants:                          # first call: the context (device) is known now
            ops.prebuild_plans(ctx, self._plan_wants)
            self._plan_wants = []
        pair = self._draw_sample(ctx, training)              # one sample per epoch, shared by all layers; None: the full graph
        for layer in self.layers_:
            layer.agg.sample = pair
        return model_base.__call__(self, ctx, H, training)

    def _refuse_sampling(self, fanout, keep) -> None:
        if self.aggr != "max" and self._rescale_checked() is None:
            refuse_sampling(f'sage(aggr="{self.aggr}")', fanout, keep)

    def _refuse_rescale(self, rescale) -> None:
        if self.aggr == "max":
            raise ValueError(f'sage(aggr="max") reads no values: edge_rescale (rescale) must be None, got {rescale!r}')

    def reset_input_cache(self) -> None:
        """drops layer 0's kept aggregate agg(X): the next forward computes it again"""
        self.layers_[0].reset_input_cache()

    def save(self, ctx, path: str, optimizer: bool = True) -> None:
        refuse_checkpoint("save: the checkpoint file")

    def load(self, ctx, path: str) -> None:
        refuse_checkpoint("load: the checkpoint file")

    def _write_checkpoint(self, ctx, path: str, tensors, optimizer: bool, step: int) -> None:
        refuse_checkpoint("the checkpoint file (model_selector.save_best included)")
