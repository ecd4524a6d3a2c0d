"""GraphSAGE on the 1D row partition: one process per GPU, the layer of sage.py on this rank's rows (opt-in; the reference
has no such model).  DESIGN.md 3.13.1 has the algebra, the bytes and the measurements.

Rank r owns rows [p_r, p_{r+1}) of every activation; W_l, b_l, W_r, b_r (and gamma, beta) are replicated.  A layer is
sage.sage_layer with two dist_row_linear -- each sums its gradients over the ranks with an all-reduce of its own, as
dist_gcn's residual linear does --, gcn.layer_norm with its two gradient rows in ``lin.extra`` (summed by lin's all-reduce),
and one of two aggregators:

  aggr="mean"   dist_sparse_linear behind dist._rank_aggregation: the buffers and the three schedules of dist_gcn_layer.
  aggr="max"    dist_max_aggregate.  Both kernels walk a whole row in one piece, so a rank runs them over ITS row block of
                each matrix with global column indices (dist_row_csr_matrix.row_block_global):
      forward   ONE all-gather of B_loc [n/P x in] into H_all (n/P . in . 4 bytes from this rank); ops.agg_max_forward
                over the row block of A_T with src0 = 0, so ``arg`` holds GLOBAL vertex numbers, exactly what the
                single-GPU call writes.  H_all is read by that one kernel only: the layers share one buffer.
      backward  the rank packs (arg, G_M) of its destinations into rows of 8-byte records (ops.agg_max_pack) and ONE
                all-gather of n/P . in . 8 bytes delivers the records of all destinations; ops.agg_max_backward_rec over the
                rank's row block of the row-sorted pattern of A (rows: local sources, columns: global destinations) with
                src0 = p_r.  The pack and the exchange start right after lin.backward (sage_layer.backward calls
                start_backward), so the root linear's GEMMs run under the collective.
  Every row of either pattern is walked by one rank, whole, in the order the single-GPU kernel walks it: M, arg and the
  aggregator's input gradient are the single-GPU rows bit for bit at any P (given the same B and G_M).  A single rank that
  exchanges nothing (no dist_context.self_gather) gathers nothing, packs nothing and calls the plain kernels: on one GPU the
  record form did not beat the plain call by more than its run-to-run spread.

The order of work in a layer is sage_layer's, so at P = 1 the model is sage bit for bit.  The forward gather is NOT hidden
under the root GEMM: H W_r would have to come before agg(H) W_l, which changes the bits of Y.

dist_sage is dist.dist_model_base (set_splits, split_metrics, train_step, set_dropout: a rank drops its rows of the global
mask, row0 = p_r).  Refused with ValueError naming the argument, before any device work or collective, on every rank alike:
an unknown ``aggr`` or ``mode``, aggr="max" with a mode other than "allgather", a pair that is not square or not of equal
size, n % P != 0, sage's own errors for ``norm``, ``loss`` and ``dropout``, and save / load / save_best.

Not built: bf16 on the wire or in the record, the halo and rounds schedules for max, hiding the forward gather under the
root GEMM, one all-reduce for both linears of a layer, checkpoints, sum / min / pooling aggregators, the C++ host layer and
CLI, a planned form for very long rows."""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np

from . import ops
from .dist import (_rank_aggregation, _torch, _wrap_local, dist_context, dist_model_base, dist_row_csr_matrix,
                   dist_row_dn_matrix, dist_row_linear, dist_row_softmax_cross_entropy_loss, dist_sparse_linear,
                   partition_bounds)
from .dist_gat import dist_attention
from .gcn import check_loss, check_norm, layer_norm
from .matrix import context, csr_matrix, dn_matrix
from .sage import check_aggr, refuse_checkpoint, sage_layer

__all__ = ["dist_max_aggregate", "dist_sage", "dist_sage_layer", "sorted_row_block"]
MODES = ("allgather", "halo", "rounds")


def sorted_row_block(F: csr_matrix) -> csr_matrix:
    """The pattern of ``F`` with every row's indices in ascending order, so that equal indices are adjacent (what
    ops.agg_max_backward and its record form ask of the matrix they walk); duplicates are kept, the values are dropped (ones).
    Host only."""
    indptr = np.asarray(F.indptr).astype(np.int64)
    indices = np.asarray(F.indices)
    rows = np.repeat(np.arange(indptr.size - 1), np.diff(indptr))
    order = np.lexsort((indices, rows))
    return csr_matrix(np.asarray(F.indptr, dtype=np.uint32).copy(), np.ascontiguousarray(indices[order], dtype=np.uint32),
                      np.ones(indices.size, dtype=np.float32), F.m())


class dist_max_aggregate:
    """sage.max_aggregate on one rank's rows, with its call shape: agg(ctx, B, M) and agg.backward(ctx, G_M, G_B, discard)
    on the rank's shards.  ``F``: the rank's row block of the forward matrix ([n/P x n], global columns); ``F_T``: the
    rank's row block of the ROW-SORTED pattern of the backward matrix (sorted_row_block; None with keep_arg=False).

    ``H_all_buffer`` (n x the widest input, floats), ``rec_buffer`` (n/P x width x 2) and ``rec_all_buffer`` (n x width x 2
    4-byte words, 8-byte aligned) may be shared by the layers of a model: a gather into them is ordered on the comm stream
    after everything the compute stream has queued, the previous reader included.  Without ``H_all_buffer``, or for an
    operand wider than it (layer 0's features), the gathered copy is allocated for the call and released after it.
    start_backward(ctx, G_M) packs and starts the record exchange; backward() starts it itself where nobody has."""

    def __init__(self, dctx: dist_context, name: str, F: csr_matrix, F_T: Optional[csr_matrix], keep_arg: bool = True,
                 H_all_buffer=None, rec_buffer=None, rec_all_buffer=None):
        p = partition_bounds(F.m(), dctx.P)
        self.name, self.F, self.F_T, self.keep_arg = name, F, F_T, bool(keep_arg)
        self.n, self.rows, self.row0 = F.m(), p[dctx.rank + 1] - p[dctx.rank], p[dctx.rank]
        assert F.n() == self.rows and (F_T is None or F_T.shape() == F.shape()), "the rank's row blocks of a square matrix"
        self._dctx = dctx
        self.exchanging = dctx.P > 1 or dctx.self_gather
        self.H_all_buffer, self.rec_buffer, self.rec_all_buffer = H_all_buffer, rec_buffer, rec_all_buffer
        self.arg: Optional[dn_matrix] = None
        self._rec_ready = None

    _exchange = dist_attention._exchange            # reads _dctx and name

    def __call__(self, ctx: context, B: dn_matrix, M: dn_matrix, discard: bool = True, flags: int = 0) -> None:
        if not discard or flags:
            raise ValueError("dist_max_aggregate: the forward overwrites its output and has no epilogue")
        if self.keep_arg and (self.arg is None or self.arg.shape() != M.shape()):
            self.arg = dn_matrix(M.n(), M.m(), dtype=np.int32, device=ctx.device)
        H_all, own = B, False
        if self.exchanging:
            d, buf = B.m(), self.H_all_buffer
            own = buf is None or buf.numel() < self.n * d
            H_all = dn_matrix(self.n, d, device=ctx.device) if own else dn_matrix(self.n, d, buf)
            ctx.wait(self._exchange(B.t, H_all.t, "0_sage-exchange"), 0)
        ops.agg_max_forward(ctx, self.F, H_all, M, self.arg if self.keep_arg else None, 0, timer=self.name + "0_agg-max")
        if own:
            ctx.sync()                              # the one-time copy is released: its reader has run

    def _records(self, d: int):
        """(rec_loc [rows x 2 d], rec_all [n x 2 d]) over the front of the buffers, made where there are none"""
        torch = _torch()
        dev = self._dctx.ctx.device
        if self.rec_buffer is None or self.rec_buffer.numel() < self.rows * 2 * d:
            self.rec_buffer = torch.empty(self.rows * 2 * d, dtype=torch.int32, device=dev)
        if self.rec_all_buffer is None or self.rec_all_buffer.numel() < self.n * 2 * d:
            self.rec_all_buffer = torch.empty(self.n * 2 * d, dtype=torch.int32, device=dev)
        return self.rec_buffer[:self.rows * 2 * d].view(self.rows, 2 * d), self.rec_all_buffer[:self.n * 2 * d].view(self.n, 2 * d)

    def start_backward(self, ctx: context, G_M: dn_matrix) -> None:
        """packs (arg, G_M) of the rank's destinations and starts the all-gather of the records on the comm stream"""
        if self.arg is None:
            raise ValueError("dist_max_aggregate: no forward has stored a selection (keep_arg=False, or none has run)")
        if not self.exchanging:
            return
        rec, rec_all = self._records(G_M.m())
        ops.agg_max_pack(ctx, self.arg, G_M, rec, timer=self.name + "1_agg-max-pack")
        self._rec_ready = (self._exchange(rec, rec_all, "1_sage-exchange-rec"), rec_all)

    def backward(self, ctx: context, G_M: dn_matrix, G_B: dn_matrix, discard: bool = True) -> None:
        if self.arg is None:
            raise ValueError("dist_max_aggregate: no forward has stored a selection (keep_arg=False, or none has run)")
        n = self.name
        if not self.exchanging:                     # one rank: every destination is its own, src0 = p_0 = 0
            ops.agg_max_backward(ctx, self.F_T, self.arg, G_M, G_B, accumulate=not discard, timer=n + "1_agg-max")
            return
        if self._rec_ready is None:
            self.start_backward(ctx, G_M)
        (ready, rec_all), self._rec_ready = self._rec_ready, None
        ctx.wait(ready, 0)
        ops.agg_max_backward_rec(ctx, self.F_T, rec_all, G_M.m(), G_B, accumulate=not discard, src0=self.row0,
                                 timer=n + "1_agg-max")


class dist_sage_layer(sage_layer):
    """sage.sage_layer on this rank's rows: two dist_row_linear, gcn.layer_norm with its gradient rows in ``lin.extra`` and
    ``agg``, a dist_max_aggregate or a _rank_aggregation.  ``row0`` = p_r: the rank drops its rows of the global mask."""

    def __init__(self, dctx: dist_context, name: str, agg, n: int, in_: int, out: int, activation: bool, first: bool,
                 G_M_buffer=None, norm=None, tail_floats: int = 8):
        normed = check_norm(norm) == "layer" and activation
        p = partition_bounds(n, dctx.P)
        rows, dev = p[dctx.rank + 1] - p[dctx.rank], dctx.ctx.device
        # the norm's backward runs before lin.backward, whose all-reduce of [G_W | G_b | tail | G_gamma | G_beta] sums the
        # norm's two gradient rows too
        lin = dist_row_linear(dctx, name, in_, out, not first, True, 2 * out if normed else 0, tail_floats)
        res_lin = dist_row_linear(dctx, name + "root_", in_, out, not first, True)
        with _torch().cuda.device(dev):
            norm_layer = layer_norm(name, rows, out, True, dev, lin.extra, adam_fused=True) if normed else None
            sage_layer.__init__(self, name, agg, rows, in_, out, activation, first, G_M_buffer, norm, lin, res_lin, norm_layer)
        self.n, self.row0 = int(n), int(p[dctx.rank])
        self.AHW = self.Y                               # the layer's output under the name dist_model_base reads

    def __call__(self, dctx: dist_context, H: dist_row_dn_matrix) -> dist_row_dn_matrix:
        return _wrap_local(sage_layer.__call__(self, dctx.ctx, H.local), self.n)

    def backward(self, dctx: dist_context, G: dist_row_dn_matrix) -> Optional[dist_row_dn_matrix]:
        G_out = sage_layer.backward(self, dctx.ctx, G.local)
        return None if G_out is None else _wrap_local(G_out, self.n)

    def finish_backward(self, dctx) -> None:
        self.lin.finish_backward(dctx)
        self.res_lin.finish_backward(dctx)

    def adam_update(self, dctx, lr, beta1, beta2, weight_decay, eps):
        sage_layer.adam_update(self, dctx.ctx, lr, beta1, beta2, weight_decay, eps)


class dist_sage(dist_model_base):
    """sage.sage on the row partition.

    dist_sage(dctx, A, A_T, sizes, aggr="mean", loss="softmax", fused=True, weights=None, dropout=0.0, norm=None,
    mode="allgather"): ``A`` / ``A_T`` are the dist_row_csr_matrix pair dist_gcn and dist_gat take (the forward aggregates
    over A_T's rows; for "mean" the caller has normalised them, as for dist_gcn, for "max" the values are ignored);
    ``mode``: the schedule of the mean aggregator's exchange (dist_sparse_linear), "allgather" only for "max"; everything
    else means what it means on sage.  Every rank calls every method with the same arguments.  See the module's text for
    what is refused and what is not built."""

    def __init__(self, dctx: dist_context, A: dist_row_csr_matrix, A_T: dist_row_csr_matrix, sizes: Sequence[int],
                 aggr: str = "mean", loss: str = "softmax", fused: bool = True, weights=None, dropout: float = 0.0, norm=None,
                 mode: str = "allgather"):
        self.aggr = check_aggr(aggr)                         # option checks come before any device work or collective
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}, not {mode!r}")
        if self.aggr == "max" and mode != "allgather":
            raise ValueError(f"mode={mode!r}: aggr=\"max\" has the \"allgather\" schedule only")
        if not (A.n() == A.m() == A_T.n() == A_T.m()):
            raise ValueError(f"A and A_T must be a square matrix and its transpose, got {A.n()} x {A.m()} and {A_T.n()} x {A_T.m()}")
        n = A.n()
        p = partition_bounds(n, dctx.P)                      # n % P != 0: ValueError
        self._init_dropout(dropout, len(sizes) - 1)
        self.norm = check_norm(norm)
        self.loss = check_loss(loss)
        self.sizes = [int(s) for s in sizes]
        self.mode, self._out_width, self.fused, self._adam, self._loss_host = mode, self.sizes[-1], bool(fused), None, None
        torch = _torch()
        P, dev = dctx.P, dctx.ctx.device
        n_layers = len(self.sizes) - 1
        self.n, self.row0 = n, p[dctx.rank]
        rows = n // P
        self.loss_layer = dist_row_softmax_cross_entropy_loss(f"{n_layers}_", True, True, self.loss)
        widest = max(self.sizes[1:-1], default=1)            # the widest input of a layer that has an input gradient
        self.G_M_buffer = torch.empty(rows * widest, dtype=torch.float32, device=dev) if n_layers > 1 else None
        exchanging = P > 1 or dctx.self_gather
        self._plan_wants = []
        if self.aggr == "mean":
            max_d = max(self.sizes[:-1])
            big = n * max_d if mode in ("allgather", "halo") else rows * max_d
            self.bcast_buffer = torch.empty(big, dtype=torch.float32, device=dev)
            self.bcast_buffer2 = torch.empty(rows * max_d, dtype=torch.float32, device=dev)
            for l in range(n_layers):
                w = self.sizes[l]
                for M in ([A_T] if l == 0 else [A_T, A]):
                    parts = list(M.blocks) if mode == "rounds" else \
                        [M.diag] + (list(M.remote_chunks) if mode == "allgather" and P > 1 else [])
                    self._plan_wants += [(blk, max(w, 128), w) for blk in parts]
        else:
            self.F = A_T.row_block_global()
            self.F_T = sorted_row_block(A.row_block_global()) if n_layers > 1 else None
            # the gathered input and the records: one buffer each for the layers above the first (layer 0's gathered
            # features are allocated for its one-time aggregate and released)
            many = exchanging and n_layers > 1
            self.H_all_buffer = torch.empty(n * widest, dtype=torch.float32, device=dev) if many else None
            self.rec_buffer = torch.empty(rows * widest * 2, dtype=torch.int32, device=dev) if many else None
            self.rec_all_buffer = torch.empty(n * widest * 2, dtype=torch.int32, device=dev) if many else None
        self.layers_: List[dist_sage_layer] = []
        for l in range(n_layers):
            name, last = f"{l}_", l + 1 == n_layers
            if self.aggr == "mean":
                agg = _rank_aggregation(dctx, dist_sparse_linear(name, A_T, A, self.bcast_buffer, self.bcast_buffer2, mode))
                agg.A = agg.op.A                        # sage_layer keys layer 0's kept aggregate on the matrix it walks
            else:
                agg = dist_max_aggregate(dctx, name, self.F, self.F_T if l else None, l > 0, self.H_all_buffer,
                                         self.rec_buffer, self.rec_all_buffer)
            self.layers_.append(dist_sage_layer(dctx, name, agg, n, self.sizes[l], self.sizes[l + 1], not last, l == 0,
                                                self.G_M_buffer, self.norm,
                                                ops.BCE_SUMS if self.loss == "bce" and last else 8))
        if weights is not None:
            if len(weights) != n_layers or any(len(w) != 4 for w in weights):
                raise ValueError(f"weights must be (W_l, b_l, W_r, b_r) for each of the {n_layers} layers")
            for layer, (W_l, b_l, W_r, b_r) in zip(self.layers_, weights):
                layer.lin.W.init(np.asarray(W_l, dtype=np.float32))
                layer.lin.b.init(np.asarray(b_l, dtype=np.float32))
                layer.res_lin.W.init(np.asarray(W_r, dtype=np.float32))
                layer.res_lin.b.init(np.asarray(b_r, dtype=np.float32))

    def __call__(self, dctx, H, training: bool = False):
        if self._plan_wants:                          # first call: this rank's SpMM plans, side by side (see dist_gcn)
            shared = dctx.P > 1 and dctx.overlap
            if shared:
                dctx.ctx.lib.mggcn_spmm_plan_reserved_cus(12)
            try:
                ops.prebuild_plans(dctx.ctx, self._plan_wants)
            finally:
                if shared:
                    dctx.ctx.lib.mggcn_spmm_plan_reserved_cus(0)
            self._plan_wants = []
        return dist_model_base.__call__(self, dctx, H, training)

    def reset_input_cache(self) -> None:
        """drops layer 0's kept aggregate agg(X): the next forward gathers and computes it again"""
        self.layers_[0].reset_input_cache()

    def save(self, dctx, path: str, optimizer: bool = True) -> None:
        refuse_checkpoint("save: the checkpoint file")

    def load(self, dctx, path: str) -> None:
        refuse_checkpoint("load: the checkpoint file")

    def _write_checkpoint(self, dctx, path: str, tensors, optimizer: bool, step: int) -> None:
        refuse_checkpoint("the checkpoint file (model_selector.save_best included)")
