"""The GAT model on the 1D row partition: one process per GPU, the classes of gat.py on this rank's rows (opt-in; the
reference has no attention layer).  DESIGN.md 3.10.1 has the algebra, the bytes and the measurements.

Rank r owns rows [p_r, p_{r+1}) of every activation; W, b and att are replicated.  The three sparse kernels walk a whole
row of F (forward, backward_dst) or of F^T (backward_src) in one piece, so a rank runs them over ITS row block of each
matrix with global column indices (dist_row_csr_matrix.row_block_global), and what it needs of the other ranks is gathered
first:

  forward    Z_loc = H_loc W + b; ONE all-gather gives Z_all [n x out] (kept until the layer's backward has run); one scores
             launch over Z_all gives s_dst_all and s_src_all (cheaper than a collective); gat_forward over the row block of
             F with Z_all, the rank's rows of s_dst_all and s_src_all gives out_loc and lse_loc.
  backward   the all-gather of G_loc into G_all starts at once on the comm stream; backward_dst runs meanwhile (it needs
             nothing remote beyond Z_all) and gives D_loc, ds_dst_loc; the rank packs (s_dst, lse, D) of its destinations
             into 16-byte records (ops.gat_pack_dst) and ONE all-gather of 16 x heads bytes per vertex delivers the records
             of all destinations; backward_src over the row block of F^T (rows: local sources, columns: global
             destinations) reads G_all and the records and gives ds_src_loc, G_Z_loc; scores_backward over the rank's rows
             gives the rank's PARTIAL G_att, which lives in the ``extra`` floats of the layer's dist_row_linear and is
             summed over the ranks by that layer's gradient all-reduce -- no collective of its own.

Every row of F and of F^T is walked by one rank, whole, in the order the single-GPU kernel walks it: out, lse, D, ds_dst,
ds_src and G_Z are the single-GPU rows bit for bit at any P (given the same Z and G), with attention dropout too -- the
mask is drawn with dst0 = p_r, src0 = 0 over F and dst0 = 0, src0 = p_r over F^T.  Only sums over vertices (G_W, G_b, G_att,
the loss sums) round differently.  A single rank exchanges nothing unless dist_context.self_gather.

dist_gat is gat.attention_model (set_dropout, the masks, attention_weights: what gat has too) over dist.dist_model_base (the
epoch of dist_gcn); of the mix-in it answers one hook, _mask_origin() = (p_r, 0).

attention_weights / attention_pattern: a rank exports the coefficients of its rows' entries (gat.attention_model's
attention_weights on the row block; no collective of its own), the single-GPU export's rows bit for bit: one [nnz of the rank's
row block x heads] dn_matrix per requested layer, the rows [indptr[p_r], indptr[p_{r+1}]) of the single-GPU model's export.

``variant="v2"`` (GATv2): the layer's one linear gives Z2_loc = [Zs | Zd] of 2 out columns and ONE
all-gather of that shard gives Z2_all, of which the forward and backward_dst over the row block of F read the Zs half
(global sources; Zd is the rank's own) and backward_src over the row block of F^T reads the Zd half (global destinations;
Zs is the rank's own).  Gathering both halves in the forward costs out x 4 bytes per vertex more than v1 in a forward that
no backward follows, and saves a collective in every backward.  backward_dst needs nothing remote beyond Z2_all and runs
under the all-gather of G_loc; its rows' shares P of G_att are summed into the rank's PARTIAL G_att (in ``extra``, as
above); the rank packs (lse, D) of its destinations into 8-byte records (ops.gatv2_pack_dst) and ONE all-gather of 8 x
heads bytes per vertex delivers all of them to backward_src (ops.gatv2_backward_src_rec).  out, lse, D, P, G_Zd and G_Zs
are the single-GPU rows bit for bit at any P.  No attention dropout (refused, as gat refuses it).

save / load / predict (checkpoint.checkpoint_option): every rank calls them; rank 0 writes its replica of W, b and att and
every rank reads the file, so a gat file loads here at any P and the other way round; predict returns the rank's rows.

Not covered: the halo and rounds schedules, bf16 on the wire, layer norm, the C++ host layer."""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np

from . import ops
from .dist import (_repl_view, _torch, _wrap_local, dist_context, dist_model_base, dist_row_csr_matrix, dist_row_dn_matrix,
                   dist_row_linear, dist_row_softmax_cross_entropy_loss, partition_bounds)
from .gat import (attention, attention_model, attention_v2, check_heads, check_single_gpu_variant, check_variant,
                  gat_layer)
from .gcn import check_dropout, check_loss
from .matrix import context, csr_matrix, dn_matrix


class dist_attention(attention):
    """gat.attention on one rank's rows: ``att`` replicated, the scores of ALL vertices (s_dst_all, s_src_all [n x heads];
    s_dst / s_src are views of the rank's rows), lse, D, ds_dst, ds_src of the rank's rows, and the three exchanges.

    ``grad_buffer``: 2 x out floats that some all-reduce sums over the ranks (the layer's dist_row_linear.extra) -- G_att
    lives there and is this rank's partial until then; None allocates it.  ``G_all_buffer`` (n x out floats) and
    ``rec_buffer`` (n x heads x 4 floats, 16-byte aligned) may be shared by the layers of a model: a layer's gather into
    them is ordered on the comm stream after everything the compute stream has queued, the previous layer's backward_src
    included.  Z_all is this layer's own: it is written in the forward and read until the backward, so a second forward
    before the backward overwrites it, as gat_layer's Z is."""

    def __init__(self, dctx: dist_context, name: str, n: int, out: int, heads: int, slope: float = ops.GAT_SLOPE,
                 grad_buffer=None, G_all_buffer=None, rec_buffer=None):
        torch = _torch()
        p = partition_bounds(n, dctx.P)
        dev = dctx.ctx.device
        self.n, self.rows, self.row0 = int(n), p[dctx.rank + 1] - p[dctx.rank], p[dctx.rank]
        attention.__init__(self, name, self.rows, self.rows, out, heads, slope, dev)
        self._dctx = dctx
        self.exchanging = dctx.P > 1 or dctx.self_gather
        if grad_buffer is not None:
            self.G_att = dn_matrix(2, out, grad_buffer)
        K, lo, hi = self.heads, self.row0, self.row0 + self.rows
        self.s_dst_all, self.s_src_all = dn_matrix(n, K, device=dev), dn_matrix(n, K, device=dev)
        self.s_dst, self.s_src = dn_matrix(self.rows, K, self.s_dst_all.t[lo:hi]), dn_matrix(self.rows, K, self.s_src_all.t[lo:hi])
        self.rec = torch.empty(self.rows * K * 4, dtype=torch.float32, device=dev)
        self.Z_all = self.G_all = None
        self.rec_all = self.rec
        if self.exchanging:
            self.Z_all = dn_matrix(n, out, device=dev)
            self.G_all = dn_matrix(n, out, G_all_buffer) if G_all_buffer is not None else dn_matrix(n, out, device=dev)
            self.rec_all = (rec_buffer if rec_buffer is not None else torch.empty(n * K * 4, dtype=torch.float32, device=dev))[:n * K * 4]

    def _exchange(self, shard, out, tag: str) -> str:
        """the all-gather of this rank's [rows x d] ``shard`` into ``out`` [n x d] on the comm stream, after everything the
        compute stream has queued so far -- the producer of the shard and the last reader of ``out``; all_gather_rows
        orders neither.  Returns the event that marks the gathered ``out``; timer: the collective on the comm stream."""
        dctx, ctx, tag = self._dctx, self._dctx.ctx, self.name + tag
        cs = dctx.bcast_stream_id()
        ctx.record(tag + "_ready", 0)
        ctx.wait(tag + "_ready", cs)
        ctx.record(tag + "_0", cs)
        dctx.all_gather_rows(shard, out, cs).wait(cs)
        ctx.record(tag + "_1", cs)
        ctx.register_timer(tag, tag + "_0", tag + "_1")
        return tag + "_1"

    def __call__(self, ctx: context, F: csr_matrix, Z: dn_matrix, out: dn_matrix, drop=None) -> None:
        """out = the attention-weighted gather over ``F``, the rank's row block of the forward matrix ([n/P x n], global
        columns), of the rows of Z_all that ``Z``, the rank's rows, is gathered into.  ``drop``: the tuple of
        ops.gat_forward with dst0 = the rank's first row and src0 = 0 (None: the plain entry points)"""
        n = self.name
        if self.exchanging:
            ctx.wait(self._exchange(Z.t, self.Z_all.t, "0_gat-exchange"), 0)
        else:
            self.Z_all = Z
        ops.gat_scores(ctx, self.Z_all, self.att, self.s_dst_all, self.s_src_all, self.heads, n + "0_gat-scores")
        ops.gat_forward(ctx, F, self.Z_all, self.s_dst, self.s_src_all, out, self.lse, self.heads, self.slope,
                        n + "0_gat-forward", drop)

    def alpha(self, ctx: context, F: csr_matrix, Z: dn_matrix, alpha: dn_matrix) -> None:
        """alpha [F.nnz() x heads] = the coefficients of the most recent forward over ``F``, the rank's row block: s_dst and
        lse of the rank's rows, s_src of all vertices -- every value is the single-GPU export's, bit for bit, because the
        scores and lse are.  No collective."""
        ops.gat_alpha(ctx, F, self.s_dst, self.s_src_all, self.lse, alpha, self.heads, self.slope, self.name + "0_gat-alpha")

    def backward(self, ctx: context, F: csr_matrix, F_T: csr_matrix, Z: dn_matrix, G: dn_matrix, out: dn_matrix,
                 G_Z: dn_matrix, drop=None) -> None:
        """G_Z = the gradient of the rank's rows of Z, and this rank's partial G_att, from G = the gradient of ``out``;
        ``F_T``: the rank's row block of F^T; ``drop``: what the forward was called with (backward_src, whose rows are
        sources, takes it with dst0 and src0 swapped)"""
        n, K = self.name, self.heads
        G_all, ready = G, None
        if self.exchanging:
            ready, G_all = self._exchange(G.t, self.G_all.t, "1_gat-exchange-G"), self.G_all
        ops.gat_backward_dst(ctx, F, self.Z_all, self.s_dst, self.s_src_all, self.lse, G, out, self.D, self.ds_dst, K,
                             self.slope, n + "1_gat-backward-dst", drop)
        ops.gat_pack_dst(ctx, self.s_dst, self.lse, self.D, self.rec)
        if self.exchanging:
            ctx.wait(self._exchange(self.rec.view(self.rows, K * 4), self.rec_all.view(self.n, K * 4), "1_gat-exchange-rec"), 0)
            ctx.wait(ready, 0)
        drop_src = None if drop is None else (*drop[:4], drop[5], drop[4])
        # ds_dst is the rank's own: backward_src indexes it by row, and its rows are the rank's sources
        ops.gat_backward_src_rec(ctx, F_T, Z, self.rec_all, self.s_src, G_all, self.att, self.ds_dst, self.ds_src, G_Z, K,
                                 self.slope, n + "1_gat-backward-src", drop_src)
        ops.gat_scores_backward(ctx, self.ds_dst, Z, self.ds_src, Z, self.G_att, K, n + "1_gat-scores-backward")


class dist_gat_layer(gat_layer):
    """gat.gat_layer on this rank's rows: a dist_row_linear, a dist_attention over the rank's row blocks ``F`` / ``F_T``
    ([n/P x n] csr_matrix, global columns) and the activation.  The rank's partial G_att sits behind [G_W | G_b | tail] in
    the linear's gradient buffer: attention.backward runs before lin.backward, whose all-reduce therefore sums it too."""

    def __init__(self, dctx: dist_context, name: str, F: csr_matrix, F_T: csr_matrix, in_: int, out: int, heads: int,
                 activation: bool, slope: float = ops.GAT_SLOPE, backward_out: bool = True, G_Z_buffer=None,
                 G_all_buffer=None, rec_buffer=None, tail_floats: int = 8):
        n, dev = F.m(), dctx.ctx.device
        assert F.n() == F_T.n() and F_T.m() == n, "the rank's row blocks of a square matrix and of its transpose"
        lin = dist_row_linear(dctx, name, in_, out, backward_out, True, 2 * out, tail_floats)
        attn = dist_attention(dctx, name, n, out, heads, slope, lin.extra, G_all_buffer, rec_buffer)
        # row0: dropout -- this rank draws ITS rows of the global mask
        self._setup(name, F, F_T, lin, attn, attn.rows, in_, out, activation, G_Z_buffer, dev, attn.row0)
        self.n = n
        self.AHW = self.act                             # the layer's output under the name dist_gcn's plumbing reads

    def __call__(self, dctx: dist_context, H: dist_row_dn_matrix) -> dist_row_dn_matrix:
        return _wrap_local(gat_layer.__call__(self, dctx.ctx, H.local), self.n)

    def backward(self, dctx: dist_context, G: dist_row_dn_matrix) -> Optional[dist_row_dn_matrix]:
        G_out = gat_layer.backward(self, dctx.ctx, G.local)
        return None if G_out is None else _wrap_local(G_out, self.n)

    def finish_backward(self, dctx) -> None:
        self.lin.finish_backward(dctx)

    def adam_update(self, dctx, lr, beta1, beta2, weight_decay, eps):
        gat_layer.adam_update(self, dctx.ctx, lr, beta1, beta2, weight_decay, eps)

    def alpha(self, dctx: dist_context, out: Optional[dn_matrix] = None) -> dn_matrix:
        return gat_layer.alpha(self, dctx.ctx, out)

    def att(self): return _repl_view(self.attn.att)
    def Gatt(self): return _repl_view(self.attn.G_att)


class dist_attention_v2(attention_v2):
    """gat.attention_v2 on one rank's rows: ``att`` replicated, lse, D and P of the rank's rows, and the three exchanges.
    __call__ and backward take the rank's Z2 = [Zs | Zd] and G_Z2 = [G_Zs | G_Zd] of 2 out columns.

    ``grad_buffer``: out floats that some all-reduce sums over the ranks (the layer's dist_row_linear.extra) -- G_att
    lives there and is this rank's partial until then; None allocates it.  ``G_all_buffer`` (n x out floats) and
    ``rec_buffer`` (n x heads x 2 floats, 8-byte aligned) may be shared by the layers of a model, ``P_buffer`` (rows x
    out) too: see dist_attention.  Z2_all [n x 2 out] is this layer's own, written in the forward and read until the
    backward.  A rank that exchanges nothing has Z2_all = Z2, G_all = G and rec_all = rec.  ``packed``: backward_src
    reads the record -- always: a single rank that exchanges nothing packs and reads its own, which measured 4.5 ms faster
    per 128-wide layer than the plain call and gives the same bits (profiles/experiments/dist_gatv2.py
    sets it to False on such a rank to take that measurement)."""

    def __init__(self, dctx: dist_context, name: str, n: int, out: int, heads: int, slope: float = ops.GAT_SLOPE,
                 grad_buffer=None, G_all_buffer=None, rec_buffer=None, P_buffer=None):
        torch = _torch()
        p = partition_bounds(n, dctx.P)
        dev = dctx.ctx.device
        self.n, self.rows, self.row0 = int(n), p[dctx.rank + 1] - p[dctx.rank], p[dctx.rank]
        attention_v2.__init__(self, name, self.rows, out, heads, slope, P_buffer, dev)
        self._dctx = dctx
        self.exchanging = dctx.P > 1 or dctx.self_gather
        self.packed = True
        if grad_buffer is not None:
            self.G_att = dn_matrix(1, out, grad_buffer)
        K = self.heads
        self.rec = torch.empty(self.rows * K * 2, dtype=torch.float32, device=dev)
        self.Z2_all = self.G_all = None
        self.rec_all = self.rec
        if self.exchanging:
            self.Z2_all = dn_matrix(n, 2 * out, device=dev)
            self.G_all = dn_matrix(n, out, G_all_buffer) if G_all_buffer is not None else dn_matrix(n, out, device=dev)
            self.rec_all = (rec_buffer if rec_buffer is not None else torch.empty(n * K * 2, dtype=torch.float32, device=dev))[:n * K * 2]

    _exchange = dist_attention._exchange            # reads _dctx and name

    def __call__(self, ctx: context, F: csr_matrix, Z2: dn_matrix, out: dn_matrix, drop=None) -> None:
        """out = the attention-weighted gather over ``F``, the rank's row block of the forward matrix ([n/P x n], global
        columns), of the Zs half of Z2_all, which ``Z2``, the rank's rows, is gathered into, scored against the rank's Zd"""
        assert drop is None, "GATv2 has no attention dropout"
        if self.exchanging:
            ctx.wait(self._exchange(Z2.t, self.Z2_all.t, "0_gatv2-exchange"), 0)
        else:
            self.Z2_all = Z2
        ops.gatv2_forward(ctx, F, self.Z2_all, Z2, self.att, out, self.lse, self.heads, self.slope, self.name + "0_gatv2-forward")

    def alpha(self, ctx: context, F: csr_matrix, Z2: dn_matrix, alpha: dn_matrix) -> None:
        """alpha [F.nnz() x heads] = the coefficients of the most recent forward over ``F``, the rank's row block: Zs of all
        vertices (Z2_all), Zd and lse of the rank's rows -- the single-GPU export's values bit for bit.  No collective."""
        ops.gatv2_alpha(ctx, F, self.Z2_all, Z2, self.att, self.lse, alpha, self.heads, self.slope, self.name + "0_gatv2-alpha")

    def backward(self, ctx: context, F: csr_matrix, F_T: csr_matrix, Z2: dn_matrix, G: dn_matrix, out: dn_matrix,
                 G_Z2: dn_matrix, drop=None) -> None:
        """G_Z2 = the gradient of the rank's rows of Z2 (both halves), and this rank's partial G_att, from G = the gradient
        of ``out``; ``F_T``: the rank's row block of F^T"""
        assert drop is None, "GATv2 has no attention dropout"
        n, K = self.name, self.heads
        G_all, ready = G, None
        if self.exchanging:
            ready, G_all = self._exchange(G.t, self.G_all.t, "1_gatv2-exchange-G"), self.G_all
        ops.gatv2_backward_dst(ctx, F, self.Z2_all, Z2, self.att, self.lse, G, out, self.D, G_Z2, self.P, K, self.slope,
                               n + "1_gatv2-backward-dst")
        ops.gatv2_att_grad(ctx, self.P, self.G_att, n + "1_gatv2-att-grad")
        if not self.packed:                         # one rank, nothing exchanged: lse and D of all destinations are its own
            assert not self.exchanging, "a layer that exchanges reads the gathered record"
            ops.gatv2_backward_src(ctx, F_T, Z2, self.Z2_all, self.att, self.lse, self.D, G_all, G_Z2, K, self.slope,
                                   n + "1_gatv2-backward-src")
            return
        ops.gatv2_pack_dst(ctx, self.lse, self.D, self.rec)
        if self.exchanging:
            ctx.wait(self._exchange(self.rec.view(self.rows, K * 2), self.rec_all.view(self.n, K * 2), "1_gatv2-exchange-rec"), 0)
            ctx.wait(ready, 0)
        # rows: the rank's sources (its own Zs half), columns: global destinations (the Zd half of Z2_all, G_all, the records)
        ops.gatv2_backward_src_rec(ctx, F_T, Z2, self.Z2_all, self.att, self.rec_all, G_all, G_Z2, K, self.slope,
                                   n + "1_gatv2-backward-src")


class dist_gatv2_layer(dist_gat_layer):
    """gat.gatv2_layer on this rank's rows: ONE dist_row_linear of 2 out columns, a dist_attention_v2 over the rank's row
    blocks and the activation.  The rank's partial G_att [1 x out] sits behind [G_W | G_b | tail] in the linear's gradient
    buffer, as dist_gat_layer's does; everything but the construction is dist_gat_layer's."""

    def __init__(self, dctx: dist_context, name: str, F: csr_matrix, F_T: csr_matrix, in_: int, out: int, heads: int,
                 activation: bool, slope: float = ops.GAT_SLOPE, backward_out: bool = True, G_Z_buffer=None,
                 G_all_buffer=None, rec_buffer=None, tail_floats: int = 8, P_buffer=None):
        n, dev = F.m(), dctx.ctx.device
        assert F.n() == F_T.n() and F_T.m() == n, "the rank's row blocks of a square matrix and of its transpose"
        lin = dist_row_linear(dctx, name, in_, 2 * out, backward_out, True, out, tail_floats)
        attn = dist_attention_v2(dctx, name, n, out, heads, slope, lin.extra, G_all_buffer, rec_buffer, P_buffer)
        self._setup(name, F, F_T, lin, attn, attn.rows, in_, out, activation, G_Z_buffer, dev, attn.row0, z_width=2 * out)
        self.n = n
        self.AHW = self.act


class dist_gat(attention_model, dist_model_base):
    """gat.gat on the row partition.

    dist_gat(dctx, A, A_T, sizes, heads=4, attn_slope=0.2, loss="softmax", fused=True, weights=None, dropout=0.0,
    attn_dropout=0.0, variant="v1"): ``A`` / ``A_T`` are the dist_row_csr_matrix pair dist_gcn takes (load_rank_local feeds
    both; the layers aggregate over A_T's pattern, values are ignored), everything else means what it means on gat --
    ``variant``: "v1" (this model as it always was) or "v2" (GATv2: W is [in x 2 out], b [1 x 2 out], att [1 x out]; no
    attention dropout).  ValueError before any device work or collective, on every rank alike, for what gat refuses (an
    unknown variant, "v2" with attn_dropout > 0 and set_dropout(attn > 0) on a v2 model among it), for variant="dot"
    (dot-product attention has no row-partitioned form yet) and for n % P != 0.

    Every rank calls every method with the same arguments.  set_dropout(p, seed, epoch, attn): a rank drops its rows of
    the masks the single-GPU model draws (feature dropout with row0 = p_r; attention dropout see the module docstring).
    __call__, train_forward, backward, adam_update, train_step (one synchronisation; the loss sums ride on the last layer's
    gradient all-reduce), set_splits(dctx, Sd), split_metrics and layers() are dist.dist_model_base's, as for dist_gcn, which
    has no evaluate() either: a plain call is the forward that never drops.  save(dctx, path, optimizer=True) / load(dctx, path) /
    predict(dctx, X): see checkpoint.checkpoint_option -- a refused load raises on every rank alike, before any collective."""

    def __init__(self, dctx: dist_context, A: dist_row_csr_matrix, A_T: dist_row_csr_matrix, sizes: Sequence[int], heads=4,
                 attn_slope: float = ops.GAT_SLOPE, loss: str = "softmax", fused: bool = True, weights=None,
                 dropout: float = 0.0, attn_dropout: float = 0.0, variant: str = "v1"):
        self.sizes = [int(s) for s in sizes]
        self.heads = check_heads(self.sizes, heads)              # option checks come before any device work or collective
        n_layers = len(self.sizes) - 1
        self._attn_dropout_params = check_dropout(attn_dropout, n_layers)
        self.variant = check_variant(variant, float(attn_dropout))
        check_single_gpu_variant(self.variant)                   # "dot": refused on every rank alike
        self._init_dropout(dropout, n_layers)
        self.attn_dropout_p = float(attn_dropout)
        self.loss = check_loss(loss)
        if not (A.n() == A.m() == A_T.n() == A_T.m()):
            raise ValueError(f"dist_gat needs a square matrix and its transpose, got {A.n()} x {A.m()} and {A_T.n()} x {A_T.m()}")
        n = A.n()
        p = partition_bounds(n, dctx.P)
        self.attn_slope, self._out_width, self.fused, self._adam, self._loss_host = float(attn_slope), self.sizes[-1], bool(fused), None, None
        torch = _torch()
        dev = dctx.ctx.device
        self.n, self.row0 = n, p[dctx.rank]
        self.loss_layer = dist_row_softmax_cross_entropy_loss(f"{n_layers}_", True, True, self.loss)
        self.F, self.F_T = A_T.row_block_global(), A.row_block_global()          # forward over A_T's rows, like gcn
        widest = max(self.sizes[1:])
        exchanging = dctx.P > 1 or dctx.self_gather
        v2 = self.variant == "v2"                                # G_Z2 = [G_Zs | G_Zd] and P, once at the widest layer
        self.G_Z_buffer = torch.empty(n // dctx.P * widest * (2 if v2 else 1), dtype=torch.float32, device=dev)
        if v2:
            self.P_buffer = torch.empty(n // dctx.P * widest, dtype=torch.float32, device=dev)
        # the gathered gradient and the gathered records: one buffer each for all layers (Z_all is per layer)
        self.G_all_buffer = torch.empty(n * widest, dtype=torch.float32, device=dev) if exchanging else None
        self.rec_buffer = torch.empty(n * max(self.heads) * (2 if v2 else 4), dtype=torch.float32, device=dev) if exchanging else None
        self.layers_: List[dist_gat_layer] = []
        for i in range(n_layers):
            last = i + 1 == n_layers
            args = (dctx, f"{i}_", self.F, self.F_T, self.sizes[i], self.sizes[i + 1], self.heads[i], not last, self.attn_slope,
                    i != 0, self.G_Z_buffer, self.G_all_buffer, self.rec_buffer, ops.BCE_SUMS if self.loss == "bce" and last else 8)
            self.layers_.append(dist_gatv2_layer(*args, self.P_buffer) if v2 else dist_gat_layer(*args))
        if weights is not None:
            assert len(weights) == n_layers
            for layer, w in zip(self.layers_, weights):
                layer.W().local.init(np.asarray(w[0], dtype=np.float32))
                layer.b().local.init(np.asarray(w[1], dtype=np.float32))
                if len(w) > 2:
                    layer.attn.init(w[2])

    def _mask_origin(self):
        """the rank's row block of the forward matrix: destinations from the rank's first row, every source"""
        return self.row0, 0

    def attention_pattern(self):
        """(indptr, indices): the host arrays of the rank's row block of the matrix the forward walks -- row i is the
        rank's destination p_r + i, its entries are its sources as GLOBAL vertex numbers, and row p of every matrix
        attention_weights returns belongs to indices[p]"""
        return self.F.indptr, self.F.indices
