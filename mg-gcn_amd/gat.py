"""Graph attention (GAT) layers over the HIP engine, single GPU (opt-in; the reference has no attention layer).

A layer of ``heads = K`` heads of width ``dh`` (``out = K * dh``) computes, over the pattern of the matrix the GCN forward
aggregates with (F = A.transpose(): row i lists the sources j of destination i; values are ignored, a duplicate entry
counts as two edges):

    Z = H W + 1 b^T                                   (the existing ``linear``; always GEMM first)
    s_dst[i, k] = Z[i, head k] . att[0, head k]       s_src[j, k] = Z[j, head k] . att[1, head k]
    e_ijk = lrelu(s_dst[i, k] + s_src[j, k], slope)   alpha_ijk = softmax over the entries j of row i
    out[i, head k] = sum_j alpha_ijk Z[j, head k]

and every layer but the last applies the project's leaky ReLU (0.01) afterwards.  The bias sits inside Z and so enters the
scores (PyG adds its bias after the aggregation instead).  The kernels are those of csrc/gat.hip (include/mggcn.h:
mggcn_gat_*): nothing of nnz x heads is stored, the backward pass recomputes alpha from s_dst, s_src and lse.

Two dropouts (opt-in, both 0 by default: nothing new is launched or allocated), in training forwards only:
  * ``dropout=p``: the input of every layer but the first goes through ops.dropout_raw, and so does the gradient that layer
    returns -- gcn's convention, stream = epoch * 64 + layer; the features are never dropped;
  * ``attn_dropout=p``: every layer's normalised coefficients, the first layer's included, are multiplied by
    q_ijk = keep ? 1 / (1 - p) : 0 in the gather (out = sum_j alpha q Z; the softmax still runs over all entries), with a
    Philox mask on (seed, the same stream number, destination, source, head) that the three sparse kernels regenerate
    (mggcn_gat_*_drop_f32) -- no edge mask is stored.  Duplicate entries (i, j) share one bit.
set_dropout(p, seed, epoch, attn) sets both; evaluate() and a plain call never drop.

The row-partitioned form is dist_gat.dist_gat (one process per GPU; DESIGN.md 3.10 "The row partition").

``variant="v2"`` selects GATv2 (dynamic attention; Brody, Alon, Yahav 2022; PyG's GATv2Conv) in every layer:

    Z2 = H W + 1 b^T, W [in x 2 out]                  Zs = Z2[:, :out] (PyG's lin_l)   Zd = Z2[:, out:] (lin_r)
    e_ijk = att[head k] . lrelu(Zd[i, head k] + Zs[j, head k], slope)     att [1 x out]
    alpha_ijk = softmax over the entries j of row i   out[i, head k] = sum_j alpha_ijk Zs[j, head k]

The non-linearity sits inside the dot product, so a destination can rank its sources in an order of its own, which the
v1 score (monotone in s_src[j]) cannot.  One GEMM forward, the linear's fused gradient GEMMs backward; the kernels are
those of csrc/gatv2.hip (mggcn_gatv2_*).  The default ``variant="v1"`` is the model described above and calls exactly what
it called before the keyword existed.  GATv2 has no attention dropout (refused); its
row-partitioned form is dist_gat.dist_gat(variant="v2").

The coefficients can be written out: gat.attention_weights(ctx, X) returns one [nnz x heads] matrix per layer (PyG's
return_attention_weights), attention_pattern() the (indptr, indices) their rows belong to; gat_layer.alpha is the layer's.
The values are the backward kernels' own expression exp(e - lse) (mggcn_gat_alpha_f32 / mggcn_gatv2_alpha_f32); nothing is
allocated or launched unless one of these is called.

``variant="dot"`` selects dot-product (transformer) attention (Vaswani et al. 2017; Shi et al. 2021, UniMP; PyG's
TransformerConv without its root weight, gate and edge features) in every layer:

    Z3 = H W + 1 b^T, W [in x 3 out]                  Zq = Z3[:, :out]   Zk = Z3[:, out:2 out]   Zv = Z3[:, 2 out:]
    e_ijk = c (Zq[i, head k] . Zk[j, head k]),  c = fp32(1 / sqrt(dh))
    alpha_ijk = softmax over the entries j of row i   out[i, head k] = sum_j alpha_ijk Zv[j, head k]

The score is the scaled dot product of the destination's query and the source's key, the aggregated row is the source's
value; the attention has no parameter of its own (a layer's parameters are W and b).  One GEMM forward, the linear's fused
gradient GEMMs backward over 3 out columns; the kernels are those of csrc/gatdot.hip (mggcn_gatdot_*).  ``weights=`` takes
(W [in x 3 out], b [1 x 3 out]) per layer.  Refused with ValueError before any device work: attention dropout, the export
(attention_weights, gat_layer.alpha), save / load (the checkpoint file has no version for this variant yet; model_selector's
in-memory restore works, save_best does not), dist_gat(variant="dot"), and a graph so large that rows x 3 x the widest
layer reaches 2^31 elements (the limit of the GEMM's output).  predict, evaluate, split_metrics and model_selector work
unchanged.

The model is gcn.model_base (the epoch, splits, evaluate: what gcn is too) under attention_model, the mix-in dist_gat.dist_gat
shares: set_dropout, the arming of the two masks and attention_weights.  Every trained tensor is one row of its owner's
gcn.param_owner table -- att of attention and attention_v2, w of gated_skip, nothing of attention_dot -- and a layer lists
its owners (gat_layer.owners): Adam, params() and the checkpoint's names follow from those.

save / load / predict and model_selector are gcn's (checkpoint.checkpoint_option, selection.model_selector): the file stores
the layer type -- variant, heads, attn_slope, the attention dropout probability -- next to W, b and att of every layer
(version 3 of the checkpoint file, INTEGRATION.md "Checkpoint file"), and a resumed run is the uninterrupted run bit for bit
(DESIGN.md 3.10.6).  Nothing is allocated or launched unless one of these is called.

``skip="add" | "gate"`` and ``norm="layer"`` (both None by default: nothing new is launched or allocated) put a skip
connection and a layer normalisation after the aggregation of every variant -- attention -> skip -> norm -> activation:

    r = H W_r + 1 b_r^T                               (``res_lin``: always a linear, PyG's lin_skip; H is what lin reads)
    "add":  y = out + r                               (GATConv(residual=True))
    "gate": g_i = sigmoid(sum_c (w[0,c] out[i,c] + w[1,c] r[i,c] + w[2,c] (out[i,c] - r[i,c])));  y = g r + (1 - g) out
                                                      (TransformerConv(beta=True); w [3 x out], no bias, one g per row)
    norm:   y <- layer_norm(y) with gamma, beta       (gcn's: every layer but the last)

and the layer's leaky ReLU rides in whichever of the two kernels runs last (csrc/gated_skip.hip: mggcn_gated_skip_*; the
norm's are gcn's).  With variant="dot", skip="gate", norm="layer" a layer is the UniMP / graph-transformer block.  W_r and
b_r are trained like any linear's, w with W's weight decay, gamma and beta with none; ``skip_weights=`` takes (W_r, b_r) or
(W_r, b_r, w) per layer, ``layer.res_lin``, ``layer.gate`` (``.w``, the rows' ``.gate``) and ``layer.norm`` hold them.
Refused with ValueError before anything is created, read or written: save, load and model_selector.save_best on a model
with either option (the checkpoint file has no version that stores them; the selector's in-memory restore works), and
dist_gat does not take the arguments.

``label_input=rate`` (0 by default: nothing new is allocated, launched or registered) feeds masked labels into layer 0, the
other half of UniMP and the "label trick" of Wang et al. 2021.  Feeding a label is appending a masked one-hot label to the
features, [X | M onehot(y)] [W ; E] = X W + M E[y], so the feature is a trained table E [classes x width of layer 0's Z]:

    Z[i] += E[y_i] for the fed rows i, after layer 0's GEMM and before its attention (the skip's res_lin sees H only)
    G_E[c] = sum of G_Z[i] over the fed rows of class c            (csrc/label_input.hip: mggcn_label_input_*)

In training forward e a vertex r is fed iff it is in the training set and word 0 of Philox4x32-10((0xFFFFFFFF, r, r >> 32, e),
seed) is below floor(rate 2^32) -- never stored, regenerated by both kernels, no bits shared with dropout -- and the loss runs
over the training rows that were NOT fed: the loss layer sees them in its "other" slot and the counts of the epoch
(train = T - fed, other = other + fed), which the host takes from its own Philox (label_mask) one epoch ahead, under the
device's work.  A plain call, evaluate() and predict() feed every training row.  set_label_input(Y, rate=None, seed=0, epoch=0)
after set_splits hands the model its labels (epoch=e replays training forward e); ``label_input_p``, ``label_seed``,
``label_epoch`` and ``layers()[0].label`` (``.E``) read the state; ``label_weights=`` takes E.  E is a row of the fused Adam
table with W's weight decay, listed by layer 0 alone.  Refused with ValueError naming label_input before any device work: a
rate outside [0, 1), loss="bce", more than ops.LABEL_INPUT_MAX_CLASSES classes, a label outside [0, classes) on a training
row, set_label_input before set_splits, a forward before set_label_input, an epoch that leaves no row to predict, and save /
load / save_best (no version of the checkpoint file stores E; the selector's in-memory restore includes it).  Not built: the
row partition (dist_gat does not take the arguments; the partial G_E would ride on layer 0's all-reduce), the checkpoint
version, gcn, multi-label targets, the C++ layer.

``agg_dtype="bf16"`` (default "f32": nothing new is allocated, launched or registered, the same bits as before) stores the
GATHERED operand of every sparse attention kernel in bf16, as gcn(agg_dtype="bf16") does for its SpMM: every dense operand a
kernel indexes by an entry's column is read from a bf16 image of the fp32 tensor (round to nearest even,
mggcn_convert_f32_bf16), half the bytes per gathered row --

    variant   forward / backward_dst (rows of F)   backward_src (rows of F^T)
    v1        Z                                    G
    v2        Zs                                   Zd, G
    dot       Zk, Zv                               Zq, G

-- and everything else stays fp32 and is read from the fp32 tensor: every operand indexed by the kernel's own row, the scores
kernel and the [n x heads] scalars, all arithmetic and sums, every output, the GEMMs, skip, norm, label input, loss and Adam.
A self-loop entry therefore meets the rounded row in the gathered role and the fp32 row in the own role.  The kernels are the
fp32 kernels with the gathered loads on the image (csrc/*_b16.hip: mggcn_gat*_bf16), so a call equals the fp32 call on the
exactly widened image bit for bit.  The model owns two bf16 buffers shared by all layers, ``Z_image_buffer``
(n x 1 / 2 / 3 x the widest layer) and ``G_image_buffer`` (n x the widest layer); a layer makes its images itself -- forward:
after the GEMM and the label-input embed, immediately before the forward kernel; backward: ALL of the backward pass's images
in one block ahead of backward_dst, i.e. the forward's image again (the layers above have overwritten the shared buffer; same
input, same bits) and with it what backward_src gathers (G, v2 Zd, dot Zq), one kernel early: nothing in between writes Z or
G -- only in the columns that are gathered, under the timers ``<layer>0_gat-convert`` and ``<layer>1_gat-convert``.  evaluate, predict and a plain call run
the bf16 forward; both dropouts, skip=, norm=, label_input=, loss="bce", splits, both Adam modes and model_selector compose.
agg_dtype is an execution option: it is not written to checkpoints, and a file saved by either form loads into the other.
attention_weights on v1 is unchanged (its scores and lse never see an image); on variant="v2" with agg_dtype="bf16"
attention_weights and gatv2_layer.alpha raise ValueError naming agg_dtype before any device work (the export kernel would
score the fp32 Zs against an lse taken over rounded rows).  Not built: dist_gat and bf16 on the wire, bf16 record forms, the
v2 and dot export under bf16, any change of the lane geometry (eight columns per lane), the C++ layer and CLI
(DESIGN.md 3.10.10).

``edge_attr=E`` (None by default: nothing new is constructed, allocated, launched or registered, the same bits as before)
puts edge features into the score of variant="v1", PyG's GATConv(edge_dim=de):

    e_ijk = lrelu(s_dst[i, k] + s_src[j, k] + E_p . att_edge[k], slope),   p the entry (i, j)

E is a numpy array [A.nnz() x de], 1 <= de <= ops.GAT_MAX_EDGE_DIM, converted to fp32; row p belongs to entry p of ``A`` as
given (row r of A lists the destinations that gather source r), and the caller supplies a row for every entry, self-loops
included -- there is no fill_value.  The edge term enters the score only, the message stays alpha Z[j].  The trained tensor
is ``layer.attn.att_edge`` [heads x de] per layer, gradient ``G_att_edge``: PyG's lin_edge(E_p)[head k] . att_edge[k] is
E_p . U[k] with U[k, c] = sum_d W_e[c, k dh + d] att_edge[k, d], and att_edge here IS U -- the same function class without
the redundant factorisation.  It starts seed-99 uniform like att, is a row of the fused Adam table with W's weight decay,
``edge_weights=`` takes one [heads x de] array per layer and ``model.edge_dim`` reads de (0 without the option).  The
entry points are those of csrc/gat_efeat.hip (mggcn_gat_*_efeat_f32 and their _drop twins): de loads and FMAs per (entry, head)
on the lane that owns the entry, nothing of nnz x heads stored, G_att_edge the fixed-order column sum of per-row shares
P_e [n x heads de].  The model holds E twice on the device, shared by all layers -- ``E_A`` in A's entry order for
backward_src and ``E_F`` = E[edge_permutation(A)] in A.transpose()'s for forward and backward_dst: 2 nnz de 4 bytes.  Both
dropouts (attention dropout draws the same Philox words as without E), skip=, norm=, label_input=, loss="bce", splits,
evaluate, predict, both Adam modes and model_selector's in-memory restore (att_edge included) compose.  Refused with
ValueError naming edge_attr before any device work: variant="v2" / "dot", agg_dtype="bf16", an array that is not
[A.nnz() x de] with de in range, a value that is not finite, a matrix whose indptr does not begin with 0 (row p of E is entry p
of A's indices array), edge_weights without edge_attr, save / load / save_best (no
version of the checkpoint file stores att_edge) and attention_weights / gat_layer.alpha (no export kernel has the edge
term).  Not built: edge features for "v2" and "dot" and in the message, dist_gat (it does not take the arguments), bf16
gathers or a bf16 E, the export and a checkpoint version, fill_value, reading E through a permutation instead of the second
copy, the C++ layer and CLI.

``fanout=k`` / ``edge_keep=q`` (None and 1.0 by default: no sampler, no buffer, no launch, no timer, the same bits as before)
train every epoch on a fresh sample of the edges, drawn on the device (edge_sample.py; csrc/edge_sample.hip): DropEdge with
``edge_keep``, an expected GraphSAGE fan-out with ``fanout``, or both -- destination i keeps each of its entries with
probability q_i = edge_keep * min(1, fanout / deg_i), self-loops always, by a Philox bit on (seed, epoch, i, j) that the
forward matrix and its transpose draw independently and still end up exact transposes of each other.  A training forward
(train_forward / train_step) draws the sample of ``sample_epoch``, runs every layer's sparse kernels, forward and backward,
over that one pair (one sample per epoch, shared by all layers), and moves ``sample_epoch`` on, exactly as dropout_epoch
moves; set_sampling(fanout=None, keep=1.0, seed=0, epoch=0) sets all of it (epoch=e replays training forward e) and
``sample_fanout``, ``sample_keep``, ``sample_seed``, ``sample_epoch`` read the state; ``sampler`` is the edge_sampler (None
when off).  A plain call, evaluate(), predict(), attention_weights(ctx, X) and correct_and_smooth.predict run on the full
graph with the bits they always had; model_selector defaults to clean=True, so its validation number is the full graph's.
All three variants, both dropouts (attention dropout is keyed by vertex numbers, not entry positions), skip=, norm=,
label_input=, loss="bce", splits, agg_dtype="bf16" and both Adam modes compose without special cases.  ``fanout`` is an
EXPECTED fan-out, not an exact one.  Checkpoints do not store the sampling state: save works, load leaves the state alone,
and a resumed run calls set_sampling(..., epoch=...) itself.  Refused with ValueError naming the argument before any device
work: a keep outside (0, 1], a fanout that is not None or an integer >= 1, sampling together with edge_attr= (the rows of E
are aligned to entry positions), and attention_weights(ctx) / gat_layer.alpha without X when the most recent forward was a
sampled one (its lse belongs to a pattern the export does not walk).  Not built: exact-k sampling, per-layer samples,
carrying or renormalising values, dist_gat (it does not take the arguments), edge features under sampling, the export of a
sampled forward, the state in checkpoints, the C++ layer and CLI.

Not covered: the halo and rounds schedules of dist_gcn, the C++ host layer and CLI.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np

from . import _lib, label_mask, ops
from .checkpoint import checkpoint_option
from .edge_sample import sampling_option
from .gcn import (DROPOUT_MAX_LAYERS, _check_agg_dtype, check_dropout, check_loss, check_norm, dropout_option, layer_norm,
                  layer_params, linear, model_base, param_owner, sigmoid_bce_loss, softmax_cross_entropy_loss)
from .matrix import context, csr_matrix, dn_matrix


def check_heads(sizes: Sequence[int], heads) -> List[int]:
    """heads per layer from ``heads=``: an int (every layer but the last has that many, the last 1) or one int per layer;
    ValueError when a width is not divisible by its heads or a limit of the kernels is exceeded.  No device work."""
    n_layers = len(sizes) - 1
    if n_layers < 1:
        raise ValueError("gat needs at least two sizes (one layer)")
    if isinstance(heads, (list, tuple)):
        per_layer = list(heads)
        if len(per_layer) != n_layers:
            raise ValueError(f"heads lists {len(per_layer)} layers, the model has {n_layers}")
    else:
        per_layer = [heads] * (n_layers - 1) + [1]
    for li, h in enumerate(per_layer):
        ops.check_gat_heads(h, int(sizes[li + 1]), f"gat layer {li}")
    return [int(h) for h in per_layer]


class gathered_images:
    """What the three attentions share for gat(agg_dtype="bf16"): the bf16 images their sparse kernels gather from and the
    conversion that makes them.  ``Z16`` is the image of the layer's Z buffer (all its columns: 1, 2 or 3 x out) and ``G16``
    that of the gradient G [rows x out]; both alias the model's two image buffers (``images``) when given, as G_Z aliases
    G_Z_buffer, and are None with agg_dtype="f32", where nothing is allocated, launched or registered.  The forward makes its
    image immediately before the forward kernel; the backward makes all of its images in one block ahead of backward_dst --
    the forward's again, because the layers above have overwritten the shared buffer since, and those of backward_src one
    kernel early (nothing in between writes Z or G) -- and only in the columns that are gathered."""

    agg_dtype = "f32"
    Z16 = G16 = None

    def _init_images(self, agg_dtype: str, rows_z: int, z_cols: int, rows_g: int, g_cols: int, images, device) -> None:
        self.agg_dtype = _check_agg_dtype(agg_dtype)
        if self.agg_dtype != "bf16":
            return
        import torch
        z_buffer, g_buffer = images if images is not None else (None, None)

        def image(buffer, rows, cols):
            if buffer is None:
                buffer = torch.empty(rows * cols, dtype=torch.bfloat16, device=device or "cuda")
            return ops.bf16_image(buffer.view(-1)[: rows * cols].view(rows, cols))
        self.Z16, self.G16 = image(z_buffer, rows_z, z_cols), image(g_buffer, rows_g, g_cols)

    def _convert(self, ctx: context, tag: str, *parts) -> None:
        """image[:, c0:c1] = bf16(M[:, c0:c1]), round to nearest even, for every (M, image, c0, c1) of ``parts``, under the
        timer ``<name><tag>_gat-convert`` ("0": the forward's, "1": the backward's)"""
        n = self.name
        ctx.record(n + tag + "_0_gat-convert", 0)
        for M, image, c0, c1 in parts:
            ops.convert_bf16(ctx, M.t[:, c0:c1], image.t[:, c0:c1])
        ctx.record(n + tag + "_1_gat-convert", 0)
        ctx.register_timer(n + tag + "_gat-convert", n + tag + "_0_gat-convert", n + tag + "_1_gat-convert")


def refuse_bf16_export(owner, what: str) -> None:
    """ValueError naming agg_dtype when ``owner`` (a gat model, a gatv2_layer or an attention_v2) is GATv2 with bf16 gathers:
    the export kernel would score the fp32 Zs against an lse taken over the rounded rows, which is not the coefficient the
    model trains with.  v1 exports unchanged: its scores and lse never see an image."""
    if getattr(owner, "agg_dtype", "f32") == "bf16" and getattr(owner, "variant", "v2") == "v2":
        raise ValueError(f'gat(variant="v2", agg_dtype="bf16") has no {what}: the export kernel reads the fp32 Zs, the '
                         'coefficients were trained on its bf16 image')


class attention(gathered_images, param_owner):
    """The attention of one layer: the parameter ``att`` [2 x out] (row 0 the destination vector, row 1 the source
    vector; seed-99 uniform like W), its gradient and Adam state, and what the backward pass needs of the forward --
    s_dst, s_src, lse [n x heads].  att is trained by Adam with the weight decay of W; the per-tensor step of
    gat(fused=False) is the fused kernel for every owner of an attention model, so both modes give the same bits.
    ``agg_dtype="bf16"``: forward and backward_dst gather Z, and backward_src gathers G, from bf16 images (gathered_images;
    ``images``: the model's two buffers); the scores, and so s_dst, s_src and lse, come from the fp32 Z."""

    params_table = (("att", "att", "G_att", "m", "v", True),)
    adam_fused = True
    m = v = None
    variant = "v1"

    def __init__(self, name: str, n_dst: int, n_src: int, out: int, heads: int, slope: float = ops.GAT_SLOPE, device=None,
                 agg_dtype: str = "f32", images=None):
        self._init_images(agg_dtype, n_src, out, n_dst, out, images, device)
        self.name, self.heads, self.slope = name, int(heads), float(slope)
        self.att, self.G_att = dn_matrix(2, out, device=device), dn_matrix(2, out, device=device)
        host = np.empty((2, out), dtype=np.float32)
        _lib.load().mggcn_init_uniform_host(host.ctypes.data, out, 2, -1.0)
        self.att.init(host)
        self.s_dst, self.lse, self.D, self.ds_dst = (dn_matrix(n_dst, heads, device=device) for _ in range(4))
        self.s_src, self.ds_src = dn_matrix(n_src, heads, device=device), dn_matrix(n_src, heads, device=device)

    def __call__(self, ctx: context, F: csr_matrix, Z: dn_matrix, out: dn_matrix, drop=None) -> None:
        """out = the attention-weighted gather of Z over F's rows (destinations and sources are the same vertices);
        ``drop``: attention dropout, the tuple of ops.gat_forward (None: the plain entry point)"""
        n = self.name
        ops.gat_scores(ctx, Z, self.att, self.s_dst, self.s_src, self.heads, n + "0_gat-scores")
        if self.Z16 is None:
            ops.gat_forward(ctx, F, Z, self.s_dst, self.s_src, out, self.lse, self.heads, self.slope, n + "0_gat-forward", drop)
            return
        self._convert(ctx, "0", (Z, self.Z16, 0, Z.m()))
        ops.gat_forward_bf16(ctx, F, self.Z16, self.s_dst, self.s_src, out, self.lse, self.heads, self.slope,
                             n + "0_gat-forward", drop)

    def backward(self, ctx: context, F: csr_matrix, F_T: csr_matrix, Z: dn_matrix, G: dn_matrix, out: dn_matrix,
                 G_Z: dn_matrix, drop=None) -> None:
        """G_Z = the gradient of Z and G_att, from G = the gradient of ``out``; ``drop``: what the forward was called with"""
        n = self.name
        if self.Z16 is None:
            ops.gat_backward_dst(ctx, F, Z, self.s_dst, self.s_src, self.lse, G, out, self.D, self.ds_dst, self.heads,
                                 self.slope, n + "1_gat-backward-dst", drop)
            ops.gat_backward_src(ctx, F_T, Z, self.s_dst, self.s_src, self.lse, self.D, G, self.att, self.ds_dst, self.ds_src,
                                 G_Z, self.heads, self.slope, n + "1_gat-backward-src", drop)
        else:
            # both images in one timed block: nothing between the two kernels writes Z or G
            self._convert(ctx, "1", (Z, self.Z16, 0, Z.m()), (G, self.G16, 0, G.m()))
            ops.gat_backward_dst_bf16(ctx, F, self.Z16, self.s_dst, self.s_src, self.lse, G, out, self.D, self.ds_dst,
                                      self.heads, self.slope, n + "1_gat-backward-dst", drop)
            ops.gat_backward_src_bf16(ctx, F_T, Z, self.s_dst, self.s_src, self.lse, self.D, self.G16, self.att, self.ds_dst,
                                      self.ds_src, G_Z, self.heads, self.slope, n + "1_gat-backward-src", drop)
        ops.gat_scores_backward(ctx, self.ds_dst, Z, self.ds_src, Z, self.G_att, self.heads, n + "1_gat-scores-backward")

    def alpha(self, ctx: context, F: csr_matrix, Z: dn_matrix, alpha: dn_matrix) -> None:
        """alpha [F.nnz() x heads] = the coefficients of the most recent forward over ``F``, from its s_dst, s_src and lse
        (Z is not read: the scores hold all of it that the coefficients need)"""
        ops.gat_alpha(ctx, F, self.s_dst, self.s_src, self.lse, alpha, self.heads, self.slope, self.name + "0_gat-alpha")

    def init(self, att) -> None:
        self.att.init(np.asarray(att, dtype=np.float32))


def check_edge_attr(edge_attr, edge_weights, variant: str, agg_dtype: str, n_layers: int):
    """option checking of edge_attr= / edge_weights=, before any device work and before the matrix is looked at: the fp32
    [entries x de] array (None without the option).  ValueError naming edge_attr for variant="v2" / "dot", agg_dtype="bf16",
    an array that is not [entries x de] with 1 <= de <= ops.GAT_MAX_EDGE_DIM, a value that is not finite, and for
    edge_weights without edge_attr or of another length than the layers."""
    if edge_attr is None:
        if edge_weights is not None:
            raise ValueError("edge_weights needs edge_attr: gat(..., edge_attr=E)")
        return None
    if variant != "v1":
        raise ValueError(f'gat(variant="{variant}") has no edge_attr: edge features are built for variant="v1" only (the '
                         "other scores need a vector of the layer's width per entry)")
    if agg_dtype != "f32":
        raise ValueError(f'gat(agg_dtype="{agg_dtype}") has no edge_attr: the edge-feature kernels gather fp32 rows only')
    E = np.asarray(edge_attr)
    if E.ndim != 2 or E.dtype.kind not in "fiu":
        raise ValueError(f"edge_attr must be a numeric [entries x de] array, got shape {E.shape} of {E.dtype}")
    if not 1 <= E.shape[1] <= ops.GAT_MAX_EDGE_DIM:
        raise ValueError(f"edge_attr supports 1 <= de <= {ops.GAT_MAX_EDGE_DIM} columns, got {E.shape[1]}")
    E = np.ascontiguousarray(E, dtype=np.float32)
    if not np.isfinite(E).all():
        raise ValueError("edge_attr holds a value that is not finite")
    if edge_weights is not None and len(edge_weights) != n_layers:
        raise ValueError(f"edge_weights (of edge_attr) lists {len(edge_weights)} layers, the model has {n_layers}")
    return E


def edge_permutation(A: csr_matrix) -> np.ndarray:
    """perm with E[perm] in the entry order of A.transpose() for E in A's: mggcn_csr_transpose_host emits a transposed row
    in increasing source-row order, which is the stable order of A's entries by column; the two entries of a duplicate
    pair (i, j) keep their order, a consistent bijection between the two copies.  int64, no device work.  Row p of E is entry
    p of A's indices array and the kernels take indptr's values as the rows of E, so A must start at entry 0: ValueError
    naming edge_attr for an indptr that does not begin with 0."""
    if int(A.indptr[0]) != 0:
        raise ValueError(f"edge_attr needs a matrix whose indptr begins with 0 (row p of E is entry p of A), got {int(A.indptr[0])}")
    return np.argsort(A.indices[:int(A.indptr[A.n()])], kind="stable")


def refuse_edge_attr(model, what: str) -> None:
    """ValueError naming edge_attr when ``model`` has edge features: ``what`` is a member such a model does not have yet
    (read with getattr: a model built without __init__ has no such attribute)"""
    if getattr(model, "edge_dim", 0):
        raise ValueError(f"gat(edge_attr=...) has no {what}")


class attention_efeat(gathered_images):
    """The attention of one gat(edge_attr=E) layer: ``attention``'s state and parameter with the edge term in the score,

        e_ijk = lrelu(s_dst[i, k] + s_src[j, k] + E_p . att_edge[k]),   p the entry (i, j),

    and one more trained tensor, ``att_edge`` [heads x de] (seed-99 uniform like att), with its gradient ``G_att_edge`` and
    Adam moments -- the second row of this owner's table, W's weight decay like att.  PyG's GATConv(edge_dim=de) scores
    an edge with lin_edge(E_p)[head k] . att_edge[k]; that product is E_p . U[k] with U[k, c] = sum_d W_e[c, k dh + d]
    att_edge[k, d], so att_edge here IS U: the same function class without the redundant factorisation.  ``E_F`` / ``E_A``
    are the model's two device copies of E ([entries x de]; E_F in the entry order of F, which forward and backward_dst
    walk, E_A in that of F^T, which backward_src walks) and ``P_e`` [n x heads de] the rows' shares of G_att_edge between
    backward_dst and the column sum; it aliases ``P_buffer`` (the model's, at the layer with the most heads).  The entry
    points are those of csrc/gat_efeat.hip (mggcn_gat_*_efeat_f32 and their _drop twins).  There is no export and no bf16 form.

    A parameter owner by its table and gcn.param_owner's own three methods, not by inheritance (as label_input is): the
    subclasses of param_owner are enumerated for the checkpoint's names per slot, and no version of the checkpoint file
    stores att_edge.  What it has of ``attention`` -- the constructor's buffers, init -- it takes by name."""

    params_table = attention.params_table + (("att_edge", "att_edge", "G_att_edge", "m_edge", "v_edge", True),)
    adam_fused = True
    step = 0
    m = v = m_edge = v_edge = None
    variant = "v1"
    adam_state, adam_tensors, adam_update = param_owner.adam_state, param_owner.adam_tensors, param_owner.adam_update
    init = attention.init

    def __init__(self, name: str, n_dst: int, n_src: int, out: int, heads: int, slope: float, E_F: dn_matrix, E_A: dn_matrix,
                 P_buffer=None, device=None):
        attention.__init__(self, name, n_dst, n_src, out, heads, slope, device)
        self.E_F, self.E_A, self.edge_dim = E_F, E_A, E_F.m()
        de = self.edge_dim
        self.att_edge, self.G_att_edge = dn_matrix(heads, de, device=device), dn_matrix(heads, de, device=device)
        host = np.empty((heads, de), dtype=np.float32)
        _lib.load().mggcn_init_uniform_host(host.ctypes.data, de, heads, -1.0)
        self.att_edge.init(host)
        self.P_e = dn_matrix(n_dst, heads * de, P_buffer) if P_buffer is not None else dn_matrix(n_dst, heads * de, device=device)
        self._G_row = dn_matrix(1, heads * de, self.G_att_edge.t)       # G_att_edge as the column sum's [1 x heads de]

    def __call__(self, ctx: context, F: csr_matrix, Z: dn_matrix, out: dn_matrix, drop=None) -> None:
        n = self.name
        ops.gat_scores(ctx, Z, self.att, self.s_dst, self.s_src, self.heads, n + "0_gat-scores")
        ops.gat_forward_efeat(ctx, F, Z, self.s_dst, self.s_src, out, self.lse, self.E_F, self.att_edge, self.heads, self.slope,
                              n + "0_gat-forward", drop)

    def backward(self, ctx: context, F: csr_matrix, F_T: csr_matrix, Z: dn_matrix, G: dn_matrix, out: dn_matrix,
                 G_Z: dn_matrix, drop=None) -> None:
        n = self.name
        ops.gat_backward_dst_efeat(ctx, F, Z, self.s_dst, self.s_src, self.lse, G, out, self.D, self.ds_dst, self.E_F,
                                   self.att_edge, self.P_e, self.heads, self.slope, n + "1_gat-backward-dst", drop)
        ops.gatv2_att_grad(ctx, self.P_e, self._G_row, n + "1_gat-edge-grad")
        ops.gat_backward_src_efeat(ctx, F_T, Z, self.s_dst, self.s_src, self.lse, self.D, G, self.att, self.ds_dst, self.ds_src,
                                   G_Z, self.E_A, self.att_edge, self.heads, self.slope, n + "1_gat-backward-src", drop)
        ops.gat_scores_backward(ctx, self.ds_dst, Z, self.ds_src, Z, self.G_att, self.heads, n + "1_gat-scores-backward")

    def alpha(self, ctx: context, F: csr_matrix, Z: dn_matrix, alpha: dn_matrix) -> None:
        raise ValueError("gat(edge_attr=...) has no export of the attention coefficients: there is no export kernel with "
                         "the edge term yet")

    def init_edge(self, att_edge) -> None:
        att_edge = np.asarray(att_edge, dtype=np.float32)
        if att_edge.shape != self.att_edge.shape():
            raise ValueError(f"edge_attr: edge_weights of layer {self.name} must be {self.heads} x {self.edge_dim} "
                             f"(heads x de), got {att_edge.shape}")
        self.att_edge.init(att_edge)


class attention_v2(attention):
    """The GATv2 attention of one layer: the parameter ``att`` [1 x out] (seed-99 uniform like W), its gradient and Adam
    state (``attention``'s: a row of the fused Adam table with W's weight decay), and what the backward pass needs of the
    forward -- lse and D [n x heads].  ``P`` [n x out] holds the rows' shares of G_att between backward_dst and att_grad; it
    aliases ``P_buffer`` (the model's, at its widest layer) when one is given.  __call__ and backward take the layer's
    Z2 = [Zs | Zd] and G_Z2 = [G_Zs | G_Zd] buffers of 2 out columns.  ``agg_dtype="bf16"``: forward and backward_dst gather
    Zs, and backward_src gathers Zd and G, from bf16 images -- ``Z16`` is the image of Z2, its halves made when they are
    gathered; Zd in the forward and Zs in backward_src are the rows' own and stay fp32.  The export is refused then."""

    variant = "v2"

    def __init__(self, name: str, n: int, out: int, heads: int, slope: float = ops.GAT_SLOPE, P_buffer=None, device=None,
                 agg_dtype: str = "f32", images=None):
        self._init_images(agg_dtype, n, 2 * out, n, out, images, device)
        self.name, self.heads, self.slope = name, int(heads), float(slope)
        self.att, self.G_att = dn_matrix(1, out, device=device), dn_matrix(1, out, device=device)
        host = np.empty((1, out), dtype=np.float32)
        _lib.load().mggcn_init_uniform_host(host.ctypes.data, out, 1, -1.0)
        self.att.init(host)
        self.lse, self.D = dn_matrix(n, heads, device=device), dn_matrix(n, heads, device=device)
        self.P = dn_matrix(n, out, P_buffer) if P_buffer is not None else dn_matrix(n, out, device=device)

    def __call__(self, ctx: context, F: csr_matrix, Z2: dn_matrix, out: dn_matrix, drop=None) -> None:
        """out = the attention-weighted gather of Zs over F's rows, scored against Zd"""
        assert drop is None, "GATv2 has no attention dropout"
        if self.Z16 is None:
            ops.gatv2_forward(ctx, F, Z2, Z2, self.att, out, self.lse, self.heads, self.slope, self.name + "0_gatv2-forward")
            return
        self._convert(ctx, "0", (Z2, self.Z16, 0, out.m()))                    # Zs
        ops.gatv2_forward_bf16(ctx, F, self.Z16, Z2, self.att, out, self.lse, self.heads, self.slope,
                               self.name + "0_gatv2-forward")

    def alpha(self, ctx: context, F: csr_matrix, Z2: dn_matrix, alpha: dn_matrix) -> None:
        """alpha [F.nnz() x heads] = the coefficients of the most recent forward over ``F``, from its Z2, att and lse;
        ValueError naming agg_dtype with bf16 gathers"""
        refuse_bf16_export(self, "export of the attention coefficients")
        ops.gatv2_alpha(ctx, F, Z2, Z2, self.att, self.lse, alpha, self.heads, self.slope, self.name + "0_gatv2-alpha")

    def backward(self, ctx: context, F: csr_matrix, F_T: csr_matrix, Z2: dn_matrix, G: dn_matrix, out: dn_matrix,
                 G_Z2: dn_matrix, drop=None) -> None:
        """G_Z2 = the gradient of Z2 (both halves) and G_att, from G = the gradient of ``out``"""
        assert drop is None, "GATv2 has no attention dropout"
        n = self.name
        if self.Z16 is None:
            ops.gatv2_backward_dst(ctx, F, Z2, Z2, self.att, self.lse, G, out, self.D, G_Z2, self.P, self.heads, self.slope,
                                   n + "1_gatv2-backward-dst")
            ops.gatv2_att_grad(ctx, self.P, self.G_att, n + "1_gatv2-att-grad")
            ops.gatv2_backward_src(ctx, F_T, Z2, Z2, self.att, self.lse, self.D, G, G_Z2, self.heads, self.slope,
                                   n + "1_gatv2-backward-src")
            return
        # Zs for backward_dst, Zd and G for backward_src, in one timed block: nothing between the kernels writes Z2 or G
        self._convert(ctx, "1", (Z2, self.Z16, 0, Z2.m()), (G, self.G16, 0, G.m()))
        ops.gatv2_backward_dst_bf16(ctx, F, self.Z16, Z2, self.att, self.lse, G, out, self.D, G_Z2, self.P, self.heads,
                                    self.slope, n + "1_gatv2-backward-dst")
        ops.gatv2_att_grad(ctx, self.P, self.G_att, n + "1_gatv2-att-grad")
        ops.gatv2_backward_src_bf16(ctx, F_T, Z2, self.Z16, self.att, self.lse, self.D, self.G16, G_Z2, self.heads, self.slope,
                                    n + "1_gatv2-backward-src")


SKIPS = (None, "add", "gate")


def check_skip(skip):
    """option checking of skip=, before any device work: None (no skip connection), "add" or "gate" """
    if skip not in SKIPS:
        raise ValueError(f"skip must be one of {SKIPS}, not {skip!r}")
    return skip


def check_skip_weights(skip, skip_weights, n_layers: int) -> None:
    """``skip_weights=`` of gat: per layer (W_r, b_r), or (W_r, b_r, w_gate) with skip="gate"; ValueError otherwise.  No
    device work."""
    if skip_weights is None:
        return
    if skip is None:
        raise ValueError("skip_weights needs skip=\"add\" or skip=\"gate\"")
    if len(skip_weights) != n_layers:
        raise ValueError(f"skip_weights lists {len(skip_weights)} layers, the model has {n_layers}")
    for li, w in enumerate(skip_weights):
        if len(w) not in ((2, 3) if skip == "gate" else (2,)):
            raise ValueError(f"skip_weights of layer {li}: skip=\"{skip}\" takes (W_r, b_r"
                             + (", w_gate)" if skip == "gate" else ")") + f", got {len(w)} tensors")


def refuse_skip(model, what: str) -> None:
    """ValueError naming the option when ``model`` has a skip connection or a layer norm: ``what`` is a member such a model
    does not have yet (read with getattr: a model built without __init__ has neither)"""
    for option in ("skip", "norm"):
        value = getattr(model, option, None)
        if value is not None:
            raise ValueError(f'gat({option}="{value}") has no {what}')


class gated_skip(param_owner):
    """The skip connection of one attention layer (gat(skip=...)): ``res_lin``, a linear r = H W_r + 1 b_r^T over the
    layer's own input -- always a linear, also where in == out (PyG's lin_skip) --, and the row kernels of
    csrc/gated_skip.hip that combine r with the attention output o: y = o + r ("add"), or y = g r + (1 - g) o with one
    g = sigmoid(sum_c (w[0] o + w[1] r + w[2] (o - r))) per row ("gate": TransformerConv(beta=True); no bias in the gate).
    "gate" holds the parameter ``w`` [3 x out] (seed-99 uniform like att), its gradient and Adam state -- a row of the
    fused Adam table with W's weight decay -- and the rows' ``gate`` [n], which the backward pass reads again.  ``r`` is
    kept per layer with the gate (its backward needs it) and lives in ``buffer`` (the model's, at its widest layer) without;
    ``G_r`` aliases ``buffer`` with the gate and is the layer's G_o without (one store).  The table is the gate's alone:
    res_lin is a linear of its own among the layer's owners."""

    params_table = (("gate", "w", "G_w", "m", "v", True),)
    adam_fused = True
    m = v = None

    def __init__(self, name: str, n: int, in_: int, out: int, mode: str, backward_out: bool = True, buffer=None, device=None):
        assert mode in ("add", "gate")
        self.name, self.mode = name, mode
        self.res_lin = linear(name, in_, out, backward_out, True)
        shared = dn_matrix(n, out, buffer) if buffer is not None else dn_matrix(n, out, device=device)
        self.w = self.G_w = self.gate = self.G_r = None
        if mode == "gate":
            self.r, self.G_r = dn_matrix(n, out, device=device), shared
            self.w, self.G_w = dn_matrix(3, out, device=device), dn_matrix(3, out, device=device)
            host = np.empty((3, out), dtype=np.float32)
            _lib.load().mggcn_init_uniform_host(host.ctypes.data, out, 3, -1.0)
            self.w.init(host)
            self.gate = dn_matrix(n, 1, device=device)
        else:
            self.r = shared

    def flags(self, leaky: bool) -> int:
        return (ops.GATED_SKIP_GATE if self.mode == "gate" else 0) | (ops.GATED_SKIP_LEAKY_RELU if leaky else 0)

    def __call__(self, ctx: context, H: dn_matrix, o: dn_matrix, y: dn_matrix, leaky: bool) -> None:
        """y = [leaky_relu](skip(o, H W_r + b_r))"""
        n = self.name
        self.res_lin(ctx, H, self.r)
        ctx.record(n + "0_0_skip", 0)
        ops.gated_skip(ctx, o, self.r, self.w, y, self.gate, self.flags(leaky))
        ctx.record(n + "0_1_skip", 0)
        ctx.register_timer(n + "0_skip", n + "0_0_skip", n + "0_1_skip")

    def backward(self, ctx: context, G: dn_matrix, act: Optional[dn_matrix], o: dn_matrix, G_o: dn_matrix) -> dn_matrix:
        """G_o = the gradient of o and, returned, the gradient of r (G_o itself without the gate), and G_w; ``act``: apply
        leaky_relu'(act) to G first.  G_o may be G or act."""
        n = self.name
        gated = self.mode == "gate"
        G_r = self.G_r if gated else G_o
        ctx.record(n + "1_0_skip", 0)
        ops.gated_skip_backward(ctx, G, act, o if gated else None, self.r if gated else None, self.w, self.gate, G_o, G_r,
                                self.G_w, self.flags(act is not None))
        ctx.record(n + "1_1_skip", 0)
        ctx.register_timer(n + "1_skip", n + "1_0_skip", n + "1_1_skip")
        return G_r

    def init(self, w) -> None:
        if self.mode != "gate":
            raise ValueError('gat(skip="add") has no gate parameter: skip_weights= takes (W_r, b_r) per layer')
        self.w.init(np.asarray(w, dtype=np.float32))


def check_label_input(rate, loss: str, n_classes: int) -> int:
    """option checking of label_input=, before any device work: the threshold floor(rate * 2^32) of a rate in [0, 1);
    ValueError naming label_input for another rate and, with a rate above 0, for loss="bce" (a row has one label to feed)
    and for more classes than the kernels take"""
    threshold = label_mask.threshold(rate)
    if rate > 0.0:
        if loss == "bce":
            raise ValueError('label_input needs one class per vertex: loss="bce" (multi-label targets) has no label input')
        if n_classes > ops.LABEL_INPUT_MAX_CLASSES:
            raise ValueError(f"label_input supports at most {ops.LABEL_INPUT_MAX_CLASSES} classes, the model has {n_classes}")
    return threshold


def refuse_label_input(model, what: str) -> None:
    """ValueError naming the option when ``model`` feeds labels: ``what`` is a member such a model does not have yet (read
    with getattr: a model built without __init__ has neither attribute)"""
    if getattr(model, "label", None) is not None or getattr(model, "label_input_p", 0.0) > 0.0:
        raise ValueError(f"gat(label_input={getattr(model, 'label_input_p', 0.0)}) has no {what}")


def label_lists(S, Y, train_set: int, n_classes: int):
    """(rows, cls, cls_ptr) of the label-input kernels from host arrays of n sets and n labels: the rows of ``train_set``
    sorted by (class, row), their classes, and the segment of each class -- int32 arrays of T, T and n_classes + 1.
    ValueError naming label_input for a label outside [0, n_classes) on a training row."""
    s, y = np.asarray(S).reshape(-1), np.asarray(Y).reshape(-1)
    if s.size != y.size:
        raise ValueError(f"label_input: {y.size} labels for {s.size} vertices")
    train = np.flatnonzero(s == train_set)
    yt = y[train].astype(np.int64)
    bad = np.flatnonzero((yt < 0) | (yt >= n_classes))
    if bad.size:
        raise ValueError(f"label_input: training row {int(train[bad[0]])} has label {int(yt[bad[0]])}, outside [0, {n_classes})")
    order = np.argsort(yt, kind="stable")               # ``train`` ascends, so a stable sort by class is (class, row)
    cls_ptr = np.zeros(n_classes + 1, dtype=np.int64)
    np.cumsum(np.bincount(yt, minlength=n_classes), out=cls_ptr[1:])
    return train[order].astype(np.int32), yt[order].astype(np.int32), cls_ptr.astype(np.int32)


class label_input:
    """The masked label input of layer 0 (gat(label_input=rate); the label trick of UniMP): the trained table ``E``
    [classes x width of layer 0's Z] (seed-99 uniform like att), its gradient and Adam state -- a row of the fused Adam
    table with W's weight decay --, the device lists of the training rows the two kernels of csrc/label_input.hip walk
    (``rows``, ``cls``, ``cls_ptr``: set_lists, None before) and ``S_e``, the sets the loss sees in a training forward
    (fed rows in the "other" slot).  ``call`` is set by the model before every forward and read again by backward():
    (threshold, feed_all, seed, epoch, write S_e).

    A parameter owner by its table and gcn.param_owner's own three methods, not by inheritance: it sits in the MODEL's
    slot of layer 0 alone, not in a slot every layer of a kind has, which is what the subclasses of param_owner are
    enumerated for (the checkpoint's names per layer)."""

    params_table = (("label", "E", "G_E", "m", "v", True),)
    adam_fused = True
    step = 0
    m = v = None
    adam_state, adam_tensors, adam_update = param_owner.adam_state, param_owner.adam_tensors, param_owner.adam_update

    def __init__(self, name: str, n_classes: int, width: int, device=None):
        self.name = name
        self.E, self.G_E = dn_matrix(n_classes, width, device=device), dn_matrix(n_classes, width, device=device)
        host = np.empty((n_classes, width), dtype=np.float32)
        _lib.load().mggcn_init_uniform_host(host.ctypes.data, width, n_classes, -1.0)
        self.E.init(host)
        self.rows = self.cls = self.cls_ptr = self.S_e = None
        self.train_set = 0
        self.call = None

    def set_lists(self, rows, cls, cls_ptr, S, train_set: int) -> None:
        """the host lists of label_lists and the host sets (n x 1): uploaded once, S_e starts as a copy of the sets"""
        device = self.E.t.device
        self.rows, self.cls, self.cls_ptr = (dn_matrix.from_numpy(a.reshape(-1, 1), device=device) for a in (rows, cls, cls_ptr))
        self.S_e = dn_matrix.from_numpy(np.ascontiguousarray(S, dtype=np.int32).reshape(-1, 1), device=device)
        self.train_set = int(train_set)

    def __call__(self, ctx: context, Z: dn_matrix, row0: int = 0) -> None:
        """Z[fed rows] += E[their class]; a training forward also rewrites the training rows of S_e"""
        n = self.name
        threshold, feed_all, seed, epoch, write = self.call
        ctx.record(n + "0_0_label-input", 0)
        ops.label_input_forward(ctx, self.rows, self.cls, self.E, Z, threshold, feed_all, seed, epoch, row0, self.train_set,
                                ops.LABEL_INPUT_FED_SET, self.S_e if write else None)
        ctx.record(n + "0_1_label-input", 0)
        ctx.register_timer(n + "0_label-input", n + "0_0_label-input", n + "0_1_label-input")

    def backward(self, ctx: context, G_Z: dn_matrix, row0: int = 0) -> None:
        """G_E from the gradient of Z, with the mask of the forward"""
        n = self.name
        threshold, feed_all, seed, epoch, _ = self.call
        ctx.record(n + "1_0_label-input", 0)
        ops.label_input_backward(ctx, self.rows, self.cls, self.cls_ptr, G_Z, self.G_E, threshold, feed_all, seed, epoch, row0)
        ctx.record(n + "1_1_label-input", 0)
        ctx.register_timer(n + "1_label-input", n + "1_0_label-input", n + "1_1_label-input")

    def init(self, E) -> None:
        E = np.asarray(E, dtype=np.float32)
        if E.shape != self.E.shape():
            raise ValueError(f"label_input: label_weights must be {self.E.n()} x {self.E.m()}, got {E.shape}")
        self.E.init(E)


_label_input_owner = label_input         # gat's constructor has an argument of that name


def refuse_sampled_export(layer, what: str) -> None:
    """ValueError naming the sampling when ``layer``'s most recent forward ran on an edge sample: its lse belongs to a pattern
    the export does not walk.  A plain forward (attention_weights(ctx, X)) clears it."""
    if getattr(layer, "sample", None) is not None:
        raise ValueError(f"{what}: the most recent forward was a sampled training forward (set_sampling / fanout / edge_keep); "
                         "its lse belongs to the sample, not to the pattern the export walks -- pass X: attention_weights(ctx, X)")


class gat_layer(layer_params):
    """One GAT layer: a ``linear`` (Z = H W + 1 b^T), an ``attention`` over (F, F^T) and the activation.  Z, the
    aggregated ``out`` (before the activation: the backward pass needs it) and the activated output are kept per layer;
    G_Z aliases the model-wide buffer.  ``backward_out=False`` (the first layer) skips the GEMM that only produces the
    gradient of the layer's input.  ``skip`` ("add" | "gate") puts a ``gated_skip`` after the aggregation and ``norm``
    ("layer") a gcn.layer_norm after that, in every layer that has an activation: attention -> skip -> norm -> activation,
    the activation fused into whichever of the two runs last.  The attributes are ``res_lin`` (the skip's linear), ``gate``
    (the skip itself where it has the gate parameter) and ``norm``, each None where the layer has none."""

    res_lin = gate = norm = None
    label = None                # the model's label_input, in layer 0 of gat(label_input=rate) only
    sample = None               # (F, F_T) of this forward where the model drew an edge sample (edge_sample.py); None: the full graph

    def _matrices(self):
        """(F, F_T) the most recent forward walked and its backward walks: the model's sample of the epoch, or the full graph"""
        return self.sample if self.sample is not None else (self.F, self.F_T)

    def __init__(self, name: str, F: csr_matrix, F_T: csr_matrix, in_: int, out: int, heads: int, activation: bool,
                 slope: float = ops.GAT_SLOPE, backward_out: bool = True, G_Z_buffer=None, skip=None, norm=None,
                 skip_buffer=None, agg_dtype: str = "f32", images=None, edge=None):
        n = F.n()
        assert F.n() == F.m() == F_T.n() == F_T.m(), "the single-GPU layer takes a square matrix"
        # ``edge``: (E_F, E_A, P_buffer) of gat(edge_attr=...), the model's; None builds the attention as it always was
        attn = (attention(name, n, n, out, heads, slope, agg_dtype=agg_dtype, images=images) if edge is None else
                attention_efeat(name, n, n, out, heads, slope, *edge))
        # the linear's own fused kernels in every mode: gat(fused=...) only picks how Adam is launched
        self._setup(name, F, F_T, linear(name, in_, out, backward_out, True), attn, n, in_,
                    out, activation, G_Z_buffer, skip=skip, norm=norm, skip_buffer=skip_buffer)

    def _setup(self, name: str, F: csr_matrix, F_T: csr_matrix, lin, attn, rows: int, in_: int, out: int, activation: bool,
               G_Z_buffer=None, device=None, row0: int = 0, z_width: Optional[int] = None, skip=None, norm=None,
               skip_buffer=None) -> None:
        """everything a layer holds besides building ``lin`` and ``attn``: its buffers over ``rows`` rows and the per-forward
        state (the row-partitioned layer, dist_gat.dist_gat_layer, calls it with its rank's pieces); ``z_width``: the columns
        of Z and G_Z where they are not ``out`` (gatv2_layer: 2 out); ``skip`` / ``norm`` / ``skip_buffer``: the gated_skip
        (its model-wide buffer) and the layer norm, None for a layer without"""
        self.name, self.F, self.F_T, self.activation = name, F, F_T, bool(activation)
        self.lin, self.attn = lin, attn
        zw = out if z_width is None else int(z_width)
        self.Z, self.out = dn_matrix(rows, zw, device=device), dn_matrix(rows, out, device=device)
        self.skip = gated_skip(name, rows, in_, out, skip, lin.backward_out, skip_buffer, device) if skip is not None else None
        self.res_lin = self.skip.res_lin if self.skip is not None else None
        self.gate = self.skip if skip == "gate" else None
        self.norm = layer_norm(name, rows, out, True, device, adam_fused=True) if norm == "layer" and activation else None
        # the layer's output y: the last layer has no activation and returns ``out`` itself, unless a skip writes a y
        self.act = dn_matrix(rows, out, device=device) if activation or self.skip is not None else self.out
        self.G_Z = dn_matrix(rows, zw, G_Z_buffer) if G_Z_buffer is not None else dn_matrix(rows, zw, device=device)
        self.G_out = dn_matrix(rows, in_, device=device) if lin.backward_out else None
        self.H: Optional[dn_matrix] = None
        # set by the model before every forward and read again by backward(): ``dropout`` -- (threshold, scale, seed, stream)
        # of ops.dropout_raw for my input and the gradient I return; ``attn_dropout`` -- the tuple of ops.gat_forward
        self.dropout = None
        self.attn_dropout = None
        self.row0 = int(row0)               # the global index of my first row (dist_gat.dist_gat_layer: the rank's)

    def _drop(self, ctx: context, M: dn_matrix, tag: str) -> None:
        """M = dropout(M) in place with this forward's mask: H on the way up ("0"), G_out on the way down ("1")"""
        n = self.name
        threshold, scale, seed, stream = self.dropout
        ctx.record(n + tag + "_0_dropout", 0)
        ops.dropout_raw(ctx, M, M, threshold, scale, seed, stream, self.row0)
        ctx.record(n + tag + "_1_dropout", 0)
        ctx.register_timer(n + tag + "_dropout", n + tag + "_0_dropout", n + tag + "_1_dropout")

    def __call__(self, ctx: context, H: dn_matrix) -> dn_matrix:
        n = self.name
        if self.dropout is not None:
            # In place: H is the ``act`` buffer of the layer below, which no backward reads as a value -- that layer's own
            # backward takes its signs and its D = G . out from its ``out``, a separate buffer wherever there is an
            # activation (every layer that has a layer above), and overwrites ``act`` with T.  My G_W GEMM wants the
            # dropped H, which is what stays here.
            self._drop(ctx, H, "0")
        self.H = H
        self.lin(ctx, H, self.Z)
        if self.label is not None:                           # [H | M onehot(y)] [W ; E] = H W + M E[y]: the skip sees H only
            self.label(ctx, self.Z, self.row0)
        self.attn(ctx, self._matrices()[0], self.Z, self.out, self.attn_dropout)
        if self.skip is not None or self.norm is not None:
            # attention -> skip -> norm -> activation; ``out`` stays as the attention wrote it (its backward reads it), y
            # goes to ``act``, the norm runs in place there, and the activation rides in whichever of the two runs last
            if self.skip is not None:
                self.skip(ctx, H, self.out, self.act, self.activation and self.norm is None)
            if self.norm is not None:
                self.norm(ctx, self.act if self.skip is not None else self.out, True, self.act)
        elif self.activation:
            ctx.record(n + "0_0_activation", 0)
            ops.leaky_relu_forward(ctx, self.out, self.act)
            ctx.record(n + "0_1_activation", 0)
            ctx.register_timer(n + "0_activation", n + "0_0_activation", n + "0_1_activation")
        return self.act

    def backward(self, ctx: context, G: dn_matrix) -> Optional[dn_matrix]:
        n = self.name
        T, G_r = G, None
        if self.skip is not None or self.norm is not None:
            # The sign source of the fused activation is the activated output ``act``, as in gcn and the layer norm.  The
            # layer above may have dropped that buffer in place: a kept element keeps its sign (the scale is positive), and a
            # dropped one is 0 here and carries a zero gradient (the layer above dropped its G_out with the same mask), so
            # either branch of leaky_relu' gives 0.  Every gradient lands in ``act``, which the layer above has finished with.
            sign = self.act if self.activation else None
            if self.norm is not None:
                self.norm.backward(ctx, G, sign, self.act)
                T, sign = self.act, None
            if self.skip is not None:
                G_r = self.skip.backward(ctx, T, sign, self.out, self.act)
                T = self.act
        elif self.activation:
            # the sign source is the aggregated output itself; T lands in the activated output's buffer, which the layer
            # above has finished with (its G_W GEMM read it earlier on this stream)
            ctx.record(n + "1_0_activation", 0)
            ops.leaky_relu_backward(ctx, self.out, G, self.act)
            ctx.record(n + "1_1_activation", 0)
            ctx.register_timer(n + "1_activation", n + "1_0_activation", n + "1_1_activation")
            T = self.act
        self.attn.backward(ctx, *self._matrices(), self.Z, T, self.out, self.G_Z, self.attn_dropout)
        if self.label is not None:
            self.label.backward(ctx, self.G_Z, self.row0)
        self.lin.setX(self.H)
        self.lin.backward(ctx, self.G_Z, self.G_out)
        if G_r is not None:                                  # the skip branch adds its share of the input's gradient
            self.res_lin.setX(self.H)
            self.res_lin.backward(ctx, G_r, self.G_out, False)
        if self.dropout is not None and self.G_out is not None:
            self._drop(ctx, self.G_out, "1")
        return self.G_out

    def alpha(self, ctx: context, out: Optional[dn_matrix] = None) -> dn_matrix:
        """The attention coefficients of this layer's most recent forward: [F.nnz() x heads], row p for entry p of F's
        indices array (row i of F lists the sources of destination i), column k for head k.  ``out``: where to put them
        (None allocates).  After a training forward with attention dropout these are the normalised coefficients BEFORE
        the dropout factor.  ValueError when no forward has run, or for an ``out`` of another shape, and, naming edge_attr and
        before anything else, on a layer of gat(edge_attr=...)."""
        refuse_edge_attr(getattr(self, "attn", None), f"export of the attention coefficients (gat layer {self.name}): there is no export "
                                    "kernel with the edge term yet")
        refuse_sampled_export(self, f"gat layer {self.name}: alpha")
        if self.H is None:
            raise ValueError(f"gat layer {self.name}: no forward has run, there are no attention coefficients yet")
        shape = (self.F.nnz(), self.attn.heads)
        if out is None:
            out = dn_matrix(*shape, device=self.Z.t.device)
        elif out.shape() != shape:
            raise ValueError(f"gat layer {self.name}: out must be {shape[0]} x {shape[1]} (entries x heads), got {out.shape()}")
        self.attn.alpha(ctx, self.F, self.Z, out)
        return out

    def linears(self):
        return [self.lin]

    def owners(self):
        pairs = (("", self.lin), ("", self.attn), ("res_", self.res_lin), ("", self.gate), ("", self.norm), ("", self.label))
        return [(prefix, o) for prefix, o in pairs if o is not None]

    def att(self): return self.attn.att
    def Gatt(self): return self.attn.G_att


class gatv2_layer(gat_layer):
    """One GATv2 layer: ONE ``linear`` of 2 out columns (Z2 = H W + 1 b^T = [Zs | Zd], the bias inside both halves), an
    ``attention_v2`` over (F, F^T) and the activation.  ``Z`` is Z2 and ``G_Z`` its gradient [G_Zs | G_Zd] (aliasing the
    model-wide buffer), so the forward is one GEMM and the backward the linear's fused weight-gradient and input-gradient
    GEMMs over 2 out columns; everything else is gat_layer's, word for word."""

    def __init__(self, name: str, F: csr_matrix, F_T: csr_matrix, in_: int, out: int, heads: int, activation: bool,
                 slope: float = ops.GAT_SLOPE, backward_out: bool = True, G_Z_buffer=None, P_buffer=None, skip=None,
                 norm=None, skip_buffer=None, agg_dtype: str = "f32", images=None):
        n = F.n()
        assert F.n() == F.m() == F_T.n() == F_T.m(), "the single-GPU layer takes a square matrix"
        self._setup(name, F, F_T, linear(name, in_, 2 * out, backward_out, True),
                    attention_v2(name, n, out, heads, slope, P_buffer, agg_dtype=agg_dtype, images=images), n, in_, out,
                    activation, G_Z_buffer, z_width=2 * out, skip=skip, norm=norm, skip_buffer=skip_buffer)

    def alpha(self, ctx: context, out: Optional[dn_matrix] = None) -> dn_matrix:
        """gat_layer.alpha; ValueError naming agg_dtype, before anything else, with bf16 gathers"""
        refuse_bf16_export(self.attn, f"export of the attention coefficients (gat layer {self.name})")
        return gat_layer.alpha(self, ctx, out)


class attention_dot(gathered_images, param_owner):
    """The dot-product attention of one layer: no parameter, only what the backward pass needs of the forward -- lse and D
    [n x heads] --, the head count and the scale c = fp32(1 / sqrt(dh)).  __call__ and backward take the layer's
    Z3 = [Zq | Zk | Zv] and G_Z3 = [G_Zq | G_Zk | G_Zv] buffers of 3 out columns.  Its table is empty: it is a row of nobody's Adam table.
    ``agg_dtype="bf16"``: forward and backward_dst gather Zk and Zv, and backward_src gathers Zq and G, from bf16 images --
    ``Z16`` is the image of Z3, its thirds made when they are gathered; Zq in the forward and Zk, Zv in backward_src are the
    rows' own and stay fp32."""

    att = G_att = m = v = None          # what gat_layer.att() / Gatt() return for such a layer
    variant = "dot"

    def __init__(self, name: str, n: int, out: int, heads: int, device=None, agg_dtype: str = "f32", images=None):
        self._init_images(agg_dtype, n, 3 * out, n, out, images, device)
        self.name, self.heads = name, int(heads)
        self.scale = ops.gatdot_scale(out // self.heads)
        self.lse, self.D = dn_matrix(n, heads, device=device), dn_matrix(n, heads, device=device)

    def __call__(self, ctx: context, F: csr_matrix, Z3: dn_matrix, out: dn_matrix, drop=None) -> None:
        """out = the attention-weighted gather of Zv over F's rows, Zq scored against Zk"""
        assert drop is None, "dot-product attention has no attention dropout"
        if self.Z16 is None:
            ops.gatdot_forward(ctx, F, Z3, Z3, Z3, out, self.lse, self.heads, self.scale, self.name + "0_gatdot-forward")
            return
        self._convert(ctx, "0", (Z3, self.Z16, out.m(), 3 * out.m()))          # [Zk | Zv]
        ops.gatdot_forward_bf16(ctx, F, Z3, self.Z16, self.Z16, out, self.lse, self.heads, self.scale,
                                self.name + "0_gatdot-forward")

    def backward(self, ctx: context, F: csr_matrix, F_T: csr_matrix, Z3: dn_matrix, G: dn_matrix, out: dn_matrix,
                 G_Z3: dn_matrix, drop=None) -> None:
        """G_Z3 = the gradient of Z3 (all three thirds), from G = the gradient of ``out``"""
        assert drop is None, "dot-product attention has no attention dropout"
        n = self.name
        if self.Z16 is None:
            ops.gatdot_backward_dst(ctx, F, Z3, Z3, Z3, self.lse, G, out, self.D, G_Z3, self.heads, self.scale,
                                    n + "1_gatdot-backward-dst")
            ops.gatdot_backward_src(ctx, F_T, Z3, Z3, Z3, self.lse, self.D, G, G_Z3, G_Z3, self.heads, self.scale,
                                    n + "1_gatdot-backward-src")
            return
        # Zk, Zv for backward_dst, Zq and G for backward_src, in one timed block: nothing between the kernels writes Z3 or G
        self._convert(ctx, "1", (Z3, self.Z16, 0, Z3.m()), (G, self.G16, 0, G.m()))
        ops.gatdot_backward_dst_bf16(ctx, F, Z3, self.Z16, self.Z16, self.lse, G, out, self.D, G_Z3, self.heads, self.scale,
                                     n + "1_gatdot-backward-dst")
        ops.gatdot_backward_src_bf16(ctx, F_T, self.Z16, Z3, Z3, self.lse, self.D, self.G16, G_Z3, G_Z3, self.heads, self.scale,
                                     n + "1_gatdot-backward-src")

    def alpha(self, ctx, F, Z3, alpha) -> None:
        raise ValueError('gat(variant="dot") has no export of the attention coefficients')

    def init(self, att) -> None:
        raise ValueError('gat(variant="dot") has no attention parameter: weights= takes (W, b) per layer')


class gatdot_layer(gat_layer):
    """One dot-product attention layer: ONE ``linear`` of 3 out columns (Z3 = H W + 1 b^T = [Zq | Zk | Zv], the bias inside
    all three thirds), an ``attention_dot`` over (F, F^T) and the activation.  ``Z`` is Z3 and ``G_Z`` its gradient
    [G_Zq | G_Zk | G_Zv] (aliasing the model-wide buffer); the layer's parameters are the linear's alone."""

    def __init__(self, name: str, F: csr_matrix, F_T: csr_matrix, in_: int, out: int, heads: int, activation: bool,
                 backward_out: bool = True, G_Z_buffer=None, skip=None, norm=None, skip_buffer=None, agg_dtype: str = "f32",
                 images=None):
        n = F.n()
        assert F.n() == F.m() == F_T.n() == F_T.m(), "the single-GPU layer takes a square matrix"
        self._setup(name, F, F_T, linear(name, in_, 3 * out, backward_out, True),
                    attention_dot(name, n, out, heads, agg_dtype=agg_dtype, images=images), n, in_,
                    out, activation, G_Z_buffer, z_width=3 * out, skip=skip, norm=norm, skip_buffer=skip_buffer)

    def alpha(self, ctx: context, out: Optional[dn_matrix] = None) -> dn_matrix:
        raise ValueError(f'gat layer {self.name}: gat(variant="dot") has no export of the attention coefficients')


VARIANTS = ("v1", "v2", "dot")
DOT_MAX_ELEMENTS = 1 << 31          # csrc/gemm.hip: the output of one GEMM, rows x 3 out, stays below this


def check_variant(variant, attn_dropout: float = 0.0) -> str:
    """``variant=`` of gat: "v1", "v2" or "dot"; ValueError for anything else and for GATv2 or dot-product attention with
    attention dropout (the _drop twins of their three sparse kernels do not exist).  No device work."""
    if variant not in VARIANTS:
        raise ValueError(f"gat variant must be one of {VARIANTS}, got {variant!r}")
    if variant != "v1" and attn_dropout > 0.0:
        raise ValueError(f"gat(variant=\"{variant}\") has no attention dropout: attn_dropout must be 0")
    return variant


def check_single_gpu_variant(variant) -> None:
    """what dist_gat.dist_gat refuses after check_variant: ValueError for "dot", which has no row-partitioned form yet.  No
    device work, no collective."""
    if variant == "dot":
        raise ValueError('dist_gat has no variant="dot": dot-product attention is single-GPU only (gat(variant="dot"))')


def refuse_dot(model, what: str) -> None:
    """ValueError when ``model`` is a dot-product attention model: ``what`` is a member it does not have yet"""
    if getattr(model, "variant", "v1") == "dot":
        raise ValueError(f'gat(variant="dot") has no {what}')


def refuse_checkpoint(model, member: str) -> None:
    """what save, load and _write_checkpoint of gat refuse, before anything is read, written or created: dot-product
    attention, the skip options, the label input and the edge features, which no version of the checkpoint file stores"""
    refuse_dot(model, f"{member} has no version for this variant yet")
    refuse_skip(model, f"{member} has no version that stores this option yet")
    refuse_label_input(model, f"{member} has no version that stores the label table E yet")
    refuse_edge_attr(model, f"{member} has no version that stores att_edge yet")


class attention_model:
    """What only the attention models have, gat and dist_gat.dist_gat alike (both list it first among their bases): the
    two dropouts and the export of the coefficients.  It reads ``variant``, ``heads``, ``layers_`` (their F, H and alpha),
    ``attn_dropout_p`` / ``_attn_dropout_params`` and the state of gcn.dropout_option; _mask_origin() is the hook of the row
    partition."""

    def set_dropout(self, p: float, seed: int = 0, epoch: int = 0, attn: Optional[float] = None) -> None:
        """p: the drop probability of the layer inputs, attn: that of the attention coefficients (None keeps the current
        one), both in [0, 1) and 0 = off; seed: 64 bits, shared by both; epoch: the number the next training forward gets
        (set_dropout(p, seed, epoch=e) replays training forward e).  ValueError before any device work, and before
        anything is stored."""
        attn = self.attn_dropout_p if attn is None else attn
        attn_params = check_dropout(attn, self._dropout_layers)
        check_variant(self.variant, float(attn))
        dropout_option.set_dropout(self, p, seed, epoch)
        self._attn_dropout_params, self.attn_dropout_p = attn_params, float(attn)

    def _mask_origin(self):
        """(dst0, src0): the global vertex numbers of the first destination and the first source of this model's forward
        matrix, which the attention mask is drawn on"""
        return 0, 0

    def _arm_dropout(self, training: bool) -> None:
        """hands every layer its two calls of this forward (None: the plain path); a training forward with either
        probability above 0 takes the current epoch number and moves it on.  Layer l uses stream epoch * 64 + l for both."""
        feat = bool(training) and self.dropout_p > 0.0
        attn = bool(training) and self.attn_dropout_p > 0.0
        origin = self._mask_origin()
        for li, layer in enumerate(self.layers_):
            stream = (self.dropout_epoch * DROPOUT_MAX_LAYERS + li) & 0xFFFFFFFF
            layer.dropout = (*self._dropout_params, self.dropout_seed, stream) if feat and li > 0 else None
            layer.attn_dropout = (*self._attn_dropout_params, self.dropout_seed, stream, *origin) if attn else None
        if feat or attn:
            self.dropout_epoch += 1

    def _alpha_requests(self, layers, out) -> List[int]:
        """the layer indices ``layers=`` names, after every check attention_weights can make without the device"""
        n_layers = len(self.layers_)
        which = list(range(n_layers)) if layers is None else [int(li) for li in layers]
        for li in which:
            if not 0 <= li < n_layers:
                raise ValueError(f"attention_weights: layer {li} is out of range, the model has {n_layers} layers")
        if out is not None:
            if len(out) != len(which):
                raise ValueError(f"attention_weights: out lists {len(out)} matrices for {len(which)} layers")
            for li, o in zip(which, out):
                want = (self.layers_[li].F.nnz(), self.heads[li])
                if o.shape() != want:
                    raise ValueError(f"attention_weights: out of layer {li} must be {want[0]} x {want[1]}, got {o.shape()}")
        return which

    def attention_weights(self, ctx, X=None, layers=None, out=None) -> List[dn_matrix]:
        """The attention coefficients alpha_ijk per layer (PyG's return_attention_weights): a list with one [nnz x heads]
        dn_matrix per requested layer, whose row p belongs to entry p of attention_pattern()'s ``indices`` and whose
        column k to head k.  With ``X`` a plain forward runs first (self(ctx, X), the forward that never drops); without,
        the export is taken from the state the most recent forward left behind -- ValueError when there was none.  After
        a training forward with attention dropout that state is the normalised coefficient BEFORE the dropout factor q:
        the softmax runs over all entries there too, so the export is what a plain forward of the same weights and
        inputs gives, not alpha q.  ``layers``: None for all, or layer indices, returned in the order given; ``out``: one
        dn_matrix per requested layer to write into (None allocates).  ValueError before any device work for an index
        out of range and for an ``out`` of the wrong length or shape.

        On the row partition ``ctx`` and ``X`` are the rank's dist_context and dist_row_dn_matrix, every rank calls with the
        same arguments and gets the entries of ITS rows (dist_gat.dist_gat); the export itself runs no collective.

        The values are exp(e_ijk - lse[i, k]) as the backward kernels evaluate it (mggcn_gat_alpha_f32 /
        mggcn_gatv2_alpha_f32): the coefficients the model trains with, the same bits on every call.  This is the one place
        where something of nnz x heads is stored: the Reddit-shaped graph (114.8 M entries) at 4 heads needs 1.84 GB per
        layer.  Nothing is allocated or launched unless this method (or gat_layer.alpha) is called."""
        which = self._alpha_requests(layers, out)
        if X is None:
            for li in which:
                refuse_sampled_export(self.layers_[li], "attention_weights")
        if X is not None:
            self(ctx, X)
        elif any(self.layers_[li].H is None for li in which):
            raise ValueError("attention_weights: no forward has run, there are no attention coefficients yet (pass X)")
        return [self.layers_[li].alpha(ctx, None if out is None else out[i]) for i, li in enumerate(which)]


class gat(attention_model, sampling_option, model_base):
    """A stack of GAT layers with the loss layers, splits and Adam of ``gcn``.

    gat(A, sizes, heads=4, attn_slope=0.2, loss="softmax", fused=True, weights=None, dropout=0.0, attn_dropout=0.0,
    variant="v1", skip=None, norm=None, skip_weights=None, label_input=0.0, label_weights=None,
    agg_dtype="f32", edge_attr=None, edge_weights=None, fanout=None, edge_keep=1.0):
    ``fanout`` / ``edge_keep``: per-epoch edge sampling, set_sampling's fanout and keep -- see the module docstring and
    edge_sample.sampling_option; ValueError naming the argument for what it refuses.
    ``edge_attr`` / ``edge_weights``: edge features in the score of variant="v1", a numpy [A.nnz() x de] array in A's entry
    order and one [heads x de] att_edge per layer -- see the module docstring; ValueError naming edge_attr for what it refuses.
    ``A`` as ``gcn`` takes it (the layers aggregate over the pattern of A.transpose(); A's values are neither used nor changed); ``heads``: an int
    (every layer but the last, which has 1) or one int per layer; ``weights``: per layer (W, b) or (W, b, att);
    ``variant``: "v1" (this model as it always was) or "v2" (GATv2, see the module docstring: W is [in x 2 out], b
    [1 x 2 out], att [1 x out]; ValueError for another name, for attn_dropout > 0 and for set_dropout(attn > 0)) or "dot"
    (dot-product attention, see the module docstring: W is [in x 3 out], b [1 x 3 out], no att; the refusals of "v2" plus
    attention_weights, save, load and rows x 3 out >= 2^31); ``skip``: None, "add" or "gate", ``norm``: None or "layer",
    ``skip_weights``: per layer (W_r, b_r) or (W_r, b_r, w_gate) -- see the module docstring; ValueError for another name or
    a list that does not fit, and for save / load / save_best on a model that has either; ``label_input``: the rate in
    [0, 1) of masked label inputs and ``label_weights``: their table E -- see the module docstring and set_label_input;
    ``agg_dtype``: "f32" or "bf16" (bf16 gathers in the sparse attention kernels, see the module docstring; gcn's names and
    gcn's ValueError for another one).  ValueError
    before any device work for a width that its heads do not divide or a limit of the kernels (ops.GAT_MAX_HEADS,
    ops.GAT_MAX_WIDTH).  ``fused`` picks how Adam is launched -- one launch for every parameter tensor, or one per tensor;
    the element-wise math is the same, so both give the same bits -- and every other kernel is the same in both modes.

    ``dropout`` / ``attn_dropout`` / set_dropout(p, seed=0, epoch=0, attn=None): see the module docstring and
    gcn.dropout_option -- ``dropout_p``, ``attn_dropout_p``, ``dropout_seed`` and ``dropout_epoch`` (the number the next
    training forward gets) read the state; only train_forward / train_step drop, the backward pass uses the stream its
    forward used, and with both probabilities 0 the plain entry points are called and nothing is launched or allocated.
    ValueError for a probability outside [0, 1), or for more than 64 layers with one of them above 0, before any device work.

    __call__, train_forward, backward, adam_update, train_step (one synchronisation), evaluate, set_splits, split_metrics
    and layers() mean what they mean on ``gcn``, and so do save(ctx, path, optimizer=True) / load(ctx, path) / predict(ctx, X)
    (checkpoint.checkpoint_option): a file loads into a gat or dist_gat of the same variant, sizes, heads, attn_slope and
    loss, whatever ``fused`` is -- ValueError naming the first differing field before anything is written -- and brings both
    dropout probabilities, the seed and the epoch counter with it."""

    def __init__(self, A: csr_matrix, sizes: Sequence[int], heads=4, attn_slope: float = ops.GAT_SLOPE,
                 loss: str = "softmax", fused: bool = True, weights=None, dropout: float = 0.0, attn_dropout: float = 0.0,
                 variant: str = "v1", skip=None, norm=None, skip_weights=None, label_input: float = 0.0,
                 label_weights=None, agg_dtype: str = "f32", edge_attr=None, edge_weights=None, fanout=None,
                 edge_keep: float = 1.0):
        self.agg_dtype = _check_agg_dtype(agg_dtype)             # option checks come before any device work
        self.sizes = [int(s) for s in sizes]
        self.heads = check_heads(self.sizes, heads)              # option checks come before any device work
        self._attn_dropout_params = check_dropout(attn_dropout, len(self.sizes) - 1)
        self.variant = check_variant(variant, float(attn_dropout))
        E = check_edge_attr(edge_attr, edge_weights, self.variant, self.agg_dtype, len(self.sizes) - 1)
        if E is not None:
            self.edge_dim = int(E.shape[1])
        self._init_sampling(fanout, edge_keep)                   # refuses edge_attr with sampling on
        for li, w in enumerate(edge_weights if E is not None and edge_weights is not None else ()):
            if np.shape(w) != (self.heads[li], E.shape[1]):
                raise ValueError(f"edge_attr: edge_weights of layer {li} must be {self.heads[li]} x {E.shape[1]} (heads x de), "
                                 f"got {np.shape(w)}")
        self.skip, self.norm = check_skip(skip), check_norm(norm)
        check_skip_weights(self.skip, skip_weights, len(self.sizes) - 1)
        self._init_dropout(dropout, len(self.sizes) - 1)
        self.attn_dropout_p = float(attn_dropout)
        self.loss = check_loss(loss)
        self._label_threshold = check_label_input(label_input, self.loss, self.sizes[-1])
        if label_weights is not None and not label_input > 0.0:
            raise ValueError("label_weights needs label_input > 0")
        if A.n() != A.m():
            raise ValueError(f"gat needs a square matrix, got {A.n()} x {A.m()}")
        if E is not None and E.shape[0] != A.nnz():
            raise ValueError(f"edge_attr must have one row per entry of A, {A.nnz()}, got {E.shape[0]}")
        perm = edge_permutation(A) if E is not None else None    # on the host; refuses an indptr that does not begin with 0
        self.attn_slope = float(attn_slope)
        self._out_width = self.sizes[-1]
        self.fused = bool(fused)
        if self.variant == "dot" and A.n() * 3 * max(self.sizes[1:]) >= DOT_MAX_ELEMENTS:
            raise ValueError(f"gat(variant=\"dot\"): {A.n()} rows x 3 x {max(self.sizes[1:])} columns reach 2^31 elements, "
                             "more than one GEMM writes")
        import torch
        n_layers = len(self.sizes) - 1
        # the loss reads the logits and writes the gradient elsewhere: the last layer's backward needs its own output
        loss_class = sigmoid_bce_loss if self.loss == "bce" else softmax_cross_entropy_loss
        self.loss_layer = loss_class(f"{n_layers}_", True, True)
        self.A, self.A_T = A, A.transpose()                      # forward over A_T's rows, like gcn
        self.layers_: List[gat_layer] = []
        # the skip's r ("add") or G_r ("gate"), once at the widest layer; the defaults add nothing to a layer's arguments
        more = {}
        if self.skip is not None or self.norm is not None:
            self.skip_buffer = (torch.empty(A.n() * max(self.sizes[1:]), dtype=torch.float32, device="cuda")
                                if self.skip is not None else None)
            more = dict(skip=self.skip, norm=self.norm, skip_buffer=self.skip_buffer)
        if self.agg_dtype == "bf16":
            # the images the sparse kernels gather from, once at the widest layer: Z (1, 2 or 3 x out columns) and G
            zw = {"v1": 1, "v2": 2, "dot": 3}[self.variant]
            self.Z_image_buffer = torch.empty(A.n() * zw * max(self.sizes[1:]), dtype=torch.bfloat16, device="cuda")
            self.G_image_buffer = torch.empty(A.n() * max(self.sizes[1:]), dtype=torch.bfloat16, device="cuda")
            more.update(agg_dtype="bf16", images=(self.Z_image_buffer, self.G_image_buffer))
        if E is not None:
            # E twice on the device, shared by all layers: E_A in A's entry order for backward_src (it walks F^T = A), E_F in
            # A.transpose()'s for forward and backward_dst; and P_e once, at the layer with the most heads
            self.edge_dim = int(E.shape[1])
            self.E_A = dn_matrix.from_numpy(E)
            self.E_F = dn_matrix.from_numpy(E[perm])
            del perm
            self.P_e_buffer = torch.empty(A.n() * max(self.heads) * self.edge_dim, dtype=torch.float32, device="cuda")
            more.update(edge=(self.E_F, self.E_A, self.P_e_buffer))
        if self.variant == "v2":                                 # G_Z2 = [G_Zs | G_Zd] and P, once at the widest layer
            self.G_Z_buffer = torch.empty(A.n() * 2 * max(self.sizes[1:]), dtype=torch.float32, device="cuda")
            self.P_buffer = torch.empty(A.n() * max(self.sizes[1:]), dtype=torch.float32, device="cuda")
            for i in range(n_layers):
                self.layers_.append(gatv2_layer(f"{i}_", self.A_T, self.A, self.sizes[i], self.sizes[i + 1], self.heads[i],
                                                i + 1 < n_layers, self.attn_slope, i != 0, self.G_Z_buffer, self.P_buffer,
                                                **more))
        elif self.variant == "dot":                              # G_Z3 = [G_Zq | G_Zk | G_Zv], once at the widest layer
            self.G_Z_buffer = torch.empty(A.n() * 3 * max(self.sizes[1:]), dtype=torch.float32, device="cuda")
            for i in range(n_layers):
                self.layers_.append(gatdot_layer(f"{i}_", self.A_T, self.A, self.sizes[i], self.sizes[i + 1], self.heads[i],
                                                 i + 1 < n_layers, i != 0, self.G_Z_buffer, **more))
        else:
            self.G_Z_buffer = torch.empty(A.n() * max(self.sizes[1:]), dtype=torch.float32, device="cuda")
            for i in range(n_layers):
                self.layers_.append(gat_layer(f"{i}_", self.A_T, self.A, self.sizes[i], self.sizes[i + 1], self.heads[i],
                                              i + 1 < n_layers, self.attn_slope, i != 0, self.G_Z_buffer, **more))
        self._adam = None
        self._make_sampler(self.A_T, self.A)                     # nothing unless sampling is on
        self.label_input_p = float(label_input)
        if self.label_input_p > 0.0:                             # with 0 nothing is allocated, launched or registered
            self.label = self.layers_[0].label = _label_input_owner("0_", self.sizes[-1], self.layers_[0].Z.m())
            if label_weights is not None:
                self.label.init(label_weights)
        if skip_weights is not None:
            for layer, w in zip(self.layers_, skip_weights):
                layer.res_lin.W.init(np.asarray(w[0], dtype=np.float32))
                layer.res_lin.b.init(np.asarray(w[1], dtype=np.float32))
                if len(w) > 2:
                    layer.skip.init(w[2])
        if weights is not None:
            assert len(weights) == n_layers
            for layer, w in zip(self.layers_, weights):
                layer.W().init(np.asarray(w[0], dtype=np.float32))
                layer.b().init(np.asarray(w[1], dtype=np.float32))
                if len(w) > 2:
                    layer.attn.init(w[2])
        if E is not None and edge_weights is not None:
            for layer, w in zip(self.layers_, edge_weights):
                layer.attn.init_edge(w)

    # ---- edge features in the score (edge_attr=E) ----------------------------------------------------------------------------
    edge_dim = 0                        # de, the columns of edge_attr; 0 without the option
    E_A = E_F = P_e_buffer = None       # E in A's and in A.transpose()'s entry order, and the rows' shares of G_att_edge

    # ---- masked label inputs (label_input=rate) ----------------------------------------------------------------------------
    label = None                        # the label_input owner; layers()[0].label is the same object
    label_input_p = 0.0
    label_seed = label_epoch = 0
    _label_Y = _label_rows = _label_splits = _label_count = None

    def set_label_input(self, Y, rate: Optional[float] = None, seed: int = 0, epoch: int = 0) -> None:
        """Hands a gat(label_input=rate) model the labels it feeds.  Y: what train_step takes (an int32 dn_matrix of n x 1,
        or n integers); rate: None keeps the current one, else a number in [0, 1) -- with 0 a training forward feeds
        nothing and a plain one still feeds every training row; seed: 64 bits; epoch: the number the next training forward
        gets (set_label_input(Y, epoch=e) replays training forward e, the way set_dropout does).  Needs set_splits first;
        a later set_splits rebuilds the lists.  ValueError naming label_input, before any device work and before anything is
        stored, for a model built without the option, a rate outside [0, 1), missing splits and a label outside
        [0, classes) on a training row."""
        if self.label is None:
            raise ValueError("set_label_input needs a model built with label_input > 0: gat(..., label_input=rate)")
        threshold = self._label_threshold if rate is None else check_label_input(rate, self.loss, self.sizes[-1])
        if self.loss_layer.S is None and self._label_splits is None:
            raise ValueError("label_input: set_label_input needs set_splits(S) first (the training rows are the ones fed)")
        y = np.ascontiguousarray(Y.numpy() if isinstance(Y, dn_matrix) else Y).reshape(-1)
        if y.dtype.kind not in "iu" or y.size != self.A.n():
            raise ValueError(f"label_input: Y must hold {self.A.n()} integer labels, got {y.dtype} of {y.size}")
        self._build_label_lists(y)
        self._label_Y, self._label_threshold = y, threshold
        if rate is not None:
            self.label_input_p = float(rate)
        self.label_seed, self.label_epoch, self._label_count = int(seed) & 0xFFFFFFFFFFFFFFFF, int(epoch), None

    def _build_label_lists(self, y) -> None:
        """the kernels' lists from the labels and the splits the loss layer holds (one copy of S to the host, here only)"""
        if self._label_splits is None:                           # (S, counts, train_set) as set_splits left them
            ll = self.loss_layer
            self._label_splits = (ll.S, list(ll.counts), ll.train_set)
        S, _, train_set = self._label_splits
        host = S.numpy()
        rows, cls, cls_ptr = label_lists(host, y, train_set, self.sizes[-1])
        self.label.set_lists(rows, cls, cls_ptr, host, train_set)
        self._label_rows = np.sort(rows).astype(np.uint64) + np.uint64(self.layers_[0].row0)     # global row numbers

    def set_splits(self, S, train_set: int = 0) -> None:
        """model_base.set_splits; a label-input model that has its labels rebuilds its lists from the new splits"""
        model_base.set_splits(self, S, train_set)
        if self.label is not None:
            self._label_splits, self._label_count = None, None
            if self.loss_layer.S is None:
                self.label.rows = None                           # no splits: a forward asks for set_label_input again
            elif self._label_Y is not None:
                self._build_label_lists(self._label_Y)

    def _fed_count(self, epoch: int) -> int:
        """how many training rows training forward ``epoch`` feeds: the host's own Philox over the T training rows
        (label_mask), taken from _launched's look-ahead when that was for the same draw"""
        key = (epoch, self.label_seed, self._label_threshold)
        if self._label_count is None or self._label_count[0] != key:
            self._label_count = (key, label_mask.fed_count(self._label_rows, self._label_threshold, self.label_seed, epoch))
        return self._label_count[1]

    def _arm_label_input(self, training: bool) -> None:
        """hands layer 0's label_input the call of this forward and the loss layer the sets and counts that go with it: a
        training forward draws epoch ``label_epoch`` (and moves it on), its fed rows count as "other"; any other forward
        feeds every training row and leaves the splits as set_splits gave them.  ValueError before anything is launched."""
        lab, ll = self.label, self.loss_layer
        if lab.rows is None:
            raise ValueError("gat(label_input=...): call set_label_input(Y) after set_splits(S) before the first forward")
        S, counts, train_set = self._label_splits
        if not training:
            ll.S, ll.counts = S, list(counts)
            lab.call = (0, True, 0, 0, False)
            return
        fed = self._fed_count(self.label_epoch)
        if counts[train_set] - fed <= 0:
            raise ValueError(f"label_input: training forward {self.label_epoch} feeds all {counts[train_set]} training "
                             "rows, none is left to predict (lower the rate)")
        now = list(counts)
        now[train_set] -= fed
        now[ops.LABEL_INPUT_FED_SET] += fed
        ll.S, ll.counts = lab.S_e, now
        lab.call = (self._label_threshold, False, self.label_seed, self.label_epoch & 0xFFFFFFFF, True)
        self.label_epoch += 1

    def __call__(self, ctx: context, H: dn_matrix, training: bool = False) -> dn_matrix:
        if self.label is not None:
            self._arm_label_input(training)
        pair = self._draw_sample(ctx, training)                  # one sample per epoch, shared by all layers; None: the full graph
        for layer in self.layers_:
            layer.sample = pair
        return model_base.__call__(self, ctx, H, training)

    # ---- per-epoch edge sampling (fanout=, edge_keep=, set_sampling: edge_sample.sampling_option) ----------------------------
    def _refuse_sampling(self, fanout, keep) -> None:
        if getattr(self, "edge_dim", 0):
            raise ValueError("gat(edge_attr=...) has no edge sampling (fanout / edge_keep / set_sampling): the rows of E are "
                             "aligned to entry positions, which a sample does not keep")

    def _launched(self) -> None:
        """train_step's hook between its last launch and its synchronisation: the next epoch's count, while the device works"""
        if self.label is not None:
            self._fed_count(self.label_epoch)

    Z_image_buffer = G_image_buffer = None      # the bf16 images of gat(agg_dtype="bf16")

    def attention_weights(self, ctx, X=None, layers=None, out=None) -> List[dn_matrix]:
        """attention_model.attention_weights; ValueError for variant="dot", and for variant="v2" with agg_dtype="bf16",
        before anything else"""
        refuse_dot(self, "attention_weights: there is no export kernel for the dot-product coefficients yet")
        refuse_bf16_export(self, "attention_weights")
        refuse_edge_attr(self, "attention_weights: there is no export kernel with the edge term yet")
        return attention_model.attention_weights(self, ctx, X, layers, out)

    def attention_pattern(self):
        """(indptr, indices): the host arrays of the matrix the forward walks, A.transpose() -- row i is a destination, its
        entries are its sources, and row p of every matrix attention_weights returns belongs to indices[p]"""
        return self.A_T.indptr, self.A_T.indices

    def save(self, ctx, path: str, optimizer: bool = True) -> None:
        """checkpoint.checkpoint_option.save; ValueError for variant="dot" before anything is read, written or created"""
        refuse_checkpoint(self, "save: the checkpoint file")
        checkpoint_option.save(self, ctx, path, optimizer)

    def load(self, ctx, path: str) -> None:
        """checkpoint.checkpoint_option.load; ValueError for variant="dot" before the file is opened"""
        refuse_checkpoint(self, "load: the checkpoint file")
        checkpoint_option.load(self, ctx, path)

    def _write_checkpoint(self, ctx, path: str, tensors, optimizer: bool, step: int) -> None:
        refuse_checkpoint(self, "checkpoint file (model_selector.save_best included): it")
        checkpoint_option._write_checkpoint(self, ctx, path, tensors, optimizer, step)
