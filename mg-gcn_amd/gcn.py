"""Layer API of the reference (src/gcn.hpp) over the HIP engine, single GPU.

``sparse_linear`` (src/gcn.hpp:13-48), ``linear`` (:88-189), ``gcn_layer``
(:411-518), ``softmax`` (:639-676), ``softmax_cross_entropy_loss`` (:769-823),
``gcn`` (:937-995) -- same names, constructor arguments, call/backward/
adam_update members, buffer aliasing and timer names.

``fused=True`` (default for ``gcn``) swaps three launch chains for their fused
kernels -- identical math, fewer passes:
  * leaky-ReLU folded into the SpMM epilogue when the SpMM is the layer's last op,
  * softmax + argmax + log-prob + gradient in one kernel instead of 8 + a GEMM,
  * leaky-ReLU-backward folded into the epilogue of the GEMM that PRODUCES its gradient operand
    (layer i+1's G_out = G_HW . W^T, masked by layer i+1's own input = layer i's activated output),
  * one Adam launch for all parameter tensors of the model instead of 7 per layer.
``fused=False`` runs the reference's launch sequence one for one.

``agg_dtype="bf16"`` (opt-in; default ``"f32"``) stores the gathered operand of every SpMM in bf16: each aggregation
rounds its dense input to bf16 into one model-owned scratch and multiplies with the bf16 SpMM, C = A . bf16(B), sums
and everything else in fp32 (GEMMs, loss, weights, gradients, Adam).

``dropout=p`` (opt-in; default 0: nothing is launched) drops the input of every layer but the first during a training
forward, with a counter-based mask that is never stored (ops.dropout, include/mggcn.h: mggcn_dropout_f32): the backward
pass regenerates it, a row-partitioned run draws the single-GPU run's mask, and numpy reproduces it bit for bit.

``norm="layer"`` (opt-in; default None: nothing is launched) puts a layer normalisation between the aggregation / linear
and the activation of every layer but the last (ops.layer_norm, include/mggcn.h: mggcn_layer_norm_forward_f32); the
activation rides in the norm kernels, and the norm's gamma / beta are trained by Adam without weight decay.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import ops
from .checkpoint import checkpoint_option
from .edge_sample import refuse_sampling, rescaled_sampling_option, sampling_on
from .matrix import context, csr_matrix, dn_matrix, host_scalars

MGGCN_SPMM_LEAKY_RELU = 1
_SQRT_1_3 = float(np.sqrt(np.float32(1.0) / np.float32(3)))     # b.init(std::sqrt((r_t)1.0 / 3)), gcn.hpp:109


def _torch():
    import torch
    return torch


AGG_DTYPES = ("f32", "bf16")


def _check_agg_dtype(agg_dtype: str) -> str:
    if agg_dtype not in AGG_DTYPES:
        raise ValueError(f"agg_dtype must be one of {AGG_DTYPES}, not {agg_dtype!r}")
    return agg_dtype


DROPOUT_MAX_LAYERS = 64            # the dropout stream of a call is epoch * 64 + the consuming layer's index


def check_dropout(p: float, n_layers: int):
    """option checking of dropout, before any device work: (threshold, scale) of ops.dropout_params, and no more than
    DROPOUT_MAX_LAYERS layers when p > 0"""
    params = ops.dropout_params(p)
    if float(p) > 0.0 and n_layers > DROPOUT_MAX_LAYERS:
        raise ValueError(f"dropout supports at most {DROPOUT_MAX_LAYERS} layers, the model has {n_layers}")
    return params


NORMS = (None, "layer")


def check_norm(norm):
    """option checking of norm=, before any device work: None (no normalisation) or "layer" """
    if norm is not None and norm != "layer":
        raise ValueError(f"norm must be one of {NORMS}, not {norm!r}")
    return norm


class dropout_option:
    """set_dropout of gcn and dist.dist_gcn (opt-in; the reference has no dropout).

    Dropout applies to the INPUT of every layer but the first: the activated output of the layer below, after any
    residual add, in place in that layer's AHW buffer.  The features X are the caller's buffer and are never dropped.
    The mask of layer l in training forward number e (counted from set_dropout; ``dropout_epoch`` is the next one) is the
    one of ops.dropout with (seed, stream = (e * 64 + l) mod 2^32, row0 = the global index of this GPU's first row);
    backward() applies the same call to the gradient that layer returns.  Only train_forward / train_step drop: a plain
    call of the model and evaluate() never do.  With splits on, split_metrics() of a training epoch therefore reports
    the DROPPED forward's validation and test numbers; evaluate() gives the clean ones."""

    def _init_dropout(self, p: float, n_layers: int) -> None:
        self._dropout_layers = int(n_layers)
        self._dropout_params = check_dropout(p, n_layers)
        self.dropout_p, self.dropout_seed, self.dropout_epoch = float(p), 0, 0

    def set_dropout(self, p: float, seed: int = 0, epoch: int = 0) -> None:
        """p in [0, 1): the drop probability (0 switches dropout off: no kernel is launched); seed: 64 bits; epoch: the
        number the next training forward gets (set_dropout(p, seed, epoch=e) replays training forward e).  ValueError for
        a p outside [0, 1) or a model of more than 64 layers, before any device work."""
        self._dropout_params = check_dropout(p, self._dropout_layers)
        self.dropout_p = float(p)
        self.dropout_seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.dropout_epoch = int(epoch)

    def _arm_dropout(self, training: bool) -> None:
        """hands every layer but the first its call of this forward (None: no dropout); a training forward takes the
        current epoch number and moves it on"""
        on = bool(training) and self.dropout_p > 0.0
        threshold, scale = self._dropout_params
        for li, layer in enumerate(self.layers_):
            layer.dropout = ((threshold, scale, self.dropout_seed, (self.dropout_epoch * DROPOUT_MAX_LAYERS + li) & 0xFFFFFFFF)
                             if on and li > 0 else None)
        if on:
            self.dropout_epoch += 1


class sparse_linear:
    """reference src/gcn.hpp:13-48: holds (A, A_T); forward SpMM with A, backward with A_T.

    ``sample``: the pair (sample of A, sample of A_T) of this forward where the model drew an edge sample with values
    (edge_sample.py), as max_aggregate has it; None: the full graph.  With a sample the forward and the backward multiply by it
    through ops.spmm_dev on the plan built with the draw -- no host plan is looked up, made or touched."""

    sample = None

    def __init__(self, name: str, A: csr_matrix, A_T: csr_matrix, agg_dtype: str = "f32", agg_buffer=None):
        self.name, self.A, self.A_T = name, A, A_T
        self.M = self.M2 = 0
        self.ext_buffer = self.ext_buffer2 = None
        self._max_d = [128, 128]     # plans are sized for at least the reference's hidden width
        self.agg_dtype = _check_agg_dtype(agg_dtype)
        self.agg_buffer = agg_buffer  # bf16: flat bf16 device tensor the dense operand is rounded into (grown on demand)

    def _spmm(self, ctx: context, M: csr_matrix, B: dn_matrix, C: dn_matrix, plan, beta: float, flags: int) -> None:
        if self.agg_dtype == "f32":
            ops.matmul(ctx, M, B, C, plan, 1.0, beta, flags)
            return
        torch = _torch()
        need = B.n() * B.m()
        if self.agg_buffer is None or self.agg_buffer.numel() < need:
            self.agg_buffer = torch.empty(need, dtype=torch.bfloat16, device=ctx.device)
        B16 = self.agg_buffer[:need].view(B.n(), B.m())
        ops.convert_bf16(ctx, B, B16)
        ops.spmm_bf16(ctx, M, B16, C, plan, 1.0, beta, flags)

    def _spmm_sampled(self, ctx: context, S, B: dn_matrix, C: dn_matrix, beta: float, flags: int) -> None:
        """_spmm over the sampled matrix ``S`` (edge_sample.sampled_csr with values and a built device plan)"""
        if self.agg_dtype != "f32":
            torch = _torch()
            need = B.n() * B.m()
            if self.agg_buffer is None or self.agg_buffer.numel() < need:
                self.agg_buffer = torch.empty(need, dtype=torch.bfloat16, device=ctx.device)
            B16 = self.agg_buffer[:need].view(B.n(), B.m())
            ops.convert_bf16(ctx, B, B16)
            B = B16
        ops.spmm_dev(ctx, S, B, C, S.plan, 1.0, beta, flags)

    def __call__(self, ctx: context, B: dn_matrix, C: dn_matrix, discard: bool = True, flags: int = 0) -> None:
        n = self.name
        if self.sample is not None:
            ctx.record(n + "0_0_matmul-spmm", 0)
            self._spmm_sampled(ctx, self.sample[0], B, C, 0.0 if discard else 1.0, flags)
            ctx.record(n + "0_1_matmul-spmm", 0)
            ctx.register_timer(n + "0_matmul-spmm", n + "0_0_matmul-spmm", n + "0_1_matmul-spmm")
            return
        if B.m() != self.M:                                   # workspace cached per width, gcn.hpp:28-31
            self.M = B.m()
            if self.ext_buffer is None or B.m() > self._max_d[0]:
                self._max_d[0] = max(B.m(), self._max_d[0])
                self.ext_buffer = ops.get_matmul_buffer(ctx, self.A, B, C, 1.0, 0.0 if discard else 1.0,
                                                        max_d=self._max_d[0])
        ctx.record(n + "0_0_matmul-spmm", 0)
        self._spmm(ctx, self.A, B, C, self.ext_buffer, 0.0 if discard else 1.0, flags)
        ctx.record(n + "0_1_matmul-spmm", 0)
        ctx.register_timer(n + "0_matmul-spmm", n + "0_0_matmul-spmm", n + "0_1_matmul-spmm")

    def backward(self, ctx: context, G: dn_matrix, G_out: dn_matrix, discard: bool = True) -> None:
        n = self.name
        if self.sample is not None:
            ctx.record(n + "1_0_matmul-spmm", 0)
            self._spmm_sampled(ctx, self.sample[1], G, G_out, 0.0 if discard else 1.0, 0)
            ctx.record(n + "1_1_matmul-spmm", 0)
            ctx.register_timer(n + "1_matmul-spmm", n + "1_0_matmul-spmm", n + "1_1_matmul-spmm")
            return
        if G.m() != self.M2:
            self.M2 = G.m()
            if self.ext_buffer2 is None or G.m() > self._max_d[1]:
                self._max_d[1] = max(G.m(), self._max_d[1])
                self.ext_buffer2 = ops.get_matmul_buffer(ctx, self.A_T, G, G_out, 1.0, 0.0 if discard else 1.0,
                                                         max_d=self._max_d[1])
        ctx.record(n + "1_0_matmul-spmm", 0)
        self._spmm(ctx, self.A_T, G, G_out, self.ext_buffer2, 0.0 if discard else 1.0, 0)
        ctx.record(n + "1_1_matmul-spmm", 0)
        ctx.register_timer(n + "1_matmul-spmm", n + "1_0_matmul-spmm", n + "1_1_matmul-spmm")


class param_owner:
    """Whatever holds parameter tensors that Adam trains: linear, layer_norm, and gat's attention, attention_v2, gated_skip
    and attention_dot.  ``params_table`` describes each tensor once, one row per tensor in file order: (file-name stem,
    parameter attribute, gradient attribute, m attribute, v attribute, decays like W).  The rows hold attribute NAMES, read
    at call time: dist_gat.dist_attention rebinds G_att after __init__ and dist.dist_row_linear places G_W / G_b inside its
    all-reduced buffer.  checkpoint.model_params names the file's tensors from the same rows.

    ``adam_fused`` picks the per-tensor step (the model-wide one is adam_update_all): True is one ops.adam_fused per
    tensor, the element-wise math of the model-wide table bit for bit; False is the reference's unfused chain
    (gcn.hpp:146-172), which rounds differently."""

    params_table = ()
    adam_fused = False
    step = 0

    def adam_state(self, ctx: context) -> None:
        """the moments, zeroed on the parameter's device, and step 0 -- made on first use"""
        if self.params_table and getattr(self, self.params_table[0][3]) is None:
            for _, p, _, m, v, _ in self.params_table:
                p = getattr(self, p)
                for moment in (m, v):
                    setattr(self, moment, dn_matrix(p.shape(), device=p.t.device))
                    getattr(self, moment).zero(ctx)
            self.step = 0

    def adam_tensors(self, weight_decay: float):
        """(param, grad, m, v, weight decay) per tensor for ops.adam_table: only W and what decays like it (gcn.hpp:163)"""
        return [(getattr(self, p), getattr(self, g), getattr(self, m), getattr(self, v), weight_decay if decays else 0.0)
                for _, p, g, m, v, decays in self.params_table]

    def adam_update(self, ctx: context, lr: float, beta1: float, beta2: float, weight_decay: float, eps: float) -> None:
        self.adam_state(ctx)
        self.step += 1
        bc1 = float(np.float32(1 - beta1 ** self.step))
        bc2 = float(np.float32(1 - beta2 ** self.step))
        rows = self.adam_tensors(weight_decay)
        if self.adam_fused:
            for p, g, m, v, wd in rows:
                ops.adam_fused(ctx, p, g, m, v, lr, beta1, beta2, wd, bc1, bc2, eps)
            return
        for (p, g, *_), (*_, decays) in zip(rows, self.params_table):      # phase by phase over the tensors, as the reference
            if decays:
                ops.axpy(ctx, p, g, weight_decay)
        for _, g, m, _, _ in rows:
            ops.axpby(ctx, g, m, 1 - beta1, beta1)
        for _, g, _, v, _ in rows:
            ops.aaxpby(ctx, g, v, 1 - beta2, beta2)
        for p, _, m, v, _ in rows:
            ops.adam_final(ctx, p, m, v, lr, bc1, bc2, eps)


class linear(param_owner):
    """reference src/gcn.hpp:88-189: XW = X.W + 1 b^T; backward G_b, G_W, G_out; Adam.

    The body of the row-partitioned form too (dist.dist_row_linear, gcn.hpp:191-296): every operand here is a dn_matrix
    on ``ctx``'s device -- the rank's shard of X and G, its replica of W and b.  What the distributed form adds lives in
    the two hooks it overrides: _gradients (where G_W / G_b are stored) and _reduce_gradients (runs after the
    weight-gradient GEMMs), plus finish_backward.  ``fused`` picks the per-tensor Adam step too (param_owner)."""

    params_table = (("W", "W", "G_W", "mW", "vW", True), ("b", "b", "G_b", "mb", "vb", False))
    mW = vW = mb = vb = None

    def __init__(self, name: str, in_: int, out: int, backward_out: bool = True, fused: bool = False):
        self.name = name
        self.W = dn_matrix(in_, out)
        self.G_W, self.G_b = self._gradients(in_, out)
        self.b = dn_matrix(1, out)
        self.backward_out, self.fused, self.adam_fused = backward_out, fused, fused
        self.W.init()
        self.b.init(_SQRT_1_3)
        self.X: Optional[dn_matrix] = None
        self.ones: Optional[dn_matrix] = None

    def _gradients(self, in_: int, out: int) -> Tuple[dn_matrix, dn_matrix]:
        return dn_matrix(in_, out), dn_matrix(1, out)

    def _reduce_gradients(self, ctx: context) -> None:
        """after the weight-gradient GEMMs: nothing to do on one GPU"""

    def finish_backward(self, ctx) -> None:
        """from here on the compute stream sees the final G_W / G_b: nothing to wait for on one GPU"""

    def setX(self, new_X: dn_matrix) -> None:
        self.X = new_X

    def __call__(self, ctx: context, X: dn_matrix, XW: dn_matrix, discard: bool = True) -> None:
        n = self.name
        if self.fused and discard:                  # bias in the GEMM epilogue: one pass, C never read
            ctx.record(n + "0_0_matmul-gemm", 0)
            ops.linear_forward(ctx, X, self.W, self.b, XW)
        else:
            ops.broadcast_rows(ctx, self.b, XW, discard)
            ctx.record(n + "0_0_matmul-gemm", 0)
            ops.matmul(ctx, X, self.W, XW, 1.0, 1.0)
        ctx.record(n + "0_1_matmul-gemm", 0)
        ctx.register_timer(n + "0_matmul-gemm", n + "0_0_matmul-gemm", n + "0_1_matmul-gemm")
        self.X = X

    def backward(self, ctx: context, G: dn_matrix, G_out: Optional[dn_matrix], discard: bool = True,
                 mask: Optional[dn_matrix] = None) -> None:
        """``mask`` (fused path): the activated output Z of the layer below -- G_out leaves the GEMM already
        multiplied by leaky_relu'(Z), i.e. it IS the T of that layer's backward (gcn.hpp:462-468)."""
        n = self.name
        if self.ones is None or self.ones.m() != G.n():
            self.ones = dn_matrix(1, G.n(), device=ctx.device)
            ctx.fill(self.ones, 1.0)        # host-side std::fill in the reference (gcn.hpp:127-128)
        ctx.record(n + "1_0_matmul-gemm", 0)
        if self.fused:                      # G_b rides on the B tiles of the G_W kernel: one pass over G
            ctx.record(n + "1_1_matmul-gemm", 0)
            ops.linear_backward_weights(ctx, self.X, G, self.G_W, self.G_b)
        else:
            ops.matmul(ctx, self.ones, G, self.G_b, 1.0, 0.0)
            ctx.record(n + "1_1_matmul-gemm", 0)
            ops.matmul(ctx, self.X, G, self.G_W, 1.0, 0.0, True)
        self._reduce_gradients(ctx)
        ctx.record(n + "1_2_matmul-gemm", 0)
        if self.backward_out and mask is not None:
            assert discard
            ops.matmul_lrelu_backward(ctx, G, self.W, mask, G_out, 1.0, False, True)
        elif self.backward_out:
            ops.matmul(ctx, G, self.W, G_out, 1.0, 0.0 if discard else 1.0, False, True)
        ctx.record(n + "1_3_matmul-gemm", 0)
        ctx.register_timer(n + "1_matmul-gemm", n + "1_0_matmul-gemm", n + "1_3_matmul-gemm")

    def update(self, ctx: context, lr: float, weight_decay: float) -> None:      # gcn.hpp:141-144
        ops.axpby(ctx, self.G_W, self.W, -lr, 1 - weight_decay)
        ops.axpy(ctx, self.G_b, self.b, -lr)

    def adam_update(self, ctx: context, lr: float, beta1: float, beta2: float, weight_decay: float,
                    eps: float) -> None:
        self.finish_backward(ctx)
        self.adam_state(ctx)                # the first step's zero fills stay outside the timer
        n = self.name
        ctx.record(n + "0_adam-update", 0)
        param_owner.adam_update(self, ctx, lr, beta1, beta2, weight_decay, eps)
        ctx.record(n + "1_adam-update", 0)
        ctx.register_timer(n + "adam-update", n + "0_adam-update", n + "1_adam-update")

    def get_b(self): return self.b
    def get_W(self): return self.W
    def get_G_W(self): return self.G_W
    def get_G_b(self): return self.G_b


class layer_norm(param_owner):
    """Layer normalisation of a layer's [n x out] pre-activation, in place, with the activation in the same launch
    (opt-in; the reference has none): gamma (ones) and beta (zeros) [1 x out], their gradients and Adam moments, and what
    the backward pass needs of the forward -- xhat [n x out] and rstd [n].  Row-local: a row shard normalises exactly the
    rows the single-GPU model does, and its two gradient rows are summed over the ranks with the linear's
    (``grad_buffer``: 2 * out floats inside that linear's all-reduced buffer).  Neither gamma nor beta decays;
    ``adam_fused``: the per-tensor Adam step (param_owner) -- gcn's is the unfused chain linear runs for b, gat's the fused
    kernel of every other parameter of an attention model."""

    params_table = (("gamma", "gamma", "G_gamma", "mg", "vg", False), ("beta", "beta", "G_beta", "mb", "vb", False))
    mg = vg = mb = vb = None

    def __init__(self, name: str, n: int, out: int, fused: bool = False, device=None, grad_buffer=None,
                 adam_fused: bool = False):
        self.name, self.fused, self.adam_fused = name, fused, adam_fused
        self.gamma, self.beta = dn_matrix(1, out, device=device), dn_matrix(1, out, device=device)
        self.gamma.init(np.ones((1, out), dtype=np.float32))
        self.beta.init(np.zeros((1, out), dtype=np.float32))
        if grad_buffer is None:
            self.G_gamma, self.G_beta = dn_matrix(1, out, device=device), dn_matrix(1, out, device=device)
        else:
            self.G_gamma, self.G_beta = dn_matrix(1, out, grad_buffer[:out]), dn_matrix(1, out, grad_buffer[out:2 * out])
        self.xhat, self.rstd = dn_matrix(n, out, device=device), dn_matrix(n, 1, device=device)

    def __call__(self, ctx: context, Z: dn_matrix, activation: bool, out: Optional[dn_matrix] = None) -> None:
        """Z = [leaky_relu](layer_norm(Z)) in place, or into ``out`` where Z has to stay (a gat layer's aggregated output)"""
        n = self.name
        ctx.record(n + "0_0_norm", 0)
        ops.layer_norm(ctx, Z, Z if out is None else out, self.xhat, self.rstd, self.gamma, self.beta,
                       ops.LAYER_NORM_LEAKY_RELU if activation else 0)
        ctx.record(n + "0_1_norm", 0)
        ctx.register_timer(n + "0_norm", n + "0_0_norm", n + "0_1_norm")

    def backward(self, ctx: context, G: dn_matrix, act: Optional[dn_matrix], G_in: dn_matrix) -> None:
        """G_in = the gradient of the norm's input, G_gamma / G_beta; ``act``: apply leaky_relu'(act) to G first"""
        n = self.name
        ctx.record(n + "1_0_norm", 0)
        ops.layer_norm_backward(ctx, G, act, self.xhat, self.rstd, self.gamma, G_in, self.G_gamma, self.G_beta,
                                ops.LAYER_NORM_LEAKY_RELU if act is not None else 0)
        ctx.record(n + "1_1_norm", 0)
        ctx.register_timer(n + "1_norm", n + "1_0_norm", n + "1_1_norm")

    def init(self, gamma, beta) -> None:
        self.gamma.init(np.asarray(gamma, dtype=np.float32))
        self.beta.init(np.asarray(beta, dtype=np.float32))


class layer_params:
    """What a layer of any model says about its parameters: owners() lists (file-name prefix, param_owner) in file order,
    and params(), the per-tensor adam_update and the reference's accessors follow from it."""

    def owners(self):
        raise NotImplementedError

    def params(self):
        """everything Adam updates: the owners that hold a tensor"""
        return [owner for _, owner in self.owners() if owner.params_table]

    def adam_update(self, ctx, lr, beta1, beta2, weight_decay, eps):
        for p in self.params():
            p.adam_update(ctx, lr, beta1, beta2, weight_decay, eps)

    def b(self): return self.lin.get_b()
    def W(self): return self.lin.get_W()
    def GW(self): return self.lin.get_G_W()
    def Gb(self): return self.lin.get_G_b()


class layer_body(layer_params):
    """Forward and backward of one GCN layer, reference src/gcn.hpp:411-518 (gcn_layer) and :520-637 (dist_gcn_layer),
    over a context and dn_matrix operands: the layer's rows on this GPU.  HW / G_HW alias the model-wide HW_buffer,
    AHW / G_out alias the layer's AHW_buffer (:433-434).  ``agg`` is the aggregation operator: agg(ctx, B, C, discard,
    flags) and agg.backward(ctx, G, G_out) -- sparse_linear for one GPU, dist_sparse_linear bound to its dist_context
    for the row partition."""

    def __init__(self, name: str, agg, lin: linear, res_lin: Optional[linear], residual_layer: bool, HW: dn_matrix,
                 AHW: dn_matrix, G_HW: dn_matrix, G_out: dn_matrix, activation: bool, backward_spmm: bool, fused: bool,
                 norm: Optional[layer_norm] = None):
        self.name, self._agg, self.lin, self.res_lin = name, agg, lin, res_lin
        # layer normalisation between aggregation / linear and activation (gcn(norm="layer")): only where there is an
        # activation, i.e. never in the last layer
        assert norm is None or activation
        self.norm = norm
        # residual connection (gcn.hpp:418, :430): a second linear when the widths differ, a plain add otherwise
        self.residual_layer = bool(residual_layer)
        self.HW, self.AHW, self.G_HW, self.G_out = HW, AHW, G_HW, G_out
        self.activation, self.backward_spmm, self.fused = activation, backward_spmm, fused
        self.H: Optional[dn_matrix] = None
        # fused backward (set by the model): mask_input_grad -- my G_out GEMM applies leaky_relu'(H) of the layer
        # below; grad_premasked -- the G I receive already carries my own activation's mask
        self.mask_input_grad = self.grad_premasked = False
        # optional (gcn(hoist_first_aggregation=True), first layer only): A_fwd . X computed once and kept
        self.hoist_input = False
        self._AX: Optional[dn_matrix] = None
        self._AX_key = None
        # dropout of my input (set by the model before every forward, see dropout_option): None, or (threshold, scale,
        # seed, stream) of ops.dropout_raw; row0: the global index of my first row (the row partition sets its shard's)
        self.dropout = None
        self.row0 = 0

    def _drop(self, ctx: context, M: dn_matrix, tag: str) -> None:
        """M = dropout(M) in place with this forward's mask: H on the way up ("0"), G_out on the way down ("1")"""
        n = self.name
        threshold, scale, seed, stream = self.dropout
        ctx.record(n + tag + "_0_dropout", 0)
        ops.dropout_raw(ctx, M, M, threshold, scale, seed, stream, self.row0)
        ctx.record(n + tag + "_1_dropout", 0)
        ctx.register_timer(n + tag + "_dropout", n + tag + "_0_dropout", n + tag + "_1_dropout")

    def gemm_first(self) -> bool:
        return self.HW.m() == self.AHW.m()        # out <= in (gcn.hpp:439)

    def __call__(self, ctx: context, H: dn_matrix) -> dn_matrix:
        if self.dropout is not None:
            # In place in the AHW buffer of the layer below.  Its backward reads that buffer for the SIGN of its
            # activation only (leaky_relu_backward, or the epilogue of my G_out GEMM): scaling by 1 / (1 - p) > 0 keeps
            # it, and where the element was dropped my backward returns a zero gradient whatever leaky_relu'(0) says.
            self._drop(ctx, H, "0")
        self.H = H
        n = self.name
        act_done = False
        if self.hoist_input and self.HW.m() == self.AHW.m():
            # Layer 0's aggregation is loop-invariant: A_fwd (X W + 1 b^T) = (A_fwd X) W + 1 b^T because A_fwd is
            # row-stochastic (A_fwd 1 = 1) and X never changes between epochs -- so A_fwd X is computed ONCE (one
            # SpMM at d = in, kept: n x in floats) and the epoch runs one SpMM fewer.  Not what the reference executes
            # per epoch (src/gcn.hpp:437-446): an option, off by default, reported separately by bench.py.  The
            # backward pass is the reference's (G_W = X^T T with the first layer's backward SpMM skipped, :954).
            # keyed on the feature buffer AND the matrix's generation (csr_matrix bumps _version when it is re-normalised
            # or replaced).  An IN-PLACE update of the feature tensor is not visible here: call
            # set_hoist_first_aggregation(True) again (it drops the cached product) after changing X in place.
            key = (H.buffer(), H.n(), H.m(), getattr(self._agg.A, "_version", 0))
            if self._AX is None or self._AX_key != key:
                self._AX = dn_matrix(self._agg.A.n(), H.m())
                self._agg(ctx, H, self._AX)
                self._AX_key = key
            self.lin(ctx, self._AX, self.AHW)
            self.lin.setX(H)
        elif self.HW.m() == self.AHW.m():         # out <= in: GEMM first (gcn.hpp:439-442)
            self.lin(ctx, H, self.HW)
            if self.fused and self.activation and self.norm is None:     # with a norm the activation rides in ITS kernel
                self._agg(ctx, self.HW, self.AHW, True, MGGCN_SPMM_LEAKY_RELU)
                act_done = True
            else:
                self._agg(ctx, self.HW, self.AHW)
        else:                                      # gcn.hpp:443-446
            self._agg(ctx, H, self.HW)
            self.lin(ctx, self.HW, self.AHW)
        if self.norm is not None:
            self.norm(ctx, self.AHW, self.fused)          # fused: norm and activation in one launch
            act_done = self.fused
        if self.activation and not act_done:
            ctx.record(n + "0_0_activation", 0)
            ops.leaky_relu_forward(ctx, self.AHW, self.AHW)
            ctx.record(n + "0_1_activation", 0)
            ctx.register_timer(n + "0_activation", n + "0_0_activation", n + "0_1_activation")
        if self.res_lin is not None:              # gcn.hpp:453-456: AHW += H . W_res + 1 b_res^T
            self.res_lin(ctx, H, self.AHW, False)
        elif self.residual_layer:
            ops.axpy(ctx, H, self.AHW, 1.0)
        return self.AHW

    def backward(self, ctx: context, G: dn_matrix) -> dn_matrix:
        n = self.name
        T = G
        if self.norm is not None and self.fused:
            # one launch: leaky_relu'(AHW as the forward left it) unless G already carries it, then the norm's backward;
            # T lands in AHW
            self.norm.backward(ctx, G, None if self.grad_premasked else self.AHW, self.AHW)
            T = self.AHW
        elif self.activation and not self.grad_premasked:
            ctx.record(n + "1_0_activation", 0)
            ops.leaky_relu_backward(ctx, self.AHW, G, self.AHW)
            ctx.record(n + "1_1_activation", 0)
            ctx.register_timer(n + "1_activation", n + "1_0_activation", n + "1_1_activation")
            T = self.AHW
            if self.norm is not None:
                self.norm.backward(ctx, self.AHW, None, self.AHW)
        if self.HW.m() == self.AHW.m():
            G_HW = self.G_HW
            if self.backward_spmm:
                self._agg.backward(ctx, T, G_HW)
            else:
                G_HW = T
            self.lin.backward(ctx, G_HW, self.G_out, mask=self.H if self.mask_input_grad else None)
            G_out = self.G_out
        else:
            self.lin.setX(self.H)
            self.lin.backward(ctx, T, self.G_HW)
            G_out = self.G_HW
            if self.backward_spmm:
                self._agg.backward(ctx, self.G_HW, self.G_out)
                G_out = self.G_out
        if self.res_lin is not None:              # gcn.hpp:484-487: the residual branch sees the incoming G
            self.res_lin.backward(ctx, G, G_out, False)
        elif self.residual_layer:
            ops.axpy(ctx, G, G_out, 1.0)
        if self.dropout is not None:              # last: after the GEMM epilogue's leaky_relu' and the residual add
            self._drop(ctx, G_out, "1")
        return G_out

    def linears(self):
        return [self.lin] + ([self.res_lin] if self.res_lin is not None else [])

    def owners(self):
        """the linears, then the norm (linears() stays what the reference's layer has)"""
        return [(prefix, o) for prefix, o in (("", self.lin), ("res_", self.res_lin), ("", self.norm)) if o is not None]

    def finish_backward(self, ctx) -> None:
        for lin in self.linears():
            lin.finish_backward(ctx)

    def update(self, ctx, lr, weight_decay):
        for lin in self.linears():
            lin.update(ctx, lr, weight_decay)


class gcn_layer(layer_body):
    """reference src/gcn.hpp:411-518, one GPU."""

    def __init__(self, name: str, A: csr_matrix, A_T: csr_matrix, in_: int, out: int, activation: bool,
                 residual_layer: bool = False, backward_spmm: bool = True, HW_buffer=None, fused: bool = False,
                 agg_dtype: str = "f32", agg_buffer=None, norm=None):
        torch = _torch()
        check_norm(norm)
        self.A = sparse_linear(name, A, A_T, agg_dtype, agg_buffer)
        mn = min(in_, out)
        if HW_buffer is None:
            HW_buffer = torch.empty(max(A.m(), A_T.n()) * mn, dtype=torch.float32, device="cuda")
        self.AHW_buffer = torch.empty(max(A.n() * out, A_T.n() * in_), dtype=torch.float32, device="cuda")
        lin = linear(name, in_, out, backward_spmm, fused)
        res_lin = linear(name, in_, out, backward_spmm, False) if residual_layer and in_ != out else None
        layer_body.__init__(self, name, self.A, lin, res_lin, residual_layer,
                            dn_matrix(A.m(), mn, HW_buffer), dn_matrix(A.n(), out, self.AHW_buffer),
                            dn_matrix(A_T.n(), mn, HW_buffer), dn_matrix(A_T.n(), in_, self.AHW_buffer),
                            activation, backward_spmm, fused,
                            layer_norm(name, A.n(), out, fused) if norm == "layer" and activation else None)


class softmax:
    """reference src/gcn.hpp:639-676: row max, exp(x - max), row sums via a GEMM with a
    ones vector, divide."""

    def __init__(self, copy: bool = True):
        self.copy = copy
        self.H = self.H_R = self.maxs = self.ones = None

    def __call__(self, ctx: context, temp: dn_matrix) -> dn_matrix:
        if self.copy:
            if self.H is None:
                self.H = dn_matrix(temp.n(), temp.m())
            temp.copy_to(ctx, self.H)
        else:
            self.H = temp
        H = self.H
        if self.maxs is None:
            self.maxs = dn_matrix(H.n(), 1)
        ops.max_rows(ctx, H, self.maxs)
        ops.subtract_rows_exp(ctx, H, self.maxs, H)
        if self.ones is None:
            self.ones = dn_matrix(H.m(), 1)
            ctx.fill(self.ones, 1.0)
        if self.H_R is None:
            self.H_R = dn_matrix(H.n(), 1)
        ops.matmul(ctx, H, self.ones, self.H_R, 1.0, 0.0)
        ops.scale_rows(ctx, H, self.H_R)
        return H


class softmax_cross_entropy_loss:
    """reference src/gcn.hpp:769-823.  Returns (loss, acc) = (sum|log p_y|, #correct) / n
    after a device sync, exactly where the reference blocks (:816-817).
    fused=True is the one-pass kernel for 1 <= m <= ops.XENT_FUSED_MAX_CLASSES classes; any other width runs the
    unfused chain, with the results of fused=False.

    set_splits(S, counts, train_set) (opt-in; the reference loads sets.bin and ignores it, src/main.cpp:85) makes the
    layer split-aware: rows outside train_set get a zero gradient row, the gradient is scaled by 1 / (the global number
    of training rows), (loss, acc) are the training split's, and split_metrics() reports every split of the last call --
    from the same pass, which sums a (loss, correct) pair per slot train / val / test / other."""

    def __init__(self, name: str, copy: bool = True, fused: bool = False, host_sums: bool = True):
        """host_sums: keep the reported sums in mapped pinned host memory (read without a device-to-host copy);
        False = a device tensor (the distributed wrapper all-reduces it over RCCL)"""
        self.name = name
        self.softmax_layer = softmax(copy)
        self.copy, self.fused, self.host_sums = copy, fused, host_sums
        self.G = self.L = self.P = self.T = None
        # one allocation of eight floats, made with the first call, and its front two:
        self.split_sums = None              # the eight sums of the last split-aware call
        self.sums = None                    # (loss sum, correct count) of the last call without splits
        self.S: Optional[dn_matrix] = None
        self.counts = None                  # global row count of the slots train / val / test / other
        self.train_set = 0
        self._planar = False                # layout of split_sums after the last call, see __call__

    def set_splits(self, S: Optional[dn_matrix], counts=None, train_set: int = 0) -> None:
        """S: int32 [n x 1] on the device, the set of every row of the logits this layer sees (None switches the
        splits off); counts: the GLOBAL number of rows per slot (train, val, test, other) -- counted here from S when
        None, which is right on one GPU only; train_set: the set the gradient and the reported pair belong to."""
        if S is None:
            self.S, self.counts = None, None
            return
        if not isinstance(S, dn_matrix):
            raise ValueError("the sets must be an int32 dn_matrix of n rows and one column")
        _, self.counts = check_splits(S, S.n(), train_set, counts)
        self.S, self.train_set = S, int(train_set)

    def active_sums(self):
        """the sums the last call wrote: the eight of the splits when they are on, the two plain ones otherwise"""
        return self.sums if self.S is None else self.split_sums

    def __call__(self, ctx: context, H: dn_matrix, Y: dn_matrix, n_global: Optional[int] = None,
                 sync: bool = True):
        """One body for both forms.  With splits on, the gradient is scaled by 1 / (the global number of training rows)
        instead of 1 / n_global, rows outside train_set get a zero gradient row and eight sums are kept instead of two:
        (loss, correct) pairs slot by slot from the fused kernel, the four loss sums then the four correct counts
        (``_planar``) from the unfused chain."""
        torch = _torch()
        n = self.name
        split = self.S is not None
        if n_global is None:
            n_global = Y.n()
        if split and self.S.n() != H.n():
            raise ValueError(f"the sets have {self.S.n()} rows, the logits {H.n()}")
        rows = self.counts[self.train_set] if split else n_global      # what the gradient is averaged over
        if self.sums is None:
            self.split_sums = (host_scalars(8) if self.host_sums
                               else torch.empty(8, dtype=torch.float32, device=ctx.device))
            self.sums = self.split_sums[0:2]
        sums = self.active_sums()
        ctx.record(n + "0_loss-layer", 0)
        if self.fused and 1 <= H.m() <= ops.XENT_FUSED_MAX_CLASSES:
            if self.copy:                       # the reference copies, then works in place (gcn.hpp:653-656): here the
                if self.G is None or self.G.shape() != H.shape():   # pass reads the logits, writes the gradient elsewhere
                    self.G = dn_matrix(H.n(), H.m())
            else:
                self.G = H
            ctx.lib.mggcn_memset_zero(sums.data_ptr(), 4 * sums.numel(), ctx.stream(0))
            if split:
                ops.softmax_xent_split(ctx, H, Y, self.S, self.train_set, 1.0 / rows, sums, out=self.G)
            else:
                ops.softmax_xent_fused(ctx, H, Y, 1.0 / rows, sums, out=self.G)
            self._planar = False
        else:
            O = self.softmax_layer(ctx, H)
            if self.P is None:
                self.P = dn_matrix(Y.shape(), dtype=np.int32)
            ops.max_row_indices(ctx, O, self.P)
            if self.L is None:
                self.L = dn_matrix(Y.shape())
            ops.index_log_rows(ctx, O, Y, self.L)
            self.G = O
            ops.add_indexed_rows(ctx, self.G, Y, -1.0)
            ops.scale_mat(ctx, self.G, float(np.float32(1) / np.float32(rows)))
            if split:
                ops.select_rows_by_set(ctx, self.G, self.S, self.train_set)
            if self.T is None:
                self.T = dn_matrix(Y.shape())
            ops.is_equal(ctx, Y, self.P, self.T)
            if split:
                ops.abssum_by_set(ctx, self.L, self.S, sums[0:4])
                ops.abssum_by_set(ctx, self.T, self.S, sums[4:8])
            else:
                ops.abssum(ctx, self.L, sums[0:1])
                ops.abssum(ctx, self.T, sums[1:2])
            self._planar = True
        ctx.record(n + "1_loss-layer", 0)
        ctx.register_timer(n + "loss-layer", n + "0_loss-layer", n + "1_loss-layer")
        self._n = H.n()
        if not sync:
            return None
        ctx.sync()
        return self.read(ctx)

    def split_sums_host(self, sums=None) -> np.ndarray:
        """the eight sums of the last call as (loss sum, correct count) pairs of train / val / test / other; ``sums``:
        eight floats in the layout of the last call (the distributed wrapper passes the all-reduced ones)"""
        if sums is None:
            sums = self.split_sums.numpy() if self.host_sums else self.split_sums.cpu().numpy()
        s = np.asarray(sums, dtype=np.float32).reshape(-1)[:8]
        return s.reshape(2, 4).T.reshape(-1).copy() if self._planar else s.copy()

    def split_metrics(self, sums=None):
        """{"train": (loss, acc), "val": ..., "test": ..., "other": ..., "counts": {...}} of the last call (after the
        caller's synchronisation); a split without a row reports nan"""
        s = self.split_sums_host(sums)
        out = {}
        for k, name in enumerate(ops.SPLIT_NAMES):
            c = self.counts[k]
            out[name] = ((float(s[2 * k] / np.float32(c)), float(s[2 * k + 1] / np.float32(c))) if c
                         else (float("nan"), float("nan")))
        out["counts"] = dict(zip(ops.SPLIT_NAMES, self.counts))
        return out

    def read(self, ctx: context, sums=None, n: Optional[int] = None):
        """(loss, acc) of the last call; the caller has synchronised (train_step reads after the
        whole epoch is done instead of blocking between forward and backward).  ``sums``: the host floats to read them
        from, in the layout of the last call, and ``n``: the rows they were summed over (the distributed wrapper passes the
        all-reduced sums and the global row count; None: this layer's own)."""
        if self.S is not None:
            return self.split_metrics(sums)[ops.SPLIT_NAMES[self.train_set]]
        if sums is None:
            sums = self.sums.numpy() if self.host_sums else self.sums.cpu().numpy()
        n = np.float32(self._n if n is None else n)
        return float(np.float32(sums[0]) / n), float(np.float32(sums[1]) / n)

    def backward(self) -> dn_matrix:
        return self.G


LOSSES = ("softmax", "bce")


def check_loss(loss: str) -> str:
    """the ``loss=`` option of gcn / dist_gcn: "softmax" (one class per vertex, the reference's) or "bce" (multi-label)"""
    if loss not in LOSSES:
        raise ValueError(f"loss must be one of {LOSSES}, got {loss!r}")
    return loss


def check_targets(loss: str, Y, n: int, width: int) -> None:
    """loss="bce": the targets are an int32 dn_matrix of n x width (one column per logit); before any launch"""
    if loss != "bce":
        return
    if not isinstance(Y, dn_matrix) or Y.t.dtype != _torch().int32 or Y.shape() != (n, width):
        got = f"{Y.t.dtype} of {Y.shape()}" if isinstance(Y, dn_matrix) else type(Y).__name__
        raise ValueError(f"loss='bce' needs int32 targets of {n} x {width} (one column per logit), got {got}")


def micro_f1(tp: float, fp: float, fn: float) -> float:
    """2 TP / (2 TP + FP + FN); nan when nothing is positive and nothing was predicted positive"""
    den = 2.0 * tp + fp + fn
    return float(2.0 * tp / den) if den else float("nan")


class sigmoid_bce_loss:
    """The multi-label loss (opt-in, ``loss="bce"``; the reference has none): every logit is a binary task of its own,
    the loss is sigmoid + binary cross-entropy averaged over rows AND columns, the score is micro-F1 with ``z > 0`` as
    the prediction.  The interface of softmax_cross_entropy_loss; ``Y`` is the int32 [n x m] target matrix (non-zero =
    positive) and (loss, micro-F1) comes back where that layer returns (loss, acc).  One kernel (ops.sigmoid_bce) makes
    the pass: there is no unfused chain to mirror, so ``fused`` is accepted and ignored.  copy=True writes the gradient
    to a second matrix, copy=False works in place.

    Sixteen sums are kept, (loss sum, TP, FP, FN) per slot train / val / test / other; without splits every row is in
    slot 0 and the front four are the active ones."""

    def __init__(self, name: str, copy: bool = True, fused: bool = False, host_sums: bool = True):
        self.name = name
        self.copy, self.fused, self.host_sums = copy, fused, host_sums
        self.G = None
        self.split_sums = None              # the sixteen sums of the last call
        self.sums = None                    # its front four: (loss sum, TP, FP, FN) of a call without splits
        self.S: Optional[dn_matrix] = None
        self.counts = None
        self.train_set = 0
        self._n = self._m = 0

    def set_splits(self, S: Optional[dn_matrix], counts=None, train_set: int = 0) -> None:
        """see softmax_cross_entropy_loss.set_splits"""
        if S is None:
            self.S, self.counts = None, None
            return
        if not isinstance(S, dn_matrix):
            raise ValueError("the sets must be an int32 dn_matrix of n rows and one column")
        _, self.counts = check_splits(S, S.n(), train_set, counts)
        self.S, self.train_set = S, int(train_set)

    def active_sums(self):
        """the sums the last call wrote: all sixteen when the splits are on, the four of slot 0 otherwise"""
        return self.sums if self.S is None else self.split_sums

    def __call__(self, ctx: context, H: dn_matrix, Y: dn_matrix, n_global: Optional[int] = None,
                 sync: bool = True):
        torch = _torch()
        n = self.name
        check_targets("bce", Y, H.n(), H.m())
        split = self.S is not None
        if n_global is None:
            n_global = Y.n()
        if split and self.S.n() != H.n():
            raise ValueError(f"the sets have {self.S.n()} rows, the logits {H.n()}")
        rows = self.counts[self.train_set] if split else n_global      # what the gradient is averaged over, times m
        if self.sums is None:
            self.split_sums = (host_scalars(ops.BCE_SUMS) if self.host_sums
                               else torch.empty(ops.BCE_SUMS, dtype=torch.float32, device=ctx.device))
            self.sums = self.split_sums[0:4]
        ctx.record(n + "0_loss-layer", 0)
        if self.copy:
            if self.G is None or self.G.shape() != H.shape():
                self.G = dn_matrix(H.n(), H.m())
        else:
            self.G = H
        # all sixteen are zeroed and written (the kernel's final pass adds sixteen): the four of slot 0 are read without splits
        ctx.lib.mggcn_memset_zero(self.split_sums.data_ptr(), 4 * ops.BCE_SUMS, ctx.stream(0))
        ops.sigmoid_bce(ctx, H, Y, self.S, self.train_set, 1.0 / (float(rows) * H.m()), self.split_sums, out=self.G)
        ctx.record(n + "1_loss-layer", 0)
        ctx.register_timer(n + "loss-layer", n + "0_loss-layer", n + "1_loss-layer")
        self._n, self._m = H.n(), H.m()
        if not sync:
            return None
        ctx.sync()
        return self.read(ctx)

    def _host(self, sums, k: int) -> np.ndarray:
        if sums is None:
            t = self.split_sums if k == ops.BCE_SUMS else self.sums
            sums = t.numpy() if self.host_sums else t.cpu().numpy()
        return np.asarray(sums, dtype=np.float32).reshape(-1)[:k].copy()

    def split_metrics(self, sums=None):
        """{"train": (loss, micro_f1), "val": ..., "test": ..., "other": ..., "counts": {...}, "confusion": {"train":
        (tp, fp, fn), ...}} of the last call (after the caller's synchronisation); a split without a row reports a nan
        loss, one without a positive target or prediction a nan F1"""
        s = self._host(sums, ops.BCE_SUMS)
        out, conf = {}, {}
        for k, name in enumerate(ops.SPLIT_NAMES):
            c = self.counts[k]
            tp, fp, fn = (float(v) for v in s[4 * k + 1:4 * k + 4])
            conf[name] = (tp, fp, fn)
            out[name] = ((float(s[4 * k]) / (float(c) * self._m), micro_f1(tp, fp, fn)) if c
                         else (float("nan"), float("nan")))
        out["counts"] = dict(zip(ops.SPLIT_NAMES, self.counts))
        out["confusion"] = conf
        return out

    def confusion(self, sums=None):
        """(tp, fp, fn) behind the micro-F1 that read() reports: train_set's with splits, every row's without"""
        if self.S is not None:
            return self.split_metrics(sums)["confusion"][ops.SPLIT_NAMES[self.train_set]]
        return tuple(float(v) for v in self._host(sums, 4)[1:4])

    def read(self, ctx: context, sums=None, n: Optional[int] = None):
        """(loss, micro_f1) of the last call; the caller has synchronised.  ``sums`` / ``n``: see
        softmax_cross_entropy_loss.read"""
        if self.S is not None:
            return self.split_metrics(sums)[ops.SPLIT_NAMES[self.train_set]]
        s = self._host(sums, 4)
        n = self._n if n is None else n
        return float(s[0]) / (float(n) * self._m), micro_f1(float(s[1]), float(s[2]), float(s[3]))

    def backward(self) -> dn_matrix:
        return self.G


def split_counts(S: np.ndarray) -> List[int]:
    """rows per slot (train, val, test, other) of a host array of set values"""
    s = np.asarray(S).reshape(-1)
    c = [int((s == k).sum()) for k in range(3)]
    return c + [int(s.size) - sum(c)]


def check_sets(S, n: int, train_set: int) -> np.ndarray:
    """train_set is one of 0 / 1 / 2 and S a numpy array of n integers or an int32 dn_matrix of n x 1; returns the sets as
    a host int32 [n x 1] array"""
    if train_set not in ops.TRAIN_SETS:
        raise ValueError(f"train_set must be one of {ops.TRAIN_SETS}, got {train_set!r}")
    if isinstance(S, dn_matrix):
        if S.t.dtype != _torch().int32 or S.shape() != (n, 1):
            raise ValueError(f"the sets must be an int32 dn_matrix of {n} x 1, got {S.t.dtype} of {S.shape()}")
        return S.numpy()
    host = np.asarray(S)
    if host.dtype.kind not in "iu" or host.size != n or host.ndim > 2 or (host.ndim == 2 and host.shape[1] != 1):
        raise ValueError(f"the sets must be {n} integers, got {host.dtype} of shape {host.shape}")
    return np.ascontiguousarray(host.reshape(n, 1).astype(np.int32))


def check_counts(counts, train_set: int) -> List[int]:
    """four global row counts (train, val, test, other) of which train_set's is not zero"""
    counts = [int(c) for c in counts]
    if len(counts) != 4 or min(counts) < 0:
        raise ValueError("counts: the global number of rows of train, val, test and other")
    if counts[train_set] == 0:
        raise ValueError(f"no vertex belongs to set {train_set}: nothing to train on")
    return counts


def check_splits(S, n: int, train_set: int, counts=None):
    """Option checking of set_splits, before any device work: check_sets, and at least one row trains (``counts``: the
    global counts of a row partition; None counts S).  Returns (the sets as a host int32 [n x 1] array, the counts)."""
    host = check_sets(S, n, train_set)
    return host, check_counts(split_counts(host) if counts is None else counts, train_set)


def evaluate_micro_f1(logits: np.ndarray, targets: np.ndarray, sets: Optional[np.ndarray] = None):
    """{"all": micro-F1 over every row, "train" / "val" / "test": over the rows of that set} from host logits and targets"""
    pred, pos = np.asarray(logits) > 0, np.asarray(targets) != 0

    def f1(rows):
        p, t = pred[rows], pos[rows]
        return micro_f1(float((p & t).sum()), float((p & ~t).sum()), float((~p & t).sum()))

    res = {"all": f1(slice(None))}
    if sets is not None:
        s = np.asarray(sets).reshape(-1)
        for k, name in enumerate(ops.SPLIT_NAMES[:3]):
            res[name] = f1(s == k)
    return res


def link_fused_backward(layers, fused: bool) -> None:
    """fused backward: layer i+1's G_out GEMM applies layer i's leaky_relu' -- possible when layer i+1 is
    GEMM-first (its G_out comes out of a GEMM, gcn.hpp:479-481) and propagates a gradient at all"""
    for lo, hi in zip(layers[:-1], layers[1:]):
        ok = bool(fused) and lo.activation and hi.gemm_first() and hi.lin.backward_out
        # a residual branch needs the UNMASKED incoming gradient (gcn.hpp:484-487) and adds to G_out afterwards
        ok = ok and not getattr(lo, "residual_layer", False) and not getattr(hi, "residual_layer", False)
        hi.mask_input_grad = lo.grad_premasked = ok


def adam_update_all(ctx: context, lins, state, lr: float, beta1: float, beta2: float, weight_decay: float, eps: float):
    """ONE launch for every parameter tensor of the model (linear::adam_update of every layer, gcn.hpp:146-172
    and :990-994).  ``state`` = (weight_decay, ops.adam_table) from the previous call or None."""
    for lin in lins:
        lin.adam_state(ctx)
        lin.step += 1
    if state is None or state[0] != weight_decay:
        tensors = [t for lin in lins for t in lin.adam_tensors(weight_decay)]
        state = (weight_decay, ops.adam_table(ctx, tensors))
    step = lins[0].step
    assert all(lin.step == step for lin in lins)
    bc1 = float(np.float32(1 - beta1 ** step))
    bc2 = float(np.float32(1 - beta2 ** step))
    ctx.record("0_adam-update", 0)
    state[1].step(ctx, lr, beta1, beta2, bc1, bc2, eps)
    ctx.record("1_adam-update", 0)
    ctx.register_timer("adam-update", "0_adam-update", "1_adam-update")
    return state


class model_base(dropout_option, checkpoint_option):
    """The epoch of a single-GPU model, whatever its layers are (gcn, gat.gat): splits, the forward pass, the loss,
    backward, Adam and evaluate, over what the constructor of the model sets -- ``loss_layer``, ``layers_``, ``loss``,
    ``A``, ``_out_width``, ``fused`` and ``_adam`` (None).  A layer is called with (ctx, H), has backward(ctx, G),
    adam_update and params() (layer_params), and takes its ``dropout`` from _arm_dropout."""

    def set_splits(self, S, train_set: int = 0) -> None:
        """Train on one split (opt-in; the reference loads sets.bin and ignores it, src/main.cpp:85).  S: the set of every
        vertex (0 train / 1 validation / 2 test, anything else belongs to no split) as a numpy array of n integers or an
        int32 dn_matrix of n rows; None restores the loss over all vertices.  From here on train_forward / train_step
        return the loss and accuracy of ``train_set`` and split_metrics() reports every split of the last epoch."""
        if S is None:
            self.loss_layer.set_splits(None)
            return
        host, counts = check_splits(S, self.A.n(), train_set)
        if not isinstance(S, dn_matrix):
            S = dn_matrix.from_numpy(host)
        self.loss_layer.set_splits(S, counts, train_set)

    def split_metrics(self):
        """every split's (loss, acc) of the last epoch, see softmax_cross_entropy_loss.split_metrics; call after
        train_forward / train_step (they synchronise).  With dropout on these are the numbers of the DROPPED training
        forward, validation and test included: evaluate() gives the clean ones."""
        if self.loss_layer.S is None:
            raise ValueError("split_metrics() needs set_splits(S) first")
        return self.loss_layer.split_metrics()

    def __call__(self, ctx: context, H: dn_matrix, training: bool = False) -> dn_matrix:
        """the forward pass; ``training``: a training forward (train_forward / train_step pass True), the only kind
        that drops -- a plain call and evaluate() never do"""
        self._arm_dropout(training)
        for layer in self.layers_:
            H = layer(ctx, H)
        return H

    def train_forward(self, ctx: context, H: dn_matrix, Y: dn_matrix):
        check_targets(self.loss, Y, self.A.n(), self._out_width)
        H = self(ctx, H, training=True)
        return self.loss_layer(ctx, H, Y)

    def backward(self, ctx: context) -> None:
        G = self.loss_layer.backward()
        for layer in reversed(self.layers_):
            G = layer.backward(ctx, G)

    def train_step(self, ctx: context, H: dn_matrix, Y: dn_matrix, lr: float, beta1: float, beta2: float,
                   weight_decay: float, eps: float):
        """One epoch = the reference's loop body (src/main.cpp:122-129: train_forward, backward,
        adam_update, sync) with ONE host synchronisation: the loss / accuracy scalars are read after
        the epoch's last kernel instead of between forward and backward (the reference blocks inside
        its loss layer, src/gcn.hpp:816-817, and leaves the GPU idle while the host catches up)."""
        check_targets(self.loss, Y, self.A.n(), self._out_width)
        out = self(ctx, H, training=True)
        self.loss_layer(ctx, out, Y, sync=False)
        self.backward(ctx)
        self.adam_update(ctx, lr, beta1, beta2, weight_decay, eps)
        self._launched()
        ctx.sync()
        return self.loss_layer.read(ctx)

    def _launched(self) -> None:
        """hook: train_step has enqueued the whole epoch and is about to wait for it -- host work that can run under the
        device's goes here (gat: the next epoch's label-input count).  Nothing by default."""

    def adam_update(self, ctx: context, lr: float, beta1: float, beta2: float, weight_decay: float,
                    eps: float) -> None:
        if not self.fused:
            for layer in self.layers_:
                layer.adam_update(ctx, lr, beta1, beta2, weight_decay, eps)
            return
        self._adam = adam_update_all(ctx, [p for l in self.layers_ for p in l.params()], self._adam, lr, beta1,
                                     beta2, weight_decay, eps)

    def layers(self):
        return self.layers_

    def evaluate(self, ctx: context, H: dn_matrix, Y: dn_matrix, S: Optional[dn_matrix] = None):
        """Forward pass + accuracy per split.  The reference loads
        sets.bin (0 train / 1 val / 2 test, test/data/prep.py:115-118) and never uses it
        (src/main.cpp:85); its reported accuracy is over ALL vertices, which is what
        ``result["all"]`` repeats.  Device work: the model's forward kernels + the argmax
        kernel; the per-split counting is a host reduction over n integers.

        With loss="bce" the numbers are micro-F1 instead of accuracy (prediction: logit > 0), a host reduction over the
        copied logits."""
        if self.loss == "bce":
            check_targets(self.loss, Y, self.A.n(), self._out_width)
            out = self(ctx, H)
            ctx.sync()
            return evaluate_micro_f1(out.numpy(), Y.numpy(), None if S is None else S.numpy())
        out = self(ctx, H)
        P = dn_matrix(Y.shape(), dtype=np.int32)
        ops.max_row_indices(ctx, out, P)
        ctx.sync()
        pred, y = P.numpy().reshape(-1), Y.numpy().reshape(-1)
        hit = pred == y
        res = {"all": float(hit.mean())}
        if S is not None:
            s = S.numpy().reshape(-1)
            for k, name in enumerate(ops.SPLIT_NAMES[:3]):
                m = s == k
                res[name] = float(hit[m].mean()) if m.any() else float("nan")
        return res

    _roc_auc_evaluator = None

    def roc_auc(self, ctx: context, H: dn_matrix, Y: dn_matrix, S=None, max_workspace_bytes: Optional[int] = None):
        """ROC-AUC per class and split of a loss="bce" model, computed on the device (metrics.roc_auc_evaluator: what it
        returns; ogbn-proteins' score is result["test"] / ["val"]).  One plain forward on the full graph -- no dropout, no
        sampling, no label mask beyond what a plain call does; no dropout or sample epoch is spent --, then keys, one stable
        sort per class and the integer statistic; the logits are never copied to the host.  S: the sets (an int32 dn_matrix
        of n x 1 or n integers); None uses those of set_splits when there are any, else every row is in slot "train".  The
        evaluator is created with the first call and kept (``max_workspace_bytes``: its cap, read then).  ValueError before
        any device work: a model whose loss is not "bce", targets that fail check_targets, an S of the wrong shape,
        n >= 2^31."""
        from . import metrics
        S = metrics.model_roc_auc_checks(self, Y, S)
        if self._roc_auc_evaluator is None:
            kw = {} if max_workspace_bytes is None else dict(max_workspace_bytes=max_workspace_bytes)
            self._roc_auc_evaluator = metrics.roc_auc_evaluator(self.A.n(), self._out_width, **kw)
        return self._roc_auc_evaluator(ctx, self(ctx, H), Y, S)


class gcn(rescaled_sampling_option, model_base):
    """reference src/gcn.hpp:937-995.  The constructor column-normalises A, builds
    A_T and hands (A_T, A) to the layers -- forward multiplies by A_T (:946-955).

    ``dropout=p`` / set_dropout(p, seed, epoch): see dropout_option -- the input of every layer but the first is dropped
    in train_forward / train_step; the features X are the caller's buffer and are not dropped.

    ``norm="layer"``: every layer but the last normalises its rows between aggregation / linear and activation (see
    layer_norm; ``layer.norm.gamma`` / ``.beta``, ``layer.norm.init(gamma, beta)``).  It has no training mode: a plain
    call and evaluate() run the same kernels.  None (the default) launches nothing new.

    save(ctx, path, optimizer=True) / load(ctx, path) / predict(ctx, X): see checkpoint.checkpoint_option -- the file
    carries the configuration, the parameters, Adam's state and the dropout state, and no execution option.

    ``fanout`` / ``edge_keep`` / ``edge_rescale`` / set_sampling(fanout, keep, seed, epoch, rescale): per-epoch edge sampling
    (edge_sample.py).  gcn is a weighted sum, so it samples only when told how the kept values are rescaled: with
    ``edge_rescale`` None (the default) any setting that is on is refused with ValueError naming the argument; "row" keeps every
    row sum (the mean over the sampled neighbours on the row-stochastic matrix built here), "inverse" divides by the keep
    probability.  A training forward then multiplies, forward and backward, by the pair of the epoch through the row-split SpMM
    on a plan built on the device (sparse_linear.sample, ops.spmm_dev); every other forward runs on the full graph with the
    bits it has without sampling.  hoist_first_aggregation does not compose: the hoisted product belongs to the full graph."""

    def __init__(self, A: csr_matrix, sizes: Sequence[int], residual_layer: bool = False,
                 weights: Optional[List[Tuple[np.ndarray, np.ndarray]]] = None, fused: bool = True,
                 hoist_first_aggregation: bool = False, agg_dtype: str = "f32", dropout: float = 0.0, norm=None,
                 loss: str = "softmax", fanout=None, edge_keep: float = 1.0, edge_rescale=None):
        self.hoist_first_aggregation = bool(hoist_first_aggregation)
        self._init_sampling(fanout, edge_keep, edge_rescale)     # option checks come before any device work
        self._init_dropout(dropout, len(sizes) - 1)
        self.norm = check_norm(norm)
        self.loss = check_loss(loss)
        self._out_width = int(sizes[-1])
        self.sizes, self.residual_layer = [int(s) for s in sizes], bool(residual_layer)      # the checkpoint's configuration
        torch = _torch()
        self.agg_dtype = _check_agg_dtype(agg_dtype)
        if self.agg_dtype != "f32" and hoist_first_aggregation:
            raise ValueError("hoist_first_aggregation is fp32-only: with agg_dtype='bf16' the hoisted product would "
                             "round X instead of X W")
        self.fused = fused
        loss_class = sigmoid_bce_loss if self.loss == "bce" else softmax_cross_entropy_loss
        self.loss_layer = loss_class(f"{len(sizes) - 1}_", residual_layer, fused)
        A.normalize(True)
        A_T = A.transpose()
        self.A, self.A_T = A, A_T
        max_d = max(min(sizes[i], sizes[i + 1]) for i in range(len(sizes) - 1))
        self.HW_buffer = torch.empty(max(A.n(), A.m()) * max_d, dtype=torch.float32, device="cuda")
        # bf16 aggregation: every SpMM's dense operand is rounded into this one scratch (n x the widest SpMM width)
        self.agg_buffer = (torch.empty(max(A.n(), A.m()) * max_d, dtype=torch.bfloat16, device="cuda")
                           if self.agg_dtype == "bf16" else None)
        self.layers_: List[gcn_layer] = []
        for i in range(1, len(sizes)):
            self.layers_.append(gcn_layer(f"{i - 1}_", A_T, A, sizes[i - 1], sizes[i], i + 1 < len(sizes),
                                          residual_layer, i != 1, self.HW_buffer, fused, self.agg_dtype,
                                          self.agg_buffer, self.norm))
        link_fused_backward(self.layers_, fused)
        self._adam = None
        self.set_hoist_first_aggregation(hoist_first_aggregation)
        self._sample_max_d = int(max_d)
        self._sample_matrices = (A_T, A)
        if sampling_on(self.sample_fanout, self.sample_keep):
            self._make_sampler(A_T, A)                           # forward multiplies by A_T: its rows are the destinations
        self._plan_wants = []                        # (matrix, max_d, width): built side by side on first use (prebuild_plans)
        for i in range(1, len(sizes)):
            w = min(sizes[i - 1], sizes[i])
            self._plan_wants.append((A_T, max(w, 128), w))           # forward multiplies by A_T (gcn.hpp:954)
            if i != 1:
                self._plan_wants.append((A, max(w, 128), w))         # the first layer's backward SpMM is skipped
        if weights is not None:                     # test constructor, gcn.hpp:957-963
            assert len(weights) == len(self.layers_)
            for layer, (W, b) in zip(self.layers_, weights):
                layer.W().init(np.asarray(W, dtype=np.float32))
                layer.b().init(np.asarray(b, dtype=np.float32))

    def set_hoist_first_aggregation(self, on: bool) -> None:
        """Pre-compute the first layer's aggregation A_fwd . X once (see gcn_layer.__call__): valid while the SAME
        feature matrix is passed every epoch (full-graph training does) and only for a GEMM-first first layer without a
        residual branch; 6 instead of 7 SpMMs per epoch on the Reddit model.  Off = the reference's epoch."""
        if on and self.agg_dtype != "f32":
            raise ValueError("hoist_first_aggregation is fp32-only: with agg_dtype='bf16' the hoisted product would "
                             "round X instead of X W")
        if on and sampling_on(self.sample_fanout, self.sample_keep):
            raise ValueError("hoist_first_aggregation does not compose with edge sampling (fanout / edge_keep / set_sampling): "
                             "the hoisted product belongs to the full graph")
        self.hoist_first_aggregation = bool(on)
        l0 = self.layers_[0]
        # A_fwd (1 b^T) = 1 b^T needs EVERY row of A_fwd to sum to one: a vertex without a single entry in its row of
        # A_fwd (no self-loop, nobody points at it) has row sum 0 and would get 0 instead of b -- the reference's data-prep
        # adds self-loops (test/data/prep.py:113), but the engine does not assume it: such a graph keeps the plain path
        fwd = l0.A.A
        stochastic = bool(np.all(np.diff(fwd.indptr.astype(np.int64)) > 0)) if fwd.n() else True
        l0.hoist_input = bool(on) and l0.gemm_first() and not l0.residual_layer and stochastic
        l0._AX = l0._AX_key = None                  # (re-)enabling recomputes the product: the way to pick up an in-place change of X

    def __call__(self, ctx: context, H: dn_matrix, training: bool = False) -> dn_matrix:
        if self._plan_wants:                          # first call: the context (device) is known now
            ops.prebuild_plans(ctx, self._plan_wants)
            self._plan_wants = []
        if self.sampler is not None or self.layers_[0].A.sample is not None:
            pair = self._draw_sample(ctx, training)          # one sample per epoch, shared by all layers; None: the full graph
            for layer in self.layers_:
                layer.A.sample = pair
        return model_base.__call__(self, ctx, H, training)

    hoist_first_aggregation = False

    def _refuse_sampling(self, fanout, keep) -> None:
        if self._rescale_checked() is None:
            refuse_sampling("gcn", fanout, keep)
        if self.hoist_first_aggregation:
            raise ValueError("gcn(hoist_first_aggregation=True) has no edge sampling (fanout / edge_keep / set_sampling): the "
                             "hoisted product belongs to the full graph")

    def update(self, ctx: context, lr: float, weight_decay: float) -> None:
        for layer in self.layers_:
            layer.update(ctx, lr, weight_decay)
