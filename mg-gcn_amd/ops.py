"""The reference's operator overload set (src/cuda_utils.hpp) over the C ABI.

Same function names, argument order and meaning as the reference's free
functions taking ``(context, matrix objects...)``; each one enqueues exactly one
C-ABI call on ``ctx.cuda_streams[0]`` (the reference's compute stream).
Shape preconditions the reference only ``assert``s raise ``ValueError`` here.
"""
from __future__ import annotations

import math
import numbers
import os

from typing import Optional

import numpy as np

from .matrix import context, csr_matrix, dn_matrix


def _req(cond: bool, what: str) -> None:
    if not cond:
        raise ValueError(what)


class spmm_buffer:
    """What get_matmul_buffer returns: the reference's opaque cuSPARSE workspace
    (src/cuda_utils.hpp:94-102) becomes the row-split plan of the HIP kernel."""

    def __init__(self, lib, handle: int):
        self.lib, self.handle = lib, handle
        self.max_d = 0
        self.d_hint = 0
        self.version = 0            # csr_matrix._version the plan was built from

    def num_items(self) -> int: return self.lib.mggcn_spmm_plan_num_items(self.handle)
    def num_split_rows(self) -> int: return self.lib.mggcn_spmm_plan_num_split_rows(self.handle)
    def num_sweep_tasks(self) -> int: return self.lib.mggcn_spmm_plan_num_sweep_tasks(self.handle)
    def num_launches(self, d: int) -> int: return self.lib.mggcn_spmm_plan_num_launches(self.handle, int(d))
    def nbytes(self) -> int: return self.lib.mggcn_spmm_plan_bytes(self.handle)

    def describe(self) -> str:
        """what the plan builder measured and decided (mggcn_spmm_plan_describe)"""
        import ctypes
        buf = ctypes.create_string_buffer(4096)
        self.lib.mggcn_spmm_plan_describe(self.handle, buf, 4096)
        return buf.value.decode()

    def __del__(self):
        try:
            if self.handle:
                self.lib.mggcn_spmm_plan_destroy(self.handle)
                self.handle = 0
        except Exception:
            pass


def get_matmul_buffer(ctx: context, A: csr_matrix, B: dn_matrix, C: dn_matrix, alpha: float = 1.0,
                      beta: float = 0.0, max_d: Optional[int] = None) -> spmm_buffer:
    """reference src/cuda_utils.hpp:94-102"""
    _req(A.m() == B.n(), "A.m() != B.n()")
    _req(A.n() == C.n() and B.m() == C.m(), "C shape mismatch")
    return spmm_plan_for(ctx, A, max(int(max_d or 0), B.m()), B.m())


def spmm_plan_for(ctx: context, A: csr_matrix, max_d: int, d_hint: int) -> spmm_buffer:
    """One plan per (matrix, device, form): the layers of a model multiply by the same two matrices,
    so the plan (0.9 GB and ~1 s of host work on the Reddit shape) is built once and shared.  The
    form depends on the width only through narrow (<= 64: lanes per row) vs wide."""
    form = ("narrow", (int(d_hint) + 15) // 16) if 1 <= int(d_hint) <= 64 else ("wide", 0)
    knobs = tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith("MGGCN_SPMM_")))   # tuning / tests
    key = (ctx.rank, form, knobs)
    cache = A.__dict__.setdefault("_spmm_plans", {})
    buf = cache.get(key)
    if buf is None or buf.max_d < max_d:
        ctx.set()
        h = ctx.lib.mggcn_spmm_plan_create_for(A.n(), A.m(), A.indptr.ctypes.data, A.indices.ctypes.data,
                                               A.data.ctypes.data, int(max_d), int(d_hint))
        buf = cache[key] = spmm_buffer(ctx.lib, h)
        buf.max_d, buf.d_hint, buf.version = int(max_d), int(d_hint), A._version
    return buf


def prebuild_plans(ctx: context, wants, max_parallel: int = 4) -> None:
    """wants = [(csr_matrix, max_d, d_hint), ...]: the plans a model is going to ask for, built SIDE BY SIDE (up to
    four host threads; ctypes releases the GIL and every plan builder threads its own passes) and filed in the
    matrices' caches, instead of one by one inside the first epoch: a single-GPU model multiplies by two matrices at
    two widths -- four plans of 0.4-1.0 s of host work each at the Reddit shape, 2.9 s in a row."""
    from concurrent.futures import ThreadPoolExecutor
    knobs = tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith("MGGCN_SPMM_")))
    jobs = {}
    for A, max_d, d_hint in wants:
        form = ("narrow", (int(d_hint) + 15) // 16) if 1 <= int(d_hint) <= 64 else ("wide", 0)
        key = (ctx.rank, form, knobs)
        have = A.__dict__.setdefault("_spmm_plans", {}).get(key)
        if have is not None and have.max_d >= max_d:
            continue
        jk = (id(A), key)
        if jk not in jobs or jobs[jk][1] < max_d:
            jobs[jk] = (A, int(max_d), int(d_hint), key)
    if not jobs:
        return

    def build(job):
        A, max_d, d_hint, _ = job
        ctx.lib.mggcn_set_device(ctx.rank)
        return ctx.lib.mggcn_spmm_plan_create_for(A.n(), A.m(), A.indptr.ctypes.data, A.indices.ctypes.data,
                                                  A.data.ctypes.data, max_d, d_hint)
    todo = list(jobs.values())
    workers = max(1, min(max_parallel, len(todo)))
    ctx.lib.mggcn_spmm_plan_concurrent_builders(workers)        # every builder threads over its share of the cores
    try:
        with ThreadPoolExecutor(max_workers=workers) as pool:
            handles = list(pool.map(build, todo))
    finally:
        ctx.lib.mggcn_spmm_plan_concurrent_builders(1)
    for (A, max_d, d_hint, key), h in zip(todo, handles):
        buf = A.__dict__["_spmm_plans"][key] = spmm_buffer(ctx.lib, h)
        buf.max_d, buf.d_hint, buf.version = max_d, d_hint, A._version


def matmul(ctx: context, A, B: dn_matrix, C: dn_matrix, *args, **kw) -> None:
    """Overloads, as in the reference:
       matmul(ctx, csr A, B, C, ext_buffer, alpha, beta)        src/cuda_utils.hpp:27-32
       matmul(ctx, dn  A, B, C, alpha, beta, A_T=False, B_T=False)  src/cuda_utils.hpp:158-172"""
    if isinstance(A, csr_matrix):
        return _spmm(ctx, A, B, C, *args, **kw)
    return _gemm(ctx, A, B, C, *args, **kw)


def _current_plan(ctx: context, A: csr_matrix, ext_buffer: Optional[spmm_buffer], d: int) -> Optional[spmm_buffer]:
    if ext_buffer is not None and ext_buffer.version != A._version:
        # the matrix was edited in place after the plan was built (csr_matrix.normalize / invalidate): the
        # reference's cuSPARSE workspace holds no values, so the same call sequence must keep working
        ext_buffer = spmm_plan_for(ctx, A, ext_buffer.max_d, ext_buffer.d_hint or d)
    return ext_buffer


def _spmm(ctx: context, A: csr_matrix, B: dn_matrix, C: dn_matrix, ext_buffer: Optional[spmm_buffer],
          alpha: float, beta: float, flags: int = 0, slope: float = 0.01, stream_id: int = 0) -> None:
    _req(A.m() == B.n() and B.m() == C.m() and A.n() == C.n(), "SpMM shape mismatch")
    ctx.set()
    ext_buffer = _current_plan(ctx, A, ext_buffer, B.m())
    ip, ix, dv = A.device(ctx.device)
    ctx.lib.mggcn_spmm_csr_f32(ctx.stream(stream_id), ext_buffer.handle if ext_buffer else None, A.n(), A.m(),
                               ip.data_ptr(), ix.data_ptr(), dv.data_ptr(), B.buffer(), B.m(), C.buffer(),
                               C.m(), B.m(), alpha, beta, flags, slope)


def _bf16_view(t, what: str):
    """(data pointer, rows, columns, leading dimension in elements) of a 2-D device tensor of 2-byte elements
    (torch.bfloat16, or int16 / uint16 holding bf16 bit patterns) with unit column stride"""
    _req(t.dim() == 2 and t.element_size() == 2 and t.is_cuda, f"{what}: a 2-D device tensor of bf16 (2-byte) elements")
    _req(t.stride(1) == 1 or t.shape[1] <= 1, f"{what}: columns must be contiguous")
    return t.data_ptr(), int(t.shape[0]), int(t.shape[1]), int(max(t.stride(0), t.shape[1]))


def convert_bf16(ctx: context, src, dst, stream_id: int = 0) -> None:
    """dst = bf16(src), rounded to nearest even (NaN stays NaN, overflow -> inf): mggcn_convert_f32_bf16.
    src: a dn_matrix or a 2-D fp32 device tensor (unit column stride); dst: a 2-D bf16 device tensor of the same shape,
    any row stride (see _bf16_view)."""
    if isinstance(src, dn_matrix):
        s_ptr, n, m, ld_s = src.buffer(), src.n(), src.m(), src.m()
    else:
        _req(src.dim() == 2 and src.element_size() == 4 and src.is_cuda and (src.stride(1) == 1 or src.shape[1] <= 1),
             "convert_bf16: src must be a dn_matrix or a 2-D fp32 device tensor")
        s_ptr, n, m, ld_s = src.data_ptr(), int(src.shape[0]), int(src.shape[1]), int(max(src.stride(0), src.shape[1]))
    d_ptr, dn, dm, ld_d = _bf16_view(dst, "convert_bf16 dst")
    _req((dn, dm) == (n, m), "convert_bf16: shape mismatch")
    ctx.set()
    ctx.lib.mggcn_convert_f32_bf16(ctx.stream(stream_id), s_ptr, ld_s, d_ptr, ld_d, n, m)


def spmm_bf16(ctx: context, A: csr_matrix, B16, C: dn_matrix, ext_buffer: Optional[spmm_buffer] = None,
              alpha: float = 1.0, beta: float = 0.0, flags: int = 0, slope: float = 0.01, stream_id: int = 0) -> None:
    """C = alpha A widen(B16) + beta C with B stored in bf16 (mggcn_spmm_csr_bf16): the products and sums are fp32 and
    equal those of matmul(ctx, A, widen(B16), C, ext_buffer, ...) bit for bit.  B16: 2-D bf16 device tensor of
    A.m() x C.m() (any row stride, see _bf16_view); ext_buffer: the same plans the fp32 SpMM uses."""
    b_ptr, bn, bm, ldb = _bf16_view(B16, "spmm_bf16 B")
    _req(A.m() == bn and bm == C.m() and A.n() == C.n(), "SpMM shape mismatch")
    ctx.set()
    ext_buffer = _current_plan(ctx, A, ext_buffer, bm)
    ip, ix, dv = A.device(ctx.device)
    ctx.lib.mggcn_spmm_csr_bf16(ctx.stream(stream_id), ext_buffer.handle if ext_buffer else None, A.n(), A.m(),
                                ip.data_ptr(), ix.data_ptr(), dv.data_ptr(), b_ptr, ldb, C.buffer(), C.m(), bm,
                                alpha, beta, flags, slope)


def _gemm(ctx: context, A: dn_matrix, B: dn_matrix, C: dn_matrix, alpha: float, beta: float,
          A_T: bool = False, B_T: bool = False) -> None:
    A_n, A_m, B_n, B_m = A.n(), A.m(), B.n(), B.m()
    if A_T:
        A_n, A_m = A_m, A_n
    if B_T:
        B_n, B_m = B_m, B_n
    _req(A_m == B_n, "GEMM inner dimensions differ")
    _req(A_n == C.n() and B_m == C.m(), "GEMM output shape mismatch")
    ctx.set()
    ws_bytes = ctx.lib.mggcn_gemm_workspace_bytes(int(A_T), int(B_T), A_n, B_m, A_m)
    ws = ctx.workspace(ws_bytes)
    ctx.lib.mggcn_gemm_f32(ctx.stream(0), int(A_T), int(B_T), A_n, B_m, A_m, alpha, A.buffer(), A.m(),
                           B.buffer(), B.m(), beta, C.buffer(), C.m(), ws.data_ptr() if ws is not None else None,
                           ws_bytes)


def linear_forward(ctx: context, X: dn_matrix, W: dn_matrix, b: dn_matrix, XW: dn_matrix) -> None:
    """XW = X.W + 1 b^T in one GEMM pass (bias in the epilogue) -- the fused form of the
    reference's broadcast_rows + sgemm(beta = 1), src/gcn.hpp:116-123."""
    _req(X.m() == W.n() and XW.n() == X.n() and XW.m() == W.m() and b.m() == W.m() and b.n() == 1, "linear shape")
    ctx.set()
    ws_bytes = ctx.lib.mggcn_gemm_workspace_bytes(0, 0, X.n(), W.m(), X.m())
    ws = ctx.workspace(ws_bytes)
    ctx.lib.mggcn_gemm_bias_f32(ctx.stream(0), 0, 0, X.n(), W.m(), X.m(), 1.0, X.buffer(), X.m(), W.buffer(), W.m(),
                                b.buffer(), XW.buffer(), XW.m(), ws.data_ptr() if ws is not None else None, ws_bytes)


def matmul_lrelu_backward(ctx: context, A: dn_matrix, B: dn_matrix, Z: dn_matrix, C: dn_matrix, alpha: float = 1.0,
                          A_T: bool = False, B_T: bool = False, slope: float = 0.01) -> None:
    """C = (alpha op(A) op(B)) .* (Z > 0 ? 1 : slope): the GEMM that produces a layer's input gradient with the
    leaky_relu_backward of the layer below folded into its epilogue (src/gcn.hpp:135-137 + :462-468)."""
    A_n, A_m, B_n, B_m = A.n(), A.m(), B.n(), B.m()
    if A_T:
        A_n, A_m = A_m, A_n
    if B_T:
        B_n, B_m = B_m, B_n
    _req(A_m == B_n and A_n == C.n() and B_m == C.m() and Z.shape() == C.shape(), "GEMM + mask shape mismatch")
    ctx.set()
    ws_bytes = ctx.lib.mggcn_gemm_workspace_bytes(int(A_T), int(B_T), A_n, B_m, A_m)
    ws = ctx.workspace(ws_bytes)
    ctx.lib.mggcn_gemm_lrelu_bwd_f32(ctx.stream(0), int(A_T), int(B_T), A_n, B_m, A_m, alpha, A.buffer(), A.m(),
                                     B.buffer(), B.m(), Z.buffer(), Z.m(), slope, C.buffer(), C.m(),
                                     ws.data_ptr() if ws is not None else None, ws_bytes)


def linear_backward_weights(ctx: context, X: dn_matrix, G: dn_matrix, G_W: dn_matrix, G_b: dn_matrix) -> None:
    """G_W = X^T G and G_b = 1^T G in ONE pass over G (the fused form of the two sgemms of linear::backward,
    src/gcn.hpp:125-134): the column sums ride on the B tiles of the X^T G kernel."""
    _req(X.n() == G.n() and G_W.shape() == (X.m(), G.m()) and G_b.shape() == (1, G.m()), "linear backward shape")
    ctx.set()
    ws_bytes = ctx.lib.mggcn_gemm_tn_colsum_workspace_bytes(X.m(), G.m(), X.n())
    ws = ctx.workspace(ws_bytes)
    ctx.lib.mggcn_gemm_tn_colsum_f32(ctx.stream(0), X.m(), G.m(), X.n(), 1.0, X.buffer(), X.m(), G.buffer(), G.m(),
                                     G_W.buffer(), G_W.m(), G_b.buffer(), ws.data_ptr() if ws is not None else None, ws_bytes)


def gather_rows(ctx: context, src: dn_matrix, indices, dst: dn_matrix, stream_id: int = 0) -> None:
    """dst[k, :] = src[indices[k], :] (halo pack; indices: device uint32 tensor viewed as int32 storage)"""
    n_idx = int(indices.numel())
    _req(dst.n() >= n_idx and dst.m() == src.m(), "gather_rows shape")
    ctx.lib.mggcn_gather_rows_f32(ctx.stream(stream_id), src.buffer(), src.m(), indices.data_ptr(), n_idx, src.m(),
                                  dst.buffer(), dst.m())


def gather_rows_bf16(ctx: context, src16, indices, dst16, stream_id: int = 0) -> None:
    """dst16[k, :] = src16[indices[k], :] on bf16 bit patterns (mggcn_gather_rows_bf16): the halo pack of a shard that
    is already rounded.  src16 / dst16: 2-D device tensors of 2-byte elements, any row stride (see _bf16_view);
    indices: device uint32 tensor viewed as int32 storage."""
    s_ptr, _, sm, ld_s = _bf16_view(src16, "gather_rows_bf16 src")
    d_ptr, dn, dm, ld_d = _bf16_view(dst16, "gather_rows_bf16 dst")
    n_idx = int(indices.numel())
    _req(dn >= n_idx and dm == sm, "gather_rows_bf16 shape")
    ctx.set()
    ctx.lib.mggcn_gather_rows_bf16(ctx.stream(stream_id), s_ptr, ld_s, indices.data_ptr(), n_idx, sm, d_ptr, ld_d)


# ---- element-wise / row kernels: src/cuda_utils.hpp:470-748 wrappers -----------------
def leaky_relu_forward(ctx: context, in_: dn_matrix, out: dn_matrix, alpha: float = 0.01) -> None:
    _req(in_.shape() == out.shape(), "shape mismatch")
    ctx.lib.mggcn_leaky_relu_forward_f32(ctx.stream(0), in_.buffer(), out.buffer(), in_.size(), alpha)


def leaky_relu_backward(ctx: context, in_: dn_matrix, G_in: dn_matrix, G_out: dn_matrix,
                        alpha: float = 0.01) -> None:
    _req(in_.shape() == G_in.shape() == G_out.shape(), "shape mismatch")
    ctx.lib.mggcn_leaky_relu_backward_f32(ctx.stream(0), in_.buffer(), G_in.buffer(), G_out.buffer(),
                                          in_.size(), alpha)


def broadcast_rows(ctx: context, row: dn_matrix, mat: dn_matrix, discard: bool = True) -> None:
    _req(row.m() == mat.m(), "row width mismatch")
    ctx.lib.mggcn_broadcast_rows_f32(ctx.stream(0), row.buffer(), mat.buffer(), mat.size(), mat.m(), int(discard))


def scale_rows(ctx: context, mat: dn_matrix, scalar: dn_matrix) -> None:
    _req(mat.n() == scalar.n(), "row count mismatch")
    ctx.lib.mggcn_scale_rows_f32(ctx.stream(0), mat.buffer(), scalar.buffer(), mat.size(), mat.m())


def max_rows(ctx: context, mat: dn_matrix, maxs: dn_matrix) -> None:
    _req(mat.n() == maxs.n() and maxs.m() == 1, "maxs must be n x 1")
    ctx.lib.mggcn_max_rows_f32(ctx.stream(0), mat.buffer(), maxs.buffer(), mat.size(), mat.m())


def max_row_indices(ctx: context, mat: dn_matrix, maxs: dn_matrix) -> None:
    _req(mat.n() == maxs.n() and maxs.m() == 1, "maxs must be n x 1")
    ctx.lib.mggcn_max_row_indices_f32(ctx.stream(0), mat.buffer(), maxs.buffer(), mat.size(), mat.m())


def index_log_rows(ctx: context, mat: dn_matrix, indices: dn_matrix, values: dn_matrix) -> None:
    _req(mat.n() == indices.n() and indices.m() == 1 and values.n() == mat.n() and values.m() == 1, "shape")
    ctx.lib.mggcn_index_log_rows_f32(ctx.stream(0), mat.buffer(), indices.buffer(), values.buffer(), mat.size(),
                                     mat.m())


def add_indexed_rows(ctx: context, mat: dn_matrix, indices: dn_matrix, alpha: float) -> None:
    _req(mat.n() == indices.n() and indices.m() == 1, "shape")
    ctx.lib.mggcn_add_indexed_rows_f32(ctx.stream(0), mat.buffer(), indices.buffer(), alpha, mat.size(), mat.m())


def is_equal(ctx: context, mat1: dn_matrix, mat2: dn_matrix, out: dn_matrix) -> None:
    _req(mat1.shape() == mat2.shape() == out.shape(), "shape mismatch")
    ctx.lib.mggcn_is_equal_i32(ctx.stream(0), mat1.buffer(), mat2.buffer(), out.buffer(), mat1.size())


def subtract_rows_exp(ctx: context, mat: dn_matrix, scalar: dn_matrix, out: dn_matrix) -> None:
    _req(mat.n() == scalar.n() and scalar.m() == 1 and mat.shape() == out.shape(), "shape")
    ctx.lib.mggcn_subtract_rows_exp_f32(ctx.stream(0), mat.buffer(), scalar.buffer(), out.buffer(), mat.size(),
                                        mat.m())


def axpy(ctx: context, A: dn_matrix, B: dn_matrix, alpha: float) -> None:
    _req(A.shape() == B.shape(), "shape mismatch")
    ctx.lib.mggcn_axpy_f32(ctx.stream(0), A.buffer(), B.buffer(), alpha, A.size())


def axpby(ctx: context, A: dn_matrix, B: dn_matrix, alpha: float, beta: float) -> None:
    _req(A.shape() == B.shape(), "shape mismatch")
    ctx.lib.mggcn_axpby_f32(ctx.stream(0), A.buffer(), B.buffer(), alpha, beta, A.size())


def aaxpby(ctx: context, A: dn_matrix, B: dn_matrix, alpha: float, beta: float) -> None:
    _req(A.shape() == B.shape(), "shape mismatch")
    ctx.lib.mggcn_aaxpby_f32(ctx.stream(0), A.buffer(), B.buffer(), alpha, beta, A.size())


def adam_final(ctx: context, param: dn_matrix, m: dn_matrix, v: dn_matrix, lr: float, c1: float, c2: float,
               eps: float) -> None:
    _req(param.shape() == m.shape() == v.shape(), "shape mismatch")
    ctx.lib.mggcn_adam_final_f32(ctx.stream(0), param.buffer(), m.buffer(), v.buffer(), lr, c1, c2, eps,
                                 param.size())


def scale_mat(ctx: context, mat: dn_matrix, scalar: float) -> None:
    ctx.lib.mggcn_scale_mat_f32(ctx.stream(0), mat.buffer(), scalar, mat.size())


def dropout_params(p: float):
    """(threshold, scale) of mggcn_dropout_f32 for a drop probability 0 <= p < 1: threshold = floor(p * 2^32) as a
    uint32 and scale = 1 / (1 - p) rounded to fp32 once, both computed in double; ValueError for any other p"""
    _req(isinstance(p, numbers.Real) and 0.0 <= p < 1.0, f"dropout: p must be a number in [0, 1), got {p!r}")   # no NaN
    p = float(p)
    return int(math.floor(p * 4294967296.0)), float(np.float32(1.0 / (1.0 - p)))


def dropout_raw(ctx: context, X: dn_matrix, out: dn_matrix, threshold: int, scale: float, seed: int, stream: int,
                row0: int = 0) -> None:
    """mggcn_dropout_f32 with the (threshold, scale) of dropout_params: what the layers call every epoch"""
    _req(X.shape() == out.shape(), "shape mismatch")
    _req(X.m() >= 1, "row width must be positive")
    ctx.lib.mggcn_dropout_f32(ctx.stream(0), X.buffer(), out.buffer(), X.size(), X.m(), int(row0), int(threshold),
                              scale, int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream) & 0xFFFFFFFF)


def dropout(ctx: context, X: dn_matrix, out: dn_matrix, p: float, seed: int, stream: int, row0: int = 0) -> None:
    """out = keep ? X / (1 - p) : +0.0 with the counter-based mask of mggcn_dropout_f32 (include/mggcn.h): a pure
    function of (seed, stream, row0 + local row, column), never stored.  out may be X; row0 is the global index of X's
    first row (a row shard draws its rows of the whole matrix's mask); the backward pass is the same call on the
    gradient.  ValueError for p outside [0, 1) before any library call."""
    threshold, scale = dropout_params(p)
    _req(int(row0) >= 0, "dropout: row0 must not be negative")
    dropout_raw(ctx, X, out, threshold, scale, seed, stream, row0)


LAYER_NORM_EPS = 1e-5               # torch.nn.LayerNorm's default
LAYER_NORM_MAX_WIDTH = 1024         # MGGCN_LN_MAX_WIDTH: a row lives in the registers of at most one wave
LAYER_NORM_LEAKY_RELU = 1           # MGGCN_LN_LEAKY_RELU: the activation (slope 0.01) rides in the norm kernels


def _req_layer_norm(X, xhat, rstd, gamma, what: str) -> None:
    """the shapes both passes share; shape-only objects are enough (nothing here touches a buffer)"""
    n, m = X.n(), X.m()
    _req(1 <= m <= LAYER_NORM_MAX_WIDTH, f"{what} supports 1 <= m <= {LAYER_NORM_MAX_WIDTH} columns, got {m}")
    _req(xhat.shape() == (n, m), f"{what}: xhat must be {n} x {m}")
    _req(rstd.size() == n, f"{what}: rstd must hold {n} floats")
    _req(gamma.shape() == (1, m), f"{what}: gamma must be 1 x {m}")


def layer_norm(ctx: context, X: dn_matrix, Y: dn_matrix, xhat: dn_matrix, rstd: dn_matrix, gamma: dn_matrix,
               beta: dn_matrix, flags: int = 0) -> None:
    """Y = act(xhat * gamma + beta) row by row, xhat = (X - mean) * rstd, rstd = 1 / sqrt(var + LAYER_NORM_EPS), biased
    variance (mggcn_layer_norm_forward_f32); writes Y, xhat [n x m] and rstd [n].  flags = LAYER_NORM_LEAKY_RELU applies
    the project's leaky ReLU in the same pass.  Y may be X.  ValueError for a width outside 1 .. LAYER_NORM_MAX_WIDTH or a
    shape mismatch, before the library is touched (it would print and exit, not raise)."""
    _req_layer_norm(X, xhat, rstd, gamma, "layer norm")
    _req(Y.shape() == X.shape(), "layer norm: Y must have X's shape")
    _req(beta.shape() == gamma.shape(), f"layer norm: beta must be 1 x {X.m()}")
    ctx.lib.mggcn_layer_norm_forward_f32(ctx.stream(0), X.buffer(), Y.buffer(), xhat.buffer(), rstd.buffer(),
                                         gamma.buffer(), beta.buffer(), X.n(), X.m(), LAYER_NORM_EPS, int(flags))


def layer_norm_backward(ctx: context, G: dn_matrix, act: Optional[dn_matrix], xhat: dn_matrix, rstd: dn_matrix,
                        gamma: dn_matrix, G_in: dn_matrix, G_gamma: dn_matrix, G_beta: dn_matrix, flags: int = 0) -> None:
    """The backward pass of layer_norm (mggcn_layer_norm_backward_f32): G_in [n x m], G_gamma and G_beta [1 x m] from the
    incoming gradient G and the forward's xhat / rstd.  With flags = LAYER_NORM_LEAKY_RELU, G is first multiplied by
    leaky_relu'(act) -- act is a sign source only, as in leaky_relu_backward -- and may be None without it.  G_in may be
    G or act.  The column sums are bitwise reproducible.  The same checks before the library as layer_norm."""
    _req_layer_norm(G, xhat, rstd, gamma, "layer norm backward")
    _req(G_in.shape() == G.shape(), "layer norm backward: G_in must have G's shape")
    _req(G_gamma.shape() == gamma.shape() and G_beta.shape() == gamma.shape(), f"layer norm backward: G_gamma and G_beta must be 1 x {G.m()}")
    leaky = bool(int(flags) & LAYER_NORM_LEAKY_RELU)
    _req(not leaky or (act is not None and act.shape() == G.shape()), "layer norm backward: act must have G's shape")
    ctx.lib.mggcn_layer_norm_backward_f32(ctx.stream(0), G.buffer(), act.buffer() if leaky else None, xhat.buffer(),
                                          rstd.buffer(), gamma.buffer(), G_in.buffer(), G_gamma.buffer(), G_beta.buffer(),
                                          G.n(), G.m(), int(flags))


GATED_SKIP_GATE = 1                 # MGGCN_GS_GATE: y = g r + (1 - g) o with g = sigmoid(the row's score); without it y = o + r
GATED_SKIP_LEAKY_RELU = 2           # MGGCN_GS_LEAKY_RELU: the activation (slope 0.01) rides in the skip kernels
GATED_SKIP_MAX_WIDTH = 1024         # MGGCN_GS_MAX_WIDTH: a row lives in the registers of at most one wave


def _req_gated_skip(o, r, w, gate, flags: int, what: str) -> bool:
    """the shapes both passes share; shape-only objects are enough.  Returns whether the gate is on."""
    n, m = o.n(), o.m()
    _req(int(flags) & ~(GATED_SKIP_GATE | GATED_SKIP_LEAKY_RELU) == 0, f"{what}: unknown flags {int(flags):#x}")
    _req(1 <= m <= GATED_SKIP_MAX_WIDTH, f"{what} supports 1 <= m <= {GATED_SKIP_MAX_WIDTH} columns, got {m}")
    gated = bool(int(flags) & GATED_SKIP_GATE)
    if gated:
        _req(r is not None and r.shape() == (n, m), f"{what}: r must be {n} x {m}")
        _req(w is not None and w.shape() == (3, m), f"{what}: w must be 3 x {m}")
        _req(gate is not None and gate.size() == n, f"{what}: gate must hold {n} floats")
    else:
        _req(w is None and gate is None, f"{what}: w and gate need GATED_SKIP_GATE")
    return gated


def gated_skip(ctx: context, o: dn_matrix, r: dn_matrix, w: Optional[dn_matrix], y: dn_matrix, gate: Optional[dn_matrix],
               flags: int = 0) -> None:
    """The skip connection of an attention layer, row by row (mggcn_gated_skip_forward_f32): y = o + r, or with
    flags & GATED_SKIP_GATE y = g r + (1 - g) o, g = sigmoid(sum_c (w[0] o + w[1] r + w[2] (o - r))) written to ``gate`` [n];
    GATED_SKIP_LEAKY_RELU applies the project's leaky ReLU in the same pass.  o, r, y: [n x m]; w: [3 x m] (None without
    the gate, and so is ``gate``).  y must be neither o nor r.  ValueError for a width outside 1 .. GATED_SKIP_MAX_WIDTH, a
    shape mismatch or an alias, before the library is touched (it would print and exit, not raise)."""
    what = "gated skip"
    gated = _req_gated_skip(o, r, w, gate, flags, what)
    _req(r is not None and r.shape() == o.shape() and y.shape() == o.shape(), f"{what}: r and y must have o's shape")
    _req(y is not o and y is not r, f"{what}: y must not be o or r (the backward pass reads both)")
    ctx.lib.mggcn_gated_skip_forward_f32(ctx.stream(0), o.buffer(), o.m(), r.buffer(), r.m(), w.buffer() if gated else None,
                                         y.buffer(), y.m(), gate.buffer() if gated else None, o.n(), o.m(), int(flags))


def gated_skip_backward(ctx: context, G: dn_matrix, act: Optional[dn_matrix], o: Optional[dn_matrix], r: Optional[dn_matrix],
                        w: Optional[dn_matrix], gate: Optional[dn_matrix], G_o: dn_matrix, G_r: dn_matrix,
                        G_w: Optional[dn_matrix], flags: int = 0) -> None:
    """The backward pass of gated_skip (mggcn_gated_skip_backward_f32): from G, the gradient of y, the gradients G_o and
    G_r [n x m] of o and r and, with the gate, G_w [3 x m].  With GATED_SKIP_LEAKY_RELU G is first multiplied by
    leaky_relu'(act) -- act is a sign source only -- and may be None without it.  Without the gate G_o = G_r = that, o, r,
    w, gate and G_w are not used (None), and G_r may be G_o; with it G_r is a matrix of its own.  G_o may be G or act.  G_w
    is bitwise reproducible.  The same checks before the library as gated_skip."""
    what = "gated skip backward"
    _req(o is not None or not int(flags) & GATED_SKIP_GATE, f"{what}: GATED_SKIP_GATE needs o")
    gated = _req_gated_skip(G if o is None else o, r, w, gate, flags, what)
    _req(o is None or o.shape() == G.shape(), f"{what}: o must have G's shape")
    _req(G_o.shape() == G.shape() and G_r.shape() == G.shape(), f"{what}: G_o and G_r must have G's shape")
    leaky = bool(int(flags) & GATED_SKIP_LEAKY_RELU)
    _req(not leaky or (act is not None and act.shape() == G.shape()), f"{what}: act must have G's shape")
    if gated:
        _req(G_w is not None and G_w.shape() == w.shape(), f"{what}: G_w must be 3 x {G.m()}")
        _req(all(G_r is not x for x in (G, act, o, r, G_o)), f"{what}: with the gate G_r must be a matrix of its own")
        _req(G_o is not o and G_o is not r, f"{what}: G_o must not be o or r")
    else:
        _req(G_w is None, f"{what}: G_w needs GATED_SKIP_GATE")
    m = G.m()
    ctx.lib.mggcn_gated_skip_backward_f32(ctx.stream(0), G.buffer(), m, act.buffer() if leaky else None, m,
                                          o.buffer() if gated else None, m, r.buffer() if gated else None, m,
                                          w.buffer() if gated else None, gate.buffer() if gated else None, G_o.buffer(), m,
                                          G_r.buffer(), m, G_w.buffer() if gated else None, G.n(), m, int(flags))


GAT_MAX_HEADS = 16                  # MGGCN_GAT_MAX_HEADS
GAT_MAX_WIDTH = 1024                # MGGCN_GAT_MAX_WIDTH: heads x width per head
GAT_MAX_EDGE_DIM = 16               # MGGCN_GAT_MAX_EDGE_DIM: columns of the edge features of gat(edge_attr=...)
GAT_SLOPE = 0.2                     # the leaky ReLU of the attention scores (not the layers' 0.01)


def check_gat_heads(heads: int, width: int, what: str = "gat") -> int:
    """the width per head of ``width`` columns cut into ``heads`` heads; ValueError when a limit of the kernels is
    exceeded or the width does not divide, before the library is touched (it would print and exit, not raise)"""
    _req(isinstance(heads, numbers.Integral) and 1 <= heads <= GAT_MAX_HEADS,
         f"{what} supports 1 <= heads <= {GAT_MAX_HEADS}, got {heads!r}")
    _req(1 <= width <= GAT_MAX_WIDTH, f"{what} supports 1 <= heads x width per head <= {GAT_MAX_WIDTH}, got {width}")
    _req(width % heads == 0, f"{what}: a width of {width} is not divisible by {heads} heads")
    return width // int(heads)


LABEL_INPUT_MAX_CLASSES = 256       # MGGCN_LABEL_INPUT_MAX_CLASSES
LABEL_INPUT_MAX_WIDTH = 3 * GAT_MAX_WIDTH      # MGGCN_LABEL_INPUT_MAX_WIDTH: the Z of a dot-product layer
LABEL_INPUT_FED_SET = 3             # the "other" slot of the split-aware loss: where a fed training row is counted


def _req_label_input(rows, cls, E, M, threshold: int, row0: int, what: str) -> None:
    """what both passes share: the lists, the table's shape and limits, ``M`` = Z or G_Z; shape-only objects are enough"""
    C, width = E.n(), E.m()
    _req(1 <= C <= LABEL_INPUT_MAX_CLASSES, f"{what} supports 1 <= classes <= {LABEL_INPUT_MAX_CLASSES}, got {C}")
    _req(1 <= width <= LABEL_INPUT_MAX_WIDTH, f"{what} supports 1 <= width <= {LABEL_INPUT_MAX_WIDTH} columns, got {width}")
    _req(M.m() == width, f"{what}: the table has {width} columns, the rows {M.m()}")
    _req(rows.m() == 1 and cls.shape() == rows.shape(), f"{what}: rows and cls must both be {rows.n()} x 1")
    _req(rows.n() <= M.n(), f"{what}: {rows.n()} listed rows, the matrix has {M.n()}")
    _req(isinstance(threshold, numbers.Integral) and 0 <= threshold < 1 << 32, f"{what}: threshold must be a uint32, got {threshold!r}")
    _req(int(row0) >= 0, f"{what}: row0 must not be negative")


def label_input_forward(ctx: context, rows: dn_matrix, cls: dn_matrix, E: dn_matrix, Z: dn_matrix, threshold: int,
                        feed_all: bool, seed: int, epoch: int, row0: int = 0, kept_set: int = 0,
                        fed_set: int = LABEL_INPUT_FED_SET, S_out: Optional[dn_matrix] = None) -> None:
    """Z[rows[t]] += E[cls[t]] for the listed training rows that are fed this forward, and S_out[rows[t]] = fed_set for
    those, kept_set for the other listed rows (mggcn_label_input_forward_f32).  rows, cls: int32 [T x 1], sorted by (class,
    row) without duplicates; E: [classes x width]; Z: [n x width]; S_out: int32 [n x 1] or None.  A row is fed when
    ``feed_all``, or when its Philox word (label_mask.words on row0 + row, seed, epoch) is below ``threshold``.
    ValueError for a limit (LABEL_INPUT_MAX_CLASSES, LABEL_INPUT_MAX_WIDTH) or a shape that does not fit, before the library
    is touched (it would print and exit, not raise)."""
    what = "label input"
    _req_label_input(rows, cls, E, Z, threshold, row0, what)
    _req(S_out is None or S_out.shape() == (Z.n(), 1), f"{what}: S_out must be {Z.n()} x 1")
    _req(kept_set in TRAIN_SETS and fed_set == int(fed_set), f"{what}: kept_set must be one of {TRAIN_SETS}, got {kept_set!r}")
    ctx.lib.mggcn_label_input_forward_f32(ctx.stream(0), rows.buffer(), cls.buffer(), rows.n(), E.buffer(), E.m(), E.n(),
                                          E.m(), int(threshold), int(bool(feed_all)), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                          int(epoch) & 0xFFFFFFFF, int(row0), int(kept_set), int(fed_set), Z.buffer(), Z.m(),
                                          Z.n(), None if S_out is None else S_out.buffer())


def label_input_backward(ctx: context, rows: dn_matrix, cls: dn_matrix, cls_ptr: dn_matrix, G_Z: dn_matrix, G_E: dn_matrix,
                         threshold: int, feed_all: bool, seed: int, epoch: int, row0: int = 0) -> None:
    """G_E[c] = the sum of G_Z[rows[t]] over the fed rows of class c, +0.0 for a class without one
    (mggcn_label_input_backward_f32); the mask is the forward's, from the same (threshold, feed_all, seed, epoch, row0).
    cls_ptr: int32 [(classes + 1) x 1], the segment of each class in the lists.  G_E is bitwise reproducible.  The same checks
    before the library as label_input_forward."""
    what = "label input backward"
    _req_label_input(rows, cls, G_E, G_Z, threshold, row0, what)
    _req(cls_ptr.shape() == (G_E.n() + 1, 1), f"{what}: cls_ptr must be {G_E.n() + 1} x 1")
    ctx.lib.mggcn_label_input_backward_f32(ctx.stream(0), rows.buffer(), cls.buffer(), cls_ptr.buffer(), rows.n(), G_E.n(),
                                           G_E.m(), int(threshold), int(bool(feed_all)), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                           int(epoch) & 0xFFFFFFFF, int(row0), G_Z.buffer(), G_Z.m(), G_Z.n(), G_E.buffer(),
                                           G_E.m())


def _gat_timed(ctx: context, timer: Optional[str], call) -> None:
    """``call()`` between two events on the compute stream, registered as ``timer`` (None: no events)"""
    if timer is None:
        return call()
    ctx.record(timer + "_0", 0)
    call()
    ctx.record(timer + "_1", 0)
    ctx.register_timer(timer, timer + "_0", timer + "_1")


def _gat_call(ctx: context, timer: Optional[str], name: str, args, extra=None, image: bool = False, tail=None) -> None:
    """mggcn_<name>_f32(*args) under ``timer``; with ``extra`` (the tuple of _gat_drop_args) its _drop twin, which takes it
    after ``args``; ``image``: the _bf16 twin of either (the gathered operands of ``args`` are bf16 images); with ``tail``
    (the tuple of _gat_efeat_args) the _efeat twin of either, fp32 only, which takes it last"""
    entry = getattr(ctx.lib, f"mggcn_{name}{'' if tail is None else '_efeat'}{'' if extra is None else '_drop'}"
                             f"_{'bf16' if image else 'f32'}")
    _gat_timed(ctx, timer, lambda: entry(*args, *(extra or ()), *(tail or ())))


class bf16_image:
    """A bf16 image of an fp32 [rows x columns] matrix, as the ``*_bf16`` attention calls gather from: a 2-D device tensor
    of 2-byte elements (torch.bfloat16, or int16 / uint16 holding the bit patterns) with unit column stride and any row
    stride -- a column range of a wider image is one too.  convert_bf16(ctx, src, image.t) makes it.  n(), m(), shape()
    as on dn_matrix; ld(): the row stride in elements; buffer(): the device pointer (ValueError for a host tensor)."""

    def __init__(self, t):
        _req(hasattr(t, "dim") and t.dim() == 2 and t.element_size() == 2,
             "bf16 image: a 2-D tensor of bf16 (2-byte) elements")
        _req(t.stride(1) == 1 or t.shape[1] <= 1, "bf16 image: columns must be contiguous")
        self.t = t

    def n(self) -> int: return int(self.t.shape[0])
    def m(self) -> int: return int(self.t.shape[1])
    def shape(self): return (self.n(), self.m())
    def ld(self) -> int: return int(max(self.t.stride(0), self.t.shape[1]))

    def buffer(self) -> int:
        _req(self.t.is_cuda, "bf16 image: a device tensor")
        return self.t.data_ptr()

    def columns(self, c0: int, c1: int) -> "bf16_image":
        """the image of columns [c0, c1)"""
        return bf16_image(self.t[:, c0:c1])


def _ld(M) -> int:
    """the leading dimension of a dense operand in elements: a dn_matrix is contiguous, an image has its row stride"""
    return M.ld() if isinstance(M, bf16_image) else M.m()


def _req_roles(what: str, image: bool, gathered, own=()) -> None:
    """the element types of a sparse attention call: with ``image`` every gathered operand is a bf16_image and without it
    none is; an operand read by the call's own rows never is.  ValueError before the library."""
    for M in gathered:
        _req(isinstance(M, bf16_image) == image,
             f"{what}: a gathered operand must be " + ("a bf16 image (ops.bf16_image), not an fp32 matrix" if image
                                                       else "an fp32 matrix, not a bf16 image (the _bf16 call takes images)"))
    for M in own:
        _req(not isinstance(M, bf16_image), f"{what}: an operand read by the call's own rows stays fp32, not a bf16 image")


def _gat_drop_args(drop, what: str, n_dst: int, n_src: int):
    """the six trailing arguments of a mggcn_gat_*_drop_f32 call from ``drop`` = (threshold, scale, seed, stream, dst0, src0):
    threshold and scale as dropout_params gives them; ValueError before the library for anything out of range"""
    _req(len(drop) == 6, f"{what}: drop must be (threshold, scale, seed, stream, dst0, src0)")
    threshold, scale, seed, stream, dst0, src0 = drop
    _req(0 <= int(threshold) <= 0xFFFFFFFF, f"{what}: the dropout threshold must fit 32 bits")
    _req(int(dst0) >= 0 and int(src0) >= 0 and int(dst0) + n_dst <= 1 << 32 and int(src0) + n_src <= 1 << 32,
         f"{what}: dst0 + destinations and src0 + sources must not exceed 2^32 (the library would exit, not raise)")
    return (int(threshold), float(scale), int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream) & 0xFFFFFFFF, int(dst0), int(src0))


def gat_scores(ctx: context, Z: dn_matrix, att: dn_matrix, s_dst: Optional[dn_matrix], s_src: Optional[dn_matrix],
               heads: int, timer: Optional[str] = None) -> None:
    """s_dst[r, k] = Z[r, head k] . att[0, head k] and s_src likewise with att[1] (mggcn_gat_scores_f32); either output
    may be None.  att is [2 x Z.m()], the outputs [Z.n() x heads]."""
    check_gat_heads(heads, Z.m(), "gat scores")
    _req(att.shape() == (2, Z.m()), f"gat scores: att must be 2 x {Z.m()}")
    for s in (s_dst, s_src):
        _req(s is None or s.shape() == (Z.n(), heads), f"gat scores: the scores must be {Z.n()} x {heads}")
    _gat_timed(ctx, timer, lambda: ctx.lib.mggcn_gat_scores_f32(
        ctx.stream(0), Z.buffer(), Z.m(), att.buffer(), s_dst.buffer() if s_dst is not None else None,
        s_src.buffer() if s_src is not None else None, Z.n(), heads, Z.m() // heads))


def gat_forward(ctx: context, F: csr_matrix, Z: dn_matrix, s_dst: dn_matrix, s_src: dn_matrix, out: dn_matrix,
                lse: dn_matrix, heads: int, slope: float = GAT_SLOPE, timer: Optional[str] = None, drop=None) -> None:
    """The edge-softmax fused with the gather (mggcn_gat_forward_f32): over F's pattern (values ignored), lse[i, k] =
    log sum_j exp(lrelu(s_dst[i, k] + s_src[j, k])) and out[i, head k] = sum_j alpha_ijk Z[j, head k].  F: destinations x
    sources; Z, s_src: one row per source; s_dst, out, lse: one row per destination.

    ``drop`` = (threshold, scale, seed, stream, dst0, src0) -- threshold, scale from dropout_params -- is attention dropout
    (mggcn_gat_forward_drop_f32): alpha_ijk is multiplied by q_ijk = keep ? scale : 0 in the gather, lse is unchanged, and
    the mask is a pure function of (seed, stream, dst0 + i, src0 + j, k) that is never stored; gat_backward_dst and
    gat_backward_src take the same tuple and draw the same mask.  None calls the plain entry point."""
    _gat_forward(False, ctx, F, Z, s_dst, s_src, out, lse, heads, slope, timer, drop)


def _gat_forward(image: bool, ctx: context, F: csr_matrix, Z: dn_matrix, s_dst: dn_matrix, s_src: dn_matrix, out: dn_matrix,
                 lse: dn_matrix, heads: int, slope: float = GAT_SLOPE, timer: Optional[str] = None, drop=None,
                 edge=None) -> None:
    """the body of gat_forward, gat_forward_bf16 and gat_forward_efeat; ``image``: the gathered operands are bf16 images
    (the _bf16 entry); ``edge`` = (E, att_edge): the edge term in the score (the _efeat entry)"""
    _req_roles("gat forward", image, (Z,))
    check_gat_heads(heads, Z.m(), "gat forward")
    _req(F.m() == Z.n() and out.shape() == (F.n(), Z.m()), "gat forward: shape mismatch")
    _req(s_dst.shape() == (F.n(), heads) and lse.shape() == (F.n(), heads) and s_src.shape() == (F.m(), heads),
         "gat forward: the scores and lse must be rows x heads")
    tail = None if edge is None else _gat_efeat_args("gat forward", F, *edge, heads)
    extra = None if drop is None else _gat_drop_args(drop, "gat forward", F.n(), F.m())
    ip, ix, _ = F.device(ctx.device)
    args = (ctx.stream(0), F.n(), F.m(), ip.data_ptr(), ix.data_ptr(), Z.buffer(), _ld(Z), s_dst.buffer(), s_src.buffer(), heads,
            Z.m() // heads, slope, out.buffer(), out.m(), lse.buffer())
    _gat_call(ctx, timer, "gat_forward", args, extra, image, tail)


def gat_backward_dst(ctx: context, F: csr_matrix, Z: dn_matrix, s_dst: dn_matrix, s_src: dn_matrix, lse: dn_matrix,
                     G: dn_matrix, out: dn_matrix, D: dn_matrix, ds_dst: dn_matrix, heads: int, slope: float = GAT_SLOPE,
                     timer: Optional[str] = None, drop=None) -> None:
    """The half of the backward pass that sums over sources, over F's rows (mggcn_gat_backward_dst_f32): D[i, k] =
    G[i, head k] . out[i, head k] and ds_dst[i, k] = sum_j alpha_ijk (G[i, head k] . Z[j, head k] - D[i, k]) lrelu'(x_ijk).
    ``drop``: the forward's tuple (see gat_forward; mggcn_gat_backward_dst_drop_f32) -- the dot product carries q_ijk."""
    _gat_backward_dst(False, ctx, F, Z, s_dst, s_src, lse, G, out, D, ds_dst, heads, slope, timer, drop)


def _gat_backward_dst(image: bool, ctx: context, F: csr_matrix, Z: dn_matrix, s_dst: dn_matrix, s_src: dn_matrix,
                      lse: dn_matrix, G: dn_matrix, out: dn_matrix, D: dn_matrix, ds_dst: dn_matrix, heads: int,
                      slope: float = GAT_SLOPE, timer: Optional[str] = None, drop=None, edge=None) -> None:
    """the body of gat_backward_dst, gat_backward_dst_bf16 and gat_backward_dst_efeat; ``image``: the gathered operands are
    bf16 images (the _bf16 entry); ``edge`` = (E, att_edge, P_e): the edge term in the score and the output it adds (the
    _efeat entry)"""
    _req_roles("gat backward", image, (Z,), (G, out))
    check_gat_heads(heads, Z.m(), "gat backward")
    _req(F.m() == Z.n() and G.shape() == (F.n(), Z.m()) and out.shape() == G.shape(), "gat backward: shape mismatch")
    _req(all(s.shape() == (F.n(), heads) for s in (s_dst, lse, D, ds_dst)) and s_src.shape() == (F.m(), heads),
         "gat backward: the scores, lse, D and ds must be rows x heads")
    tail = None
    if edge is not None:
        E, att_edge, P_e = edge
        tail = _gat_efeat_args("gat backward", F, E, att_edge, heads)
        _req(P_e.shape() == (F.n(), heads * E.m()),
             f"gat backward: P_e must be {F.n()} x {heads * E.m()} (rows x heads x edge dimension)")
        tail += (P_e.buffer(), P_e.m())
    extra = None if drop is None else _gat_drop_args(drop, "gat backward", F.n(), F.m())
    ip, ix, _ = F.device(ctx.device)
    args = (ctx.stream(0), F.n(), F.m(), ip.data_ptr(), ix.data_ptr(), Z.buffer(), _ld(Z), s_dst.buffer(), s_src.buffer(),
            lse.buffer(), G.buffer(), G.m(), out.buffer(), out.m(), heads, Z.m() // heads, slope, D.buffer(), ds_dst.buffer())
    _gat_call(ctx, timer, "gat_backward_dst", args, extra, image, tail)


def _req_gat_backward_src(F_T, Z, dst_scalars, s_src, G, att, ds_dst, ds_src, G_Z, heads: int, which: str) -> None:
    """the shapes of gat_backward_src and gat_backward_src_rec; ``dst_scalars``: the [destinations x heads] operands"""
    check_gat_heads(heads, Z.m(), "gat backward")
    _req(F_T.n() == Z.n() and G.shape() == (F_T.m(), Z.m()) and G_Z.shape() == Z.shape(), "gat backward: shape mismatch")
    _req(att.shape() == (2, Z.m()), f"gat backward: att must be 2 x {Z.m()}")
    _req(all(s.shape() == (F_T.m(), heads) for s in dst_scalars) and s_src.shape() == (F_T.n(), heads)
         and ds_src.shape() == (F_T.n(), heads) and (ds_dst is None or ds_dst.shape() == (F_T.n(), heads)),
         f"gat backward: {which} must be rows x heads")


def gat_backward_src(ctx: context, F_T: csr_matrix, Z: dn_matrix, s_dst: dn_matrix, s_src: dn_matrix, lse: dn_matrix,
                     D: dn_matrix, G: dn_matrix, att: dn_matrix, ds_dst: Optional[dn_matrix], ds_src: dn_matrix,
                     G_Z: dn_matrix, heads: int, slope: float = GAT_SLOPE, timer: Optional[str] = None, drop=None) -> None:
    """The half that sums over destinations, over the rows of F^T (mggcn_gat_backward_src_f32; after gat_backward_dst):
    ds_src[j, k] = sum_i ds_ijk and G_Z[j, head k] = sum_i alpha_ijk G[i, head k] + ds_dst[j, k] att[0, head k] +
    ds_src[j, k] att[1, head k].  ds_dst is indexed by source here (the square case passes gat_backward_dst's); None leaves
    its term out.  ``drop``: the forward's tuple (see gat_forward; mggcn_gat_backward_src_drop_f32) -- F_T's rows are the
    sources (offset src0), its entries the destinations (offset dst0)."""
    _gat_backward_src(False, ctx, F_T, Z, s_dst, s_src, lse, D, G, att, ds_dst, ds_src, G_Z, heads, slope, timer, drop)


def _gat_backward_src(image: bool, ctx: context, F_T: csr_matrix, Z: dn_matrix, s_dst: dn_matrix, s_src: dn_matrix,
                      lse: dn_matrix, D: dn_matrix, G: dn_matrix, att: dn_matrix, ds_dst: Optional[dn_matrix],
                      ds_src: dn_matrix, G_Z: dn_matrix, heads: int, slope: float = GAT_SLOPE, timer: Optional[str] = None,
                      drop=None, edge=None) -> None:
    """the body of gat_backward_src, gat_backward_src_bf16 and gat_backward_src_efeat; ``image``: the gathered operands are
    bf16 images (the _bf16 entry); ``edge`` = (E, att_edge): the edge term in the score (the _efeat entry)"""
    _req_roles("gat backward", image, (G,), (Z, G_Z))
    _req_gat_backward_src(F_T, Z, (s_dst, lse, D), s_src, G, att, ds_dst, ds_src, G_Z, heads, "the scores, lse, D and ds")
    tail = None if edge is None else _gat_efeat_args("gat backward", F_T, *edge, heads)
    extra = None if drop is None else _gat_drop_args(drop, "gat backward", F_T.m(), F_T.n())
    ip, ix, _ = F_T.device(ctx.device)
    args = (ctx.stream(0), F_T.n(), F_T.m(), ip.data_ptr(), ix.data_ptr(), Z.buffer(), Z.m(), s_dst.buffer(), s_src.buffer(),
            lse.buffer(), D.buffer(), G.buffer(), _ld(G), att.buffer(), ds_dst.buffer() if ds_dst is not None else None, heads,
            Z.m() // heads, slope, ds_src.buffer(), G_Z.buffer(), G_Z.m())
    _gat_call(ctx, timer, "gat_backward_src", args, extra, image, tail)


def _req_gat_rec(rec, rows: int, heads: int, what: str) -> None:
    """``rec``: a float32 device tensor of rows x heads x 4 floats, contiguous and 16-byte aligned (the library would exit)"""
    _req(rec.is_contiguous() and rec.numel() == rows * heads * 4 and rec.element_size() == 4 and rec.is_floating_point(),
         f"{what}: rec must hold {rows} x {heads} records of 4 floats")
    _req(rec.data_ptr() % 16 == 0, f"{what}: rec must be 16-byte aligned")


def gat_pack_dst(ctx: context, s_dst: dn_matrix, lse: dn_matrix, D: dn_matrix, rec, timer: Optional[str] = None) -> None:
    """rec[(i K + k) 4 + {0, 1, 2, 3}] = s_dst[i, k], lse[i, k], D[i, k], 0 (mggcn_gat_pack_dst_f32): the three scalars
    gat_backward_src needs of a destination as one 16-byte record.  ``rec``: a float32 device tensor of rows x heads x 4."""
    rows, heads = s_dst.shape()
    _req(1 <= heads <= GAT_MAX_HEADS, f"gat pack supports 1 <= heads <= {GAT_MAX_HEADS}")
    _req(lse.shape() == (rows, heads) and D.shape() == (rows, heads), "gat pack: s_dst, lse and D must have one shape")
    _req_gat_rec(rec, rows, heads, "gat pack")
    _gat_timed(ctx, timer, lambda: ctx.lib.mggcn_gat_pack_dst_f32(ctx.stream(0), s_dst.buffer(), lse.buffer(), D.buffer(), rows,
                                                                  heads, rec.data_ptr()))


def gat_backward_src_rec(ctx: context, F_T: csr_matrix, Z: dn_matrix, rec, s_src: dn_matrix, G: dn_matrix, att: dn_matrix,
                         ds_dst: Optional[dn_matrix], ds_src: dn_matrix, G_Z: dn_matrix, heads: int, slope: float = GAT_SLOPE,
                         timer: Optional[str] = None, drop=None) -> None:
    """gat_backward_src with the destinations' (s_dst, lse, D) as the records of gat_pack_dst (mggcn_gat_backward_src_rec_f32
    / _rec_drop_f32): one 16-byte load per (entry, head) where the plain call gathers three scalars, and the bits of the
    plain call on the arrays the record was packed from.  ``rec``: F_T.m() x heads x 4 floats."""
    _req_roles("gat backward", False, (G,), (Z, G_Z))
    _req_gat_backward_src(F_T, Z, (), s_src, G, att, ds_dst, ds_src, G_Z, heads, "the scores and ds")
    _req_gat_rec(rec, F_T.m(), heads, "gat backward")
    extra = None if drop is None else _gat_drop_args(drop, "gat backward", F_T.m(), F_T.n())
    ip, ix, _ = F_T.device(ctx.device)
    args = (ctx.stream(0), F_T.n(), F_T.m(), ip.data_ptr(), ix.data_ptr(), Z.buffer(), Z.m(), rec.data_ptr(), s_src.buffer(),
            G.buffer(), G.m(), att.buffer(), ds_dst.buffer() if ds_dst is not None else None, heads, Z.m() // heads, slope,
            ds_src.buffer(), G_Z.buffer(), G_Z.m())
    _gat_call(ctx, timer, "gat_backward_src_rec", args, extra)


def gat_scores_backward(ctx: context, ds_dst: dn_matrix, Z_dst: dn_matrix, ds_src: dn_matrix, Z_src: dn_matrix,
                        G_att: dn_matrix, heads: int, timer: Optional[str] = None) -> None:
    """G_att[0] = the column sums of ds_dst[i, k(c)] Z_dst[i, c], G_att[1] those of ds_src and Z_src
    (mggcn_gat_scores_backward_f32; bitwise reproducible).  The square case passes the same Z twice."""
    check_gat_heads(heads, Z_src.m(), "gat scores backward")
    _req(Z_dst.m() == Z_src.m() and G_att.shape() == (2, Z_src.m()), f"gat scores backward: G_att must be 2 x {Z_src.m()}")
    _req(ds_dst.shape() == (Z_dst.n(), heads) and ds_src.shape() == (Z_src.n(), heads),
         "gat scores backward: ds must be rows x heads")
    _gat_timed(ctx, timer, lambda: ctx.lib.mggcn_gat_scores_backward_f32(
        ctx.stream(0), ds_dst.buffer(), Z_dst.buffer(), Z_dst.m(), Z_dst.n(), ds_src.buffer(), Z_src.buffer(), Z_src.m(),
        Z_src.n(), heads, Z_src.m() // heads, G_att.buffer()))


def _gat_efeat_args(what: str, F: csr_matrix, E: dn_matrix, att_edge: dn_matrix, heads: int):
    """the four trailing arguments (E, lde, att_edge, de) of a mggcn_gat_*_efeat call: E [F.nnz() x de], one row per entry of
    the matrix the call walks, att_edge [heads x de]; ValueError before the library for a shape or limit that does not fit"""
    de = E.m()
    _req(1 <= de <= GAT_MAX_EDGE_DIM, f"{what} supports 1 <= edge dimension <= {GAT_MAX_EDGE_DIM}, got {de}")
    _req(E.n() == F.nnz(), f"{what}: E must have one row per entry, {F.nnz()}, got {E.n()}")
    _req(att_edge.shape() == (heads, de), f"{what}: att_edge must be {heads} x {de} (heads x edge dimension)")
    return (E.buffer(), de, att_edge.buffer(), de)


def gat_forward_efeat(ctx: context, F: csr_matrix, Z: dn_matrix, s_dst: dn_matrix, s_src: dn_matrix, out: dn_matrix,
                      lse: dn_matrix, E: dn_matrix, att_edge: dn_matrix, heads: int, slope: float = GAT_SLOPE,
                      timer: Optional[str] = None, drop=None) -> None:
    """gat_forward with edge features in the score (mggcn_gat_forward_efeat_f32 / _efeat_drop_f32): x_ijk = (s_dst[i, k] +
    s_src[j, k]) + sum_c E[p, c] att_edge[k, c] for entry p = (i, j) of F's indices array, and everything after x is
    gat_forward's.  ``E``: [F.nnz() x de] in F's entry order, ``att_edge``: [heads x de], de <= GAT_MAX_EDGE_DIM."""
    _gat_forward(False, ctx, F, Z, s_dst, s_src, out, lse, heads, slope, timer, drop, (E, att_edge))


def gat_backward_dst_efeat(ctx: context, F: csr_matrix, Z: dn_matrix, s_dst: dn_matrix, s_src: dn_matrix, lse: dn_matrix,
                           G: dn_matrix, out: dn_matrix, D: dn_matrix, ds_dst: dn_matrix, E: dn_matrix, att_edge: dn_matrix,
                           P_e: dn_matrix, heads: int, slope: float = GAT_SLOPE, timer: Optional[str] = None,
                           drop=None) -> None:
    """gat_backward_dst with the edge term in the score (mggcn_gat_backward_dst_efeat_f32 / _efeat_drop_f32), which also
    writes P_e[i, k de + c] = sum_j ds_ijk E[p, c] over the entries of row i: row i's share of the gradient of att_edge
    (gatv2_att_grad(P_e, G_att_edge viewed as 1 x heads de) sums the rows).  ``E`` in F's entry order; ``P_e``: [F.n() x
    heads de]."""
    _gat_backward_dst(False, ctx, F, Z, s_dst, s_src, lse, G, out, D, ds_dst, heads, slope, timer, drop, (E, att_edge, P_e))


def gat_backward_src_efeat(ctx: context, F_T: csr_matrix, Z: dn_matrix, s_dst: dn_matrix, s_src: dn_matrix, lse: dn_matrix,
                           D: dn_matrix, G: dn_matrix, att: dn_matrix, ds_dst: Optional[dn_matrix], ds_src: dn_matrix,
                           G_Z: dn_matrix, E: dn_matrix, att_edge: dn_matrix, heads: int, slope: float = GAT_SLOPE,
                           timer: Optional[str] = None, drop=None) -> None:
    """gat_backward_src with the edge term in the score (mggcn_gat_backward_src_efeat_f32 / _efeat_drop_f32).  ``E``:
    [F_T.nnz() x de] in F_T's entry order -- the other copy of what gat_forward_efeat read, row for row of the same edge."""
    _gat_backward_src(False, ctx, F_T, Z, s_dst, s_src, lse, D, G, att, ds_dst, ds_src, G_Z, heads, slope, timer, drop,
                      (E, att_edge))


def _req_gat_alpha(F, lse, alpha, heads: int, what: str) -> None:
    """the output of the two exports: one row per entry of F, one column per head; lse one row per destination"""
    _req(alpha.shape() == (F.nnz(), heads), f"{what}: alpha must be {F.nnz()} x {heads} (entries x heads)")
    _req(lse.shape() == (F.n(), heads), f"{what}: lse must be rows x heads")


def gat_alpha(ctx: context, F: csr_matrix, s_dst: dn_matrix, s_src: dn_matrix, lse: dn_matrix, alpha: dn_matrix, heads: int,
              slope: float = GAT_SLOPE, timer: Optional[str] = None) -> None:
    """The attention coefficients of a forward, written out (mggcn_gat_alpha_f32): alpha[p, k] = exp(lrelu(s_dst[i, k] +
    s_src[j, k]) - lse[i, k]) for entry p = (i, j) of F's indices array -- the expression gat_backward_dst and
    gat_backward_src evaluate, from what gat_scores and gat_forward left behind.  ``alpha``: [F.nnz() x heads], row p
    belongs to F's entry p.  The only GAT call that writes something of entries x heads; no training call reads it."""
    _req(isinstance(heads, numbers.Integral) and 1 <= heads <= GAT_MAX_HEADS,
         f"gat alpha supports 1 <= heads <= {GAT_MAX_HEADS}, got {heads!r}")
    _req(s_dst.shape() == (F.n(), heads) and s_src.shape() == (F.m(), heads), "gat alpha: the scores must be rows x heads")
    _req_gat_alpha(F, lse, alpha, heads, "gat alpha")
    if not F.nnz():
        return
    ip, ix, _ = F.device(ctx.device)
    _gat_timed(ctx, timer, lambda: ctx.lib.mggcn_gat_alpha_f32(
        ctx.stream(0), F.n(), F.m(), ip.data_ptr(), ix.data_ptr(), s_dst.buffer(), s_src.buffer(), lse.buffer(), heads, slope,
        alpha.buffer(), alpha.m()))


def _split_operand(M: dn_matrix, width: int, part: int, parts: int, what: str):
    """(pointer, leading dimension) of a dense operand of the GATv2 (``parts`` = 2) and dot-product (3) attention calls:
    ``M`` is either the [rows x width] matrix itself or the model's [rows x parts width] buffer, of which the operand is
    columns [part width, (part + 1) width).  GATv2: part 0 is the source half (Zs, G_Zs), 1 the destination half (Zd,
    G_Zd); dot: 0 the query third (Zq, G_Zq), 1 the key third (Zk, G_Zk), 2 the value third (Zv, G_Zv)"""
    _req(M.m() in (width, parts * width),
         f"{what}: an operand of {M.m()} columns is neither {width} nor {parts} x {width} wide")
    if M.m() == width:
        return M.buffer(), _ld(M)
    return M.buffer() + (2 if isinstance(M, bf16_image) else 4) * width * part, _ld(M)


def _gatv2_width(att: dn_matrix, heads: int, what: str) -> int:
    _req(att.n() == 1, f"{what}: att must be 1 x heads * width per head")
    check_gat_heads(heads, att.m(), what)
    return att.m()


def gatv2_forward(ctx: context, F: csr_matrix, Zs: dn_matrix, Zd: dn_matrix, att: dn_matrix, out: dn_matrix, lse: dn_matrix,
                  heads: int, slope: float = GAT_SLOPE, timer: Optional[str] = None) -> None:
    """The GATv2 edge-softmax fused with the score and the gather (mggcn_gatv2_forward_f32): over F's pattern,
    e_ijk = att[head k] . lrelu(Zd[i, head k] + Zs[j, head k]), lse[i, k] = log sum_j exp(e_ijk) and out[i, head k] =
    sum_j alpha_ijk Zs[j, head k].  F: destinations x sources; att: [1 x width]; out: [F.n() x width]; lse: [F.n() x heads].
    Zs (one row per source) and Zd (one row per destination) are [rows x width] matrices, or the model's [rows x 2 width]
    buffer, of which Zs takes columns [0, width) and Zd columns [width, 2 width) -- the same buffer may be passed as both."""
    _gatv2_forward(False, ctx, F, Zs, Zd, att, out, lse, heads, slope, timer)


def _gatv2_forward(image: bool, ctx: context, F: csr_matrix, Zs: dn_matrix, Zd: dn_matrix, att: dn_matrix, out: dn_matrix,
                   lse: dn_matrix, heads: int, slope: float = GAT_SLOPE, timer: Optional[str] = None) -> None:
    """the body of gatv2_forward and gatv2_forward_bf16; ``image``: the gathered operands are bf16 images (the _bf16 entry)"""
    _req_roles("gatv2 forward", image, (Zs,), (Zd,))
    width = _gatv2_width(att, heads, "gatv2 forward")
    _req(F.m() == Zs.n() and F.n() == Zd.n() and out.shape() == (F.n(), width), "gatv2 forward: shape mismatch")
    _req(lse.shape() == (F.n(), heads), "gatv2 forward: lse must be rows x heads")
    (zs, ldzs), (zd, ldzd) = (_split_operand(M, width, part, 2, "gatv2 forward") for part, M in enumerate((Zs, Zd)))
    ip, ix, _ = F.device(ctx.device)
    _gat_call(ctx, timer, "gatv2_forward", (
        ctx.stream(0), F.n(), F.m(), ip.data_ptr(), ix.data_ptr(), zs, ldzs, zd, ldzd, att.buffer(), heads, width // heads,
        slope, out.buffer(), out.m(), lse.buffer()), None, image)


def gatv2_alpha(ctx: context, F: csr_matrix, Zs: dn_matrix, Zd: dn_matrix, att: dn_matrix, lse: dn_matrix, alpha: dn_matrix,
                heads: int, slope: float = GAT_SLOPE, timer: Optional[str] = None) -> None:
    """The GATv2 attention coefficients of a forward, written out (mggcn_gatv2_alpha_f32): alpha[p, k] = exp(e_ijk -
    lse[i, k]) for entry p = (i, j) of F's indices array, e recomputed from the gathered head-row as gatv2_backward_dst
    does, lse from gatv2_forward.  Zs, Zd as gatv2_forward takes them; ``alpha``: [F.nnz() x heads], row p belongs to F's
    entry p.  The only GATv2 call that writes something of entries x heads; no training call reads it."""
    width = _gatv2_width(att, heads, "gatv2 alpha")
    _req(F.m() == Zs.n() and F.n() == Zd.n(), "gatv2 alpha: shape mismatch")
    _req_gat_alpha(F, lse, alpha, heads, "gatv2 alpha")
    (zs, ldzs), (zd, ldzd) = (_split_operand(M, width, part, 2, "gatv2 alpha") for part, M in enumerate((Zs, Zd)))
    if not F.nnz():
        return
    ip, ix, _ = F.device(ctx.device)
    _gat_timed(ctx, timer, lambda: ctx.lib.mggcn_gatv2_alpha_f32(
        ctx.stream(0), F.n(), F.m(), ip.data_ptr(), ix.data_ptr(), zs, ldzs, zd, ldzd, att.buffer(), lse.buffer(), heads,
        width // heads, slope, alpha.buffer(), alpha.m()))


def gatv2_backward_dst(ctx: context, F: csr_matrix, Zs: dn_matrix, Zd: dn_matrix, att: dn_matrix, lse: dn_matrix,
                       G: dn_matrix, out: dn_matrix, D: dn_matrix, G_Zd: dn_matrix, P: dn_matrix, heads: int,
                       slope: float = GAT_SLOPE, timer: Optional[str] = None) -> None:
    """The half of the GATv2 backward pass that sums over sources, over F's rows (mggcn_gatv2_backward_dst_f32):
    D[i, k] = G[i, head k] . out[i, head k], ds_ijk = alpha_ijk (G[i, head k] . Zs[j, head k] - D[i, k]),
    G_Zd[i, c] = att[c] sum_j ds_ijk lrelu'(t_ijk[c]) and P[i, c] = sum_j ds_ijk lrelu(t_ijk[c]), row i's share of G_att.
    Zs, Zd as gatv2_forward takes them; G_Zd: [F.n() x width], or the [F.n() x 2 width] gradient buffer whose columns
    [width, 2 width) are written; P: [F.n() x width]."""
    _gatv2_backward_dst(False, ctx, F, Zs, Zd, att, lse, G, out, D, G_Zd, P, heads, slope, timer)


def _gatv2_backward_dst(image: bool, ctx: context, F: csr_matrix, Zs: dn_matrix, Zd: dn_matrix, att: dn_matrix, lse: dn_matrix,
                        G: dn_matrix, out: dn_matrix, D: dn_matrix, G_Zd: dn_matrix, P: dn_matrix, heads: int,
                        slope: float = GAT_SLOPE, timer: Optional[str] = None) -> None:
    """the body of gatv2_backward_dst and gatv2_backward_dst_bf16; ``image``: the gathered operands are bf16 images (the _bf16 entry)"""
    what = "gatv2 backward"
    _req_roles(what, image, (Zs,), (Zd, G, out, G_Zd, P))
    width = _gatv2_width(att, heads, what)
    _req(F.m() == Zs.n() and F.n() == Zd.n() and G.shape() == (F.n(), width) and out.shape() == G.shape()
         and P.shape() == G.shape() and G_Zd.n() == F.n(), f"{what}: shape mismatch")
    _req(lse.shape() == (F.n(), heads) and D.shape() == (F.n(), heads), f"{what}: lse and D must be rows x heads")
    (zs, ldzs), (zd, ldzd), (gzd, ldgzd) = (_split_operand(Zs, width, 0, 2, what), _split_operand(Zd, width, 1, 2, what),
                                            _split_operand(G_Zd, width, 1, 2, what))
    ip, ix, _ = F.device(ctx.device)
    _gat_call(ctx, timer, "gatv2_backward_dst", (
        ctx.stream(0), F.n(), F.m(), ip.data_ptr(), ix.data_ptr(), zs, ldzs, zd, ldzd, att.buffer(), lse.buffer(), G.buffer(),
        G.m(), out.buffer(), out.m(), heads, width // heads, slope, D.buffer(), gzd, ldgzd, P.buffer(), P.m()), None, image)


def gatv2_att_grad(ctx: context, P: dn_matrix, G_att: dn_matrix, timer: Optional[str] = None) -> None:
    """G_att[0, c] = sum_i P[i, c] (mggcn_gatv2_att_grad_f32; fixed order, bitwise reproducible): P is gatv2_backward_dst's
    [rows x width], G_att [1 x width]"""
    _req(1 <= P.m() <= GAT_MAX_WIDTH, f"gatv2 att grad supports 1 <= width <= {GAT_MAX_WIDTH}, got {P.m()}")
    _req(G_att.shape() == (1, P.m()), f"gatv2 att grad: G_att must be 1 x {P.m()}")
    _gat_timed(ctx, timer, lambda: ctx.lib.mggcn_gatv2_att_grad_f32(ctx.stream(0), P.buffer(), P.m(), P.n(), P.m(),
                                                                    G_att.buffer()))


def gatv2_backward_src(ctx: context, F_T: csr_matrix, Zs: dn_matrix, Zd: dn_matrix, att: dn_matrix, lse: dn_matrix,
                       D: dn_matrix, G: dn_matrix, G_Zs: dn_matrix, heads: int, slope: float = GAT_SLOPE,
                       timer: Optional[str] = None) -> None:
    """The half that sums over destinations, over the rows of F^T (mggcn_gatv2_backward_src_f32; after gatv2_backward_dst,
    whose D it reads): G_Zs[j, c] = sum_i (alpha_ijk G[i, c] + ds_ijk att[c] lrelu'(t_ijk[c])).  F_T: sources x destinations;
    Zs, Zd as gatv2_forward takes them; G_Zs: [F_T.n() x width], or the [F_T.n() x 2 width] gradient buffer whose columns
    [0, width) are written."""
    _gatv2_backward_src(False, ctx, F_T, Zs, Zd, att, lse, D, G, G_Zs, heads, slope, timer)


def _gatv2_backward_src(image: bool, ctx: context, F_T: csr_matrix, Zs: dn_matrix, Zd: dn_matrix, att: dn_matrix,
                        lse: dn_matrix, D: dn_matrix, G: dn_matrix, G_Zs: dn_matrix, heads: int, slope: float = GAT_SLOPE,
                        timer: Optional[str] = None) -> None:
    """the body of gatv2_backward_src and gatv2_backward_src_bf16; ``image``: the gathered operands are bf16 images (the _bf16 entry)"""
    what = "gatv2 backward"
    _req_roles(what, image, (Zd, G), (Zs, G_Zs))
    width = _gatv2_width(att, heads, what)
    _req(F_T.n() == Zs.n() and F_T.m() == Zd.n() and G.shape() == (F_T.m(), width) and G_Zs.n() == F_T.n(),
         f"{what}: shape mismatch")
    _req(lse.shape() == (F_T.m(), heads) and D.shape() == (F_T.m(), heads), f"{what}: lse and D must be rows x heads")
    (zs, ldzs), (zd, ldzd), (gzs, ldgzs) = (_split_operand(Zs, width, 0, 2, what), _split_operand(Zd, width, 1, 2, what),
                                            _split_operand(G_Zs, width, 0, 2, what))
    ip, ix, _ = F_T.device(ctx.device)
    _gat_call(ctx, timer, "gatv2_backward_src", (
        ctx.stream(0), F_T.n(), F_T.m(), ip.data_ptr(), ix.data_ptr(), zs, ldzs, zd, ldzd, att.buffer(), lse.buffer(),
        D.buffer(), G.buffer(), _ld(G), heads, width // heads, slope, gzs, ldgzs), None, image)


def _req_gatv2_rec(rec, rows: int, heads: int, what: str) -> None:
    """``rec``: a float32 device tensor of rows x heads x 2 floats, contiguous and 8-byte aligned (the library would exit)"""
    _req(rec.is_contiguous() and rec.numel() == rows * heads * 2 and rec.element_size() == 4 and rec.is_floating_point(),
         f"{what}: rec must hold {rows} x {heads} records of 2 floats")
    _req(rec.data_ptr() % 8 == 0, f"{what}: rec must be 8-byte aligned")


def gatv2_pack_dst(ctx: context, lse: dn_matrix, D: dn_matrix, rec, timer: Optional[str] = None) -> None:
    """rec[(i K + k) 2 + {0, 1}] = lse[i, k], D[i, k] (mggcn_gatv2_pack_dst_f32): the two scalars gatv2_backward_src needs of
    a destination as one 8-byte record.  ``rec``: a float32 device tensor of rows x heads x 2."""
    rows, heads = lse.shape()
    _req(1 <= heads <= GAT_MAX_HEADS, f"gatv2 pack supports 1 <= heads <= {GAT_MAX_HEADS}")
    _req(D.shape() == (rows, heads), "gatv2 pack: lse and D must have one shape")
    _req_gatv2_rec(rec, rows, heads, "gatv2 pack")
    _gat_timed(ctx, timer, lambda: ctx.lib.mggcn_gatv2_pack_dst_f32(ctx.stream(0), lse.buffer(), D.buffer(), rows, heads,
                                                                    rec.data_ptr()))


def gatv2_backward_src_rec(ctx: context, F_T: csr_matrix, Zs: dn_matrix, Zd: dn_matrix, att: dn_matrix, rec, G: dn_matrix,
                           G_Zs: dn_matrix, heads: int, slope: float = GAT_SLOPE, timer: Optional[str] = None) -> None:
    """gatv2_backward_src with the destinations' (lse, D) as the records of gatv2_pack_dst (mggcn_gatv2_backward_src_rec_f32):
    one 8-byte load per (entry, head) where the plain call gathers two scalars, and the bits of the plain call on the arrays
    the record was packed from.  ``rec``: F_T.m() x heads x 2 floats; everything else as gatv2_backward_src takes it."""
    what = "gatv2 backward"
    width = _gatv2_width(att, heads, what)
    _req(F_T.n() == Zs.n() and F_T.m() == Zd.n() and G.shape() == (F_T.m(), width) and G_Zs.n() == F_T.n(),
         f"{what}: shape mismatch")
    _req_gatv2_rec(rec, F_T.m(), heads, what)
    (zs, ldzs), (zd, ldzd), (gzs, ldgzs) = (_split_operand(Zs, width, 0, 2, what), _split_operand(Zd, width, 1, 2, what),
                                            _split_operand(G_Zs, width, 0, 2, what))
    ip, ix, _ = F_T.device(ctx.device)
    _gat_timed(ctx, timer, lambda: ctx.lib.mggcn_gatv2_backward_src_rec_f32(
        ctx.stream(0), F_T.n(), F_T.m(), ip.data_ptr(), ix.data_ptr(), zs, ldzs, zd, ldzd, att.buffer(), rec.data_ptr(),
        G.buffer(), G.m(), heads, width // heads, slope, gzs, ldgzs))


def _gatdot_width(out: dn_matrix, heads: int, what: str) -> int:
    check_gat_heads(heads, out.m(), what)
    return out.m()


def gatdot_scale(dh: int) -> float:
    """c = fp32(1 / sqrt(dh)): the default ``scale`` of the dot-product attention calls"""
    return float(np.float32(1 / np.sqrt(dh)))


def gatdot_forward(ctx: context, F: csr_matrix, Zq: dn_matrix, Zk: dn_matrix, Zv: dn_matrix, out: dn_matrix, lse: dn_matrix,
                   heads: int, scale: Optional[float] = None, timer: Optional[str] = None) -> None:
    """The dot-product edge-softmax fused with the score and the gather (mggcn_gatdot_forward_f32): over F's pattern,
    e_ijk = scale (Zq[i, head k] . Zk[j, head k]), lse[i, k] = log sum_j exp(e_ijk) and out[i, head k] =
    sum_j alpha_ijk Zv[j, head k].  F: destinations x sources; out: [F.n() x width]; lse: [F.n() x heads]; ``scale``: None
    for fp32(1 / sqrt(width / heads)).  Zq (one row per destination), Zk and Zv (one row per source) are [rows x width]
    matrices, or the model's [rows x 3 width] buffer, of which Zq takes columns [0, width), Zk [width, 2 width) and Zv
    [2 width, 3 width) -- the same buffer may be passed as all three."""
    _gatdot_forward(False, ctx, F, Zq, Zk, Zv, out, lse, heads, scale, timer)


def _gatdot_forward(image: bool, ctx: context, F: csr_matrix, Zq: dn_matrix, Zk: dn_matrix, Zv: dn_matrix, out: dn_matrix,
                    lse: dn_matrix, heads: int, scale: Optional[float] = None, timer: Optional[str] = None) -> None:
    """the body of gatdot_forward and gatdot_forward_bf16; ``image``: the gathered operands are bf16 images (the _bf16 entry)"""
    what = "gatdot forward"
    _req_roles(what, image, (Zk, Zv), (Zq, out))
    width = _gatdot_width(out, heads, what)
    _req(F.n() == Zq.n() and F.m() == Zk.n() and F.m() == Zv.n() and out.n() == F.n(), f"{what}: shape mismatch")
    _req(lse.shape() == (F.n(), heads), f"{what}: lse must be rows x heads")
    (zq, ldq), (zk, ldk), (zv, ldv) = (_split_operand(Zq, width, 0, 3, what), _split_operand(Zk, width, 1, 3, what),
                                       _split_operand(Zv, width, 2, 3, what))
    scale = gatdot_scale(width // heads) if scale is None else float(scale)
    ip, ix, _ = F.device(ctx.device)
    _gat_call(ctx, timer, "gatdot_forward", (
        ctx.stream(0), F.n(), F.m(), ip.data_ptr(), ix.data_ptr(), zq, ldq, zk, ldk, zv, ldv, heads, width // heads, scale,
        out.buffer(), out.m(), lse.buffer()), None, image)


def gatdot_backward_dst(ctx: context, F: csr_matrix, Zq: dn_matrix, Zk: dn_matrix, Zv: dn_matrix, lse: dn_matrix, G: dn_matrix,
                        out: dn_matrix, D: dn_matrix, G_Zq: dn_matrix, heads: int, scale: Optional[float] = None,
                        timer: Optional[str] = None) -> None:
    """The half of the dot-product backward pass that sums over sources, over F's rows (mggcn_gatdot_backward_dst_f32):
    D[i, k] = G[i, head k] . out[i, head k], ds_ijk = alpha_ijk (G[i, head k] . Zv[j, head k] - D[i, k]) and
    G_Zq[i, head k] = scale sum_j ds_ijk Zk[j, head k].  Zq, Zk, Zv, scale as gatdot_forward takes them; G_Zq: [F.n() x
    width], or the [F.n() x 3 width] gradient buffer whose columns [0, width) are written."""
    _gatdot_backward_dst(False, ctx, F, Zq, Zk, Zv, lse, G, out, D, G_Zq, heads, scale, timer)


def _gatdot_backward_dst(image: bool, ctx: context, F: csr_matrix, Zq: dn_matrix, Zk: dn_matrix, Zv: dn_matrix, lse: dn_matrix,
                         G: dn_matrix, out: dn_matrix, D: dn_matrix, G_Zq: dn_matrix, heads: int,
                         scale: Optional[float] = None, timer: Optional[str] = None) -> None:
    """the body of gatdot_backward_dst and gatdot_backward_dst_bf16; ``image``: the gathered operands are bf16 images (the _bf16 entry)"""
    what = "gatdot backward"
    _req_roles(what, image, (Zk, Zv), (Zq, G, out, G_Zq))
    width = _gatdot_width(out, heads, what)
    _req(F.n() == Zq.n() and F.m() == Zk.n() and F.m() == Zv.n() and out.n() == F.n() and G.shape() == out.shape()
         and G_Zq.n() == F.n(), f"{what}: shape mismatch")
    _req(lse.shape() == (F.n(), heads) and D.shape() == (F.n(), heads), f"{what}: lse and D must be rows x heads")
    (zq, ldq), (zk, ldk), (zv, ldv), (gzq, ldgzq) = (_split_operand(M, width, part, 3, what)
                                                     for M, part in ((Zq, 0), (Zk, 1), (Zv, 2), (G_Zq, 0)))
    scale = gatdot_scale(width // heads) if scale is None else float(scale)
    ip, ix, _ = F.device(ctx.device)
    _gat_call(ctx, timer, "gatdot_backward_dst", (
        ctx.stream(0), F.n(), F.m(), ip.data_ptr(), ix.data_ptr(), zq, ldq, zk, ldk, zv, ldv, lse.buffer(), G.buffer(), G.m(),
        out.buffer(), out.m(), heads, width // heads, scale, D.buffer(), gzq, ldgzq), None, image)


def gatdot_backward_src(ctx: context, F_T: csr_matrix, Zq: dn_matrix, Zk: dn_matrix, Zv: dn_matrix, lse: dn_matrix,
                        D: dn_matrix, G: dn_matrix, G_Zk: dn_matrix, G_Zv: dn_matrix, heads: int,
                        scale: Optional[float] = None, timer: Optional[str] = None) -> None:
    """The half that sums over destinations, over the rows of F^T (mggcn_gatdot_backward_src_f32; after gatdot_backward_dst,
    whose D it reads): G_Zk[j, head k] = scale sum_i ds_ijk Zq[i, head k] and G_Zv[j, head k] = sum_i alpha_ijk G[i, head k].
    F_T: sources x destinations; G: [F_T.m() x width]; Zq, Zk, Zv, scale as gatdot_forward takes them; G_Zk, G_Zv:
    [F_T.n() x width] each, or the [F_T.n() x 3 width] gradient buffer whose columns [width, 2 width) and [2 width, 3 width)
    are written -- the same buffer may be passed as both."""
    _gatdot_backward_src(False, ctx, F_T, Zq, Zk, Zv, lse, D, G, G_Zk, G_Zv, heads, scale, timer)


def _gatdot_backward_src(image: bool, ctx: context, F_T: csr_matrix, Zq: dn_matrix, Zk: dn_matrix, Zv: dn_matrix,
                         lse: dn_matrix, D: dn_matrix, G: dn_matrix, G_Zk: dn_matrix, G_Zv: dn_matrix, heads: int,
                         scale: Optional[float] = None, timer: Optional[str] = None) -> None:
    """the body of gatdot_backward_src and gatdot_backward_src_bf16; ``image``: the gathered operands are bf16 images (the _bf16 entry)"""
    what = "gatdot backward"
    _req_roles(what, image, (Zq, G), (Zk, Zv, G_Zk, G_Zv))
    width = _gatdot_width(G, heads, what)
    _req(F_T.m() == Zq.n() and F_T.n() == Zk.n() and F_T.n() == Zv.n() and G.n() == F_T.m() and G_Zk.n() == F_T.n()
         and G_Zv.n() == F_T.n(), f"{what}: shape mismatch")
    _req(lse.shape() == (F_T.m(), heads) and D.shape() == (F_T.m(), heads), f"{what}: lse and D must be rows x heads")
    _req(G_Zk is not G_Zv or G_Zk.m() == 3 * width, f"{what}: G_Zk and G_Zv must not be the same [rows x width] matrix")
    (zq, ldq), (zk, ldk), (zv, ldv) = (_split_operand(Zq, width, 0, 3, what), _split_operand(Zk, width, 1, 3, what),
                                       _split_operand(Zv, width, 2, 3, what))
    (gzk, ldgzk), (gzv, ldgzv) = _split_operand(G_Zk, width, 1, 3, what), _split_operand(G_Zv, width, 2, 3, what)
    scale = gatdot_scale(width // heads) if scale is None else float(scale)
    ip, ix, _ = F_T.device(ctx.device)
    _gat_call(ctx, timer, "gatdot_backward_src", (
        ctx.stream(0), F_T.n(), F_T.m(), ip.data_ptr(), ix.data_ptr(), zq, ldq, zk, ldk, zv, ldv, lse.buffer(), D.buffer(),
        G.buffer(), _ld(G), heads, width // heads, scale, gzk, ldgzk, gzv, ldgzv), None, image)


# bf16 gathers (gat(agg_dtype="bf16")): one wrapper per mggcn_*_bf16 entry, the _drop forms through ``drop=`` as above.  Each
# takes what the wrapper of the same name without _bf16 takes, with every GATHERED operand -- the one the kernel indexes by
# an entry's column -- as a bf16_image (of the [rows x width] matrix, or of the model's [rows x parts width] buffer) and every
# other operand as the fp32 dn_matrix; the shape checks are the fp32 wrapper's, and an fp32 matrix where an image belongs (or
# the reverse) is a ValueError before the library is touched.  The result is that of the fp32 wrapper on the exactly widened
# images, bit for bit (include/mggcn.h).

def gat_forward_bf16(ctx: context, F: csr_matrix, Z16: bf16_image, s_dst: dn_matrix, s_src: dn_matrix, out: dn_matrix,
                     lse: dn_matrix, heads: int, slope: float = GAT_SLOPE, timer: Optional[str] = None, drop=None) -> None:
    """gat_forward gathering Z from its image (mggcn_gat_forward_bf16 / _drop_bf16); the scores come from the fp32 Z"""
    _gat_forward(True, ctx, F, Z16, s_dst, s_src, out, lse, heads, slope, timer, drop)


def gat_backward_dst_bf16(ctx: context, F: csr_matrix, Z16: bf16_image, s_dst: dn_matrix, s_src: dn_matrix, lse: dn_matrix,
                          G: dn_matrix, out: dn_matrix, D: dn_matrix, ds_dst: dn_matrix, heads: int, slope: float = GAT_SLOPE,
                          timer: Optional[str] = None, drop=None) -> None:
    """gat_backward_dst gathering Z from its image (mggcn_gat_backward_dst_bf16 / _drop_bf16); G and out are the rows' own"""
    _gat_backward_dst(True, ctx, F, Z16, s_dst, s_src, lse, G, out, D, ds_dst, heads, slope, timer, drop)


def gat_backward_src_bf16(ctx: context, F_T: csr_matrix, Z: dn_matrix, s_dst: dn_matrix, s_src: dn_matrix, lse: dn_matrix,
                          D: dn_matrix, G16: bf16_image, att: dn_matrix, ds_dst: Optional[dn_matrix], ds_src: dn_matrix,
                          G_Z: dn_matrix, heads: int, slope: float = GAT_SLOPE, timer: Optional[str] = None, drop=None) -> None:
    """gat_backward_src gathering G from its image (mggcn_gat_backward_src_bf16 / _drop_bf16); Z is the rows' own"""
    _gat_backward_src(True, ctx, F_T, Z, s_dst, s_src, lse, D, G16, att, ds_dst, ds_src, G_Z, heads, slope, timer, drop)


def gatv2_forward_bf16(ctx: context, F: csr_matrix, Zs16: bf16_image, Zd: dn_matrix, att: dn_matrix, out: dn_matrix,
                       lse: dn_matrix, heads: int, slope: float = GAT_SLOPE, timer: Optional[str] = None) -> None:
    """gatv2_forward gathering Zs from its image (mggcn_gatv2_forward_bf16); Zd is the rows' own"""
    _gatv2_forward(True, ctx, F, Zs16, Zd, att, out, lse, heads, slope, timer)


def gatv2_backward_dst_bf16(ctx: context, F: csr_matrix, Zs16: bf16_image, Zd: dn_matrix, att: dn_matrix, lse: dn_matrix,
                            G: dn_matrix, out: dn_matrix, D: dn_matrix, G_Zd: dn_matrix, P: dn_matrix, heads: int,
                            slope: float = GAT_SLOPE, timer: Optional[str] = None) -> None:
    """gatv2_backward_dst gathering Zs from its image (mggcn_gatv2_backward_dst_bf16); Zd, G and out are the rows' own"""
    _gatv2_backward_dst(True, ctx, F, Zs16, Zd, att, lse, G, out, D, G_Zd, P, heads, slope, timer)


def gatv2_backward_src_bf16(ctx: context, F_T: csr_matrix, Zs: dn_matrix, Zd16: bf16_image, att: dn_matrix, lse: dn_matrix,
                            D: dn_matrix, G16: bf16_image, G_Zs: dn_matrix, heads: int, slope: float = GAT_SLOPE,
                            timer: Optional[str] = None) -> None:
    """gatv2_backward_src gathering Zd and G from their images (mggcn_gatv2_backward_src_bf16); Zs is the rows' own"""
    _gatv2_backward_src(True, ctx, F_T, Zs, Zd16, att, lse, D, G16, G_Zs, heads, slope, timer)


def gatdot_forward_bf16(ctx: context, F: csr_matrix, Zq: dn_matrix, Zk16: bf16_image, Zv16: bf16_image, out: dn_matrix,
                        lse: dn_matrix, heads: int, scale: Optional[float] = None, timer: Optional[str] = None) -> None:
    """gatdot_forward gathering Zk and Zv from their images (mggcn_gatdot_forward_bf16); Zq is the rows' own"""
    _gatdot_forward(True, ctx, F, Zq, Zk16, Zv16, out, lse, heads, scale, timer)


def gatdot_backward_dst_bf16(ctx: context, F: csr_matrix, Zq: dn_matrix, Zk16: bf16_image, Zv16: bf16_image, lse: dn_matrix,
                             G: dn_matrix, out: dn_matrix, D: dn_matrix, G_Zq: dn_matrix, heads: int,
                             scale: Optional[float] = None, timer: Optional[str] = None) -> None:
    """gatdot_backward_dst gathering Zk and Zv from their images (mggcn_gatdot_backward_dst_bf16); Zq, G, out are the rows' own"""
    _gatdot_backward_dst(True, ctx, F, Zq, Zk16, Zv16, lse, G, out, D, G_Zq, heads, scale, timer)


def gatdot_backward_src_bf16(ctx: context, F_T: csr_matrix, Zq16: bf16_image, Zk: dn_matrix, Zv: dn_matrix, lse: dn_matrix,
                             D: dn_matrix, G16: bf16_image, G_Zk: dn_matrix, G_Zv: dn_matrix, heads: int,
                             scale: Optional[float] = None, timer: Optional[str] = None) -> None:
    """gatdot_backward_src gathering Zq and G from their images (mggcn_gatdot_backward_src_bf16); Zk, Zv are the rows' own"""
    _gatdot_backward_src(True, ctx, F_T, Zq16, Zk, Zv, lse, D, G16, G_Zk, G_Zv, heads, scale, timer)


AGG_ACCUMULATE = 1                  # MGGCN_AGG_ACCUMULATE
AGG_NONE = 0xFFFFFFFF               # MGGCN_AGG_NONE: the arg of an element for which nothing was selected


def _req_agg_max(what: str, d: int, arg, shape, src0: int, n_src: int) -> None:
    """what both passes of the max aggregator share: the width, the arg matrix (4-byte integers of ``shape``) and src0"""
    _req(1 <= d <= GAT_MAX_WIDTH, f"{what} supports 1 <= width <= {GAT_MAX_WIDTH}, got {d}")
    if arg is not None:
        _req(isinstance(arg, dn_matrix) and str(arg.t.dtype) in ("torch.int32", "torch.uint32") and arg.shape() == shape,
             f"{what}: arg must be a uint32 / int32 matrix of {shape[0]} x {shape[1]}")
    _req(isinstance(src0, numbers.Integral) and 0 <= src0 and src0 + n_src <= AGG_NONE,
         f"{what}: src0 + sources must stay below 2^32 - 1 (the library would exit, not raise)")


def agg_max_forward(ctx: context, F: csr_matrix, B: dn_matrix, out: dn_matrix, arg: Optional[dn_matrix] = None, src0: int = 0,
                    timer: Optional[str] = None) -> None:
    """The max aggregator (mggcn_agg_max_forward_f32): over F's pattern (values ignored) out[i, c] = max over the entries j
    of row i of B[j, c] and arg[i, c] = src0 + j of the winner.  The larger value wins, equal values go to the smaller j, a NaN
    is never selected; a row in which nothing is selected gives +0.0 and AGG_NONE.  F: destinations x sources; B: one row per
    source; out, arg (uint32 / int32, or None: the value only): one row per destination.  ValueError for a shape that does
    not fit, a width outside [1, GAT_MAX_WIDTH], a wrong arg or out aliasing B, before the library is touched (it would print
    and exit, not raise)."""
    what = "agg max forward"
    _req(F.m() == B.n() and out.shape() == (F.n(), B.m()), f"{what}: shape mismatch")
    _req_agg_max(what, B.m(), arg, out.shape(), src0, F.m())
    _req(out.buffer() != B.buffer(), f"{what}: out must not alias B")
    _req(arg is None or arg.buffer() not in (out.buffer(), B.buffer()), f"{what}: arg must not alias out or B")
    ip, ix, _ = F.device(ctx.device)
    _gat_timed(ctx, timer, lambda: ctx.lib.mggcn_agg_max_forward_f32(
        ctx.stream(0), F.n(), F.m(), ip.data_ptr(), ix.data_ptr(), B.buffer(), B.m(), B.m(), int(src0), out.buffer(), out.m(),
        None if arg is None else arg.buffer(), 0 if arg is None else arg.m()))


def agg_max_backward(ctx: context, F_T: csr_matrix, arg: dn_matrix, G: dn_matrix, G_B: dn_matrix, accumulate: bool = False,
                     src0: int = 0, timer: Optional[str] = None) -> None:
    """The backward pass of agg_max_forward over the rows of F^T (mggcn_agg_max_backward_f32): G_B[j, c] = (accumulate ?
    G_B[j, c] : 0) + the sum of G[i, c] over the entries i of row j with arg[i, c] == src0 + j.  An entry equal to its
    predecessor in the row is skipped (a duplicated pair delivers once), so equal indices of a row must be adjacent:
    csr_matrix.transpose() returns rows in ascending order.  F_T: sources x destinations; arg, G: one row per destination;
    G_B: one row per source.  No atomics, the same bits on every call.  The same checks before the library as the forward."""
    what = "agg max backward"
    _req(F_T.m() == G.n() and G_B.shape() == (F_T.n(), G.m()), f"{what}: shape mismatch")
    _req(arg is not None, f"{what}: arg must be the forward's, not None")
    _req_agg_max(what, G.m(), arg, G.shape(), src0, F_T.n())
    _req(G_B.buffer() != G.buffer(), f"{what}: G_B must not alias G")
    _req(arg.buffer() not in (G.buffer(), G_B.buffer()), f"{what}: arg must not alias G or G_B")
    ip, ix, _ = F_T.device(ctx.device)
    _gat_timed(ctx, timer, lambda: ctx.lib.mggcn_agg_max_backward_f32(
        ctx.stream(0), F_T.n(), F_T.m(), ip.data_ptr(), ix.data_ptr(), arg.buffer(), arg.m(), G.buffer(), G.m(), G.m(), int(src0),
        AGG_ACCUMULATE if accumulate else 0, G_B.buffer(), G_B.m()))


def _req_agg_max_rec(rec, rows: int, d: int, what: str) -> None:
    """``rec``: a device tensor of rows x d records of two 4-byte words, contiguous and 8-byte aligned (the library would
    exit)"""
    _req(rec.is_contiguous() and rec.numel() == rows * d * 2 and rec.element_size() == 4,
         f"{what}: rec must hold {rows} x {d} records of two 4-byte words")
    _req(rec.data_ptr() % 8 == 0, f"{what}: rec must be 8-byte aligned")


def agg_max_pack(ctx: context, arg: dn_matrix, G: dn_matrix, rec, timer: Optional[str] = None) -> None:
    """rec[i, 2c] = arg[i, c], rec[i, 2c + 1] = the bits of G[i, c] (mggcn_agg_max_pack_f32): what agg_max_backward gathers
    of a destination -- its selection and its gradient -- as one row of 8-byte records.  ``rec``: a device tensor of
    rows x width x 2 4-byte words (float32 or int32), contiguous, 8-byte aligned, not one of the inputs.  ValueError before
    the library is touched."""
    what = "agg max pack"
    _req(arg is not None, f"{what}: arg must be the forward's, not None")
    _req_agg_max(what, G.m(), arg, G.shape(), 0, 0)
    _req_agg_max_rec(rec, G.n(), G.m(), what)
    _req(rec.data_ptr() not in (arg.buffer(), G.buffer()) and arg.buffer() != G.buffer(), f"{what}: rec must not alias an input")
    _gat_timed(ctx, timer, lambda: ctx.lib.mggcn_agg_max_pack_f32(
        ctx.stream(0), arg.buffer(), arg.m(), G.buffer(), G.m(), G.n(), G.m(), rec.data_ptr(), 2 * G.m()))


def agg_max_backward_rec(ctx: context, F_T: csr_matrix, rec, d: int, G_B: dn_matrix, accumulate: bool = False, src0: int = 0,
                         timer: Optional[str] = None) -> None:
    """agg_max_backward with the destinations' (arg, G) as the records of agg_max_pack (mggcn_agg_max_backward_rec_f32): one
    gather stream where the plain call has two, and the plain call's bits on the matrices the record was packed from.
    ``rec``: F_T.m() x d records; G_B: one row per source, d wide; the rest as agg_max_backward takes it."""
    what = "agg max backward"
    _req(isinstance(d, numbers.Integral) and G_B.shape() == (F_T.n(), d), f"{what}: shape mismatch")
    _req_agg_max(what, d, None, None, src0, F_T.n())
    _req_agg_max_rec(rec, F_T.m(), d, what)
    _req(rec.data_ptr() != G_B.buffer(), f"{what}: G_B must not alias rec")
    ip, ix, _ = F_T.device(ctx.device)
    _gat_timed(ctx, timer, lambda: ctx.lib.mggcn_agg_max_backward_rec_f32(
        ctx.stream(0), F_T.n(), F_T.m(), ip.data_ptr(), ix.data_ptr(), rec.data_ptr(), 2 * d, int(d), int(src0),
        AGG_ACCUMULATE if accumulate else 0, G_B.buffer(), G_B.m()))


# ---- the per-epoch edge sample (csrc/edge_sample.hip) ----------------------------------------------------------------------
EDGE_SAMPLE_DOMAIN = 0xC0000000     # the third Philox counter word of every draw of the edge sample


def _req_u32(t, least: int, what: str) -> None:
    """a contiguous device tensor of at least ``least`` 4-byte integers"""
    _req(hasattr(t, "data_ptr") and t.is_cuda and t.is_contiguous() and t.element_size() == 4
         and not t.dtype.is_floating_point and t.numel() >= least,
         f"{what} must be a contiguous device tensor of at least {least} 4-byte integers")


def _edge_sample_args(what: str, n_rows: int, indptr, indices, thr, transposed, row0: int, col0: int, seed: int, epoch: int):
    _req(isinstance(n_rows, numbers.Integral) and 0 <= n_rows < 1 << 32, f"{what}: n_rows must fit 32 bits")
    _req(transposed in (0, 1, False, True), f"{what}: transposed must be 0 or 1")
    _req_u32(indptr, n_rows + 1, f"{what}: indptr")
    _req_u32(indices, 0, f"{what}: indices")
    _req_u32(thr, 0 if transposed else n_rows, f"{what}: thr")
    for name, v in (("row0", row0), ("col0", col0)):
        _req(isinstance(v, numbers.Integral) and 0 <= v < 1 << 32, f"{what}: {name} must fit 32 bits")
    return (int(n_rows), indptr.data_ptr(), indices.data_ptr(), thr.data_ptr(), int(bool(transposed)), int(row0), int(col0),
            int(seed) & 0xFFFFFFFFFFFFFFFF, int(epoch) & 0xFFFFFFFF)


def edge_sample_count(ctx: context, n_rows: int, indptr, indices, thr, transposed, counts, row0: int = 0, col0: int = 0,
                      seed: int = 0, epoch: int = 0, timer: Optional[str] = None) -> None:
    """counts[r] = the entries of row r that the edge sample keeps (mggcn_edge_sample_count_u32).  Entry (destination i,
    source j) is kept iff i == j, or thr_i == 0xFFFFFFFF, or word 0 of Philox4x32-10((j, i, EDGE_SAMPLE_DOMAIN, epoch), seed)
    is below thr_i.  ``transposed`` 0: rows are destinations (thr[r]); 1: rows are sources and the entry's column is the
    destination (thr[c], which must cover every column).  row0 / col0: the global numbers of row 0 and column 0.  The
    operands are device tensors of 4-byte integers: indptr of n_rows + 1 from its first element on (a row range passes a
    slice), indices as the indptr values address it."""
    what = "edge sample count"
    args = _edge_sample_args(what, n_rows, indptr, indices, thr, transposed, row0, col0, seed, epoch)
    _req_u32(counts, n_rows, f"{what}: counts")
    _gat_timed(ctx, timer, lambda: ctx.lib.mggcn_edge_sample_count_u32(ctx.stream(0), *args, counts.data_ptr()))


def edge_sample_scan(ctx: context, counts, n_rows: int, out_indptr, timer: Optional[str] = None) -> None:
    """out_indptr[0] = 0, out_indptr[r + 1] = counts[0] + ... + counts[r]: n_rows + 1 words (mggcn_edge_sample_scan_u32; three
    launches, no workgroup waits on another)"""
    what = "edge sample scan"
    _req(isinstance(n_rows, numbers.Integral) and 0 <= n_rows < 1 << 32, f"{what}: n_rows must fit 32 bits")
    _req_u32(counts, n_rows, f"{what}: counts")
    _req_u32(out_indptr, n_rows + 1, f"{what}: out_indptr")
    _req(counts.data_ptr() != out_indptr.data_ptr(), f"{what}: out_indptr must not alias counts")
    _gat_timed(ctx, timer, lambda: ctx.lib.mggcn_edge_sample_scan_u32(ctx.stream(0), counts.data_ptr(), int(n_rows),
                                                                      out_indptr.data_ptr()))


def edge_sample_compact(ctx: context, n_rows: int, indptr, indices, thr, transposed, out_indptr, out_indices, row0: int = 0,
                        col0: int = 0, seed: int = 0, epoch: int = 0, timer: Optional[str] = None) -> None:
    """the kept columns of row r, in their original order, at out_indices[out_indptr[r]:out_indptr[r + 1]]
    (mggcn_edge_sample_compact_u32): the bits of edge_sample_count drawn again, out_indptr the scan of its counts.  Nothing
    beyond out_indptr[n_rows] entries is written; out_indices must hold that many (the parent's nnz always does)."""
    what = "edge sample compact"
    args = _edge_sample_args(what, n_rows, indptr, indices, thr, transposed, row0, col0, seed, epoch)
    _req_u32(out_indptr, n_rows + 1, f"{what}: out_indptr")
    _req_u32(out_indices, 0, f"{what}: out_indices")
    _req(out_indices.data_ptr() != indices.data_ptr() or indices.numel() == 0, f"{what}: out_indices must not alias indices")
    _gat_timed(ctx, timer, lambda: ctx.lib.mggcn_edge_sample_compact_u32(ctx.stream(0), *args, out_indptr.data_ptr(),
                                                                         out_indices.data_ptr()))


def _req_f32(t, least: int, what: str) -> None:
    """a contiguous fp32 device tensor of at least ``least`` elements"""
    _req(hasattr(t, "data_ptr") and t.is_cuda and t.is_contiguous() and t.element_size() == 4
         and t.dtype.is_floating_point and t.numel() >= least,
         f"{what} must be a contiguous fp32 device tensor of at least {least} elements")


def edge_sample_rowscale(ctx: context, n_rows: int, indptr, indices, values, thr, counts, scale, row0: int = 0, col0: int = 0,
                         seed: int = 0, epoch: int = 0, timer: Optional[str] = None) -> None:
    """edge_sample_count over a forward matrix WITH values (rows are destinations; mggcn_edge_sample_rowscale_f32): counts[r]
    with count's bits and scale[r] = (the sum of row r's values) / (the sum over its kept entries) -- 0 where nothing of value
    is kept, exactly 1 where the row is kept whole.  values: fp32, indexed like indices."""
    what = "edge sample rowscale"
    args = _edge_sample_args(what, n_rows, indptr, indices, thr, 0, row0, col0, seed, epoch)
    _req_f32(values, 0, f"{what}: values")
    _req(values.numel() >= indices.numel(), f"{what}: values must cover indices")
    _req_u32(counts, n_rows, f"{what}: counts")
    _req_f32(scale, n_rows, f"{what}: scale")
    _gat_timed(ctx, timer, lambda: ctx.lib.mggcn_edge_sample_rowscale_f32(
        ctx.stream(0), *args[:3], values.data_ptr(), args[3], *args[5:], counts.data_ptr(), scale.data_ptr()))


def edge_sample_compact_val(ctx: context, n_rows: int, indptr, indices, values, thr, transposed, scale, scale_self, out_indptr,
                            out_indices, out_values, row0: int = 0, col0: int = 0, seed: int = 0, epoch: int = 0,
                            timer: Optional[str] = None) -> None:
    """edge_sample_compact with values (mggcn_edge_sample_compact_val_f32): beside the kept columns, out_values = value *
    scale[destination] -- scale[r] when the rows are destinations, scale[c] when ``transposed``; None: no factor.  ``scale_self``
    False leaves a self-loop (global row == global column) unscaled.  One array read by both sides: the samples of F and of F^T
    hold the same value bits."""
    what = "edge sample compact"
    args = _edge_sample_args(what, n_rows, indptr, indices, thr, transposed, row0, col0, seed, epoch)
    _req_f32(values, 0, f"{what}: values")
    _req(values.numel() >= indices.numel(), f"{what}: values must cover indices")
    if scale is not None:
        _req_f32(scale, 0 if transposed else n_rows, f"{what}: scale")
    _req(scale_self in (0, 1, False, True), f"{what}: scale_self must be 0 or 1")
    _req_u32(out_indptr, n_rows + 1, f"{what}: out_indptr")
    _req_u32(out_indices, 0, f"{what}: out_indices")
    _req_f32(out_values, 0, f"{what}: out_values")
    _req(out_values.numel() >= out_indices.numel(), f"{what}: out_values must cover out_indices")
    _req(out_indices.data_ptr() != indices.data_ptr() or indices.numel() == 0, f"{what}: out_indices must not alias indices")
    _req(out_values.data_ptr() != values.data_ptr() or values.numel() == 0, f"{what}: out_values must not alias values")
    _gat_timed(ctx, timer, lambda: ctx.lib.mggcn_edge_sample_compact_val_f32(
        ctx.stream(0), *args[:3], values.data_ptr(), *args[3:], scale.data_ptr() if scale is not None else None,
        int(bool(scale_self)), out_indptr.data_ptr(), out_indices.data_ptr(), out_values.data_ptr()))


# ---- the row-split SpMM on a device-built plan (csrc/spmm_dev.hip) ------------------------------------------------------------
def spmm_dev_capacity(lib, indptr, split: int = 0):
    """(work items, partial-sum slots, split rows) of the row-split rule on a host indptr: the capacity that holds every
    sample of that matrix (mggcn_spmm_dev_plan_capacity; no device work).  split 0: MGGCN_SPMM_SPLIT, default 512."""
    ip = np.ascontiguousarray(indptr, dtype=np.uint32)
    _req(ip.ndim == 1 and ip.size >= 1, "spmm dev capacity: indptr of n_rows + 1 words")
    _req(isinstance(split, numbers.Integral) and 0 <= split < 1 << 32, "spmm dev capacity: split must fit 32 bits")
    out = np.zeros(3, dtype=np.uint32)
    lib.mggcn_spmm_dev_plan_capacity(ip.size - 1, ip.ctypes.data, int(split), out.ctypes.data)
    return tuple(int(x) for x in out)


class spmm_dev_buffer:
    """What spmm_dev_plan returns: the capacity of a row-split plan for every sample of one parent matrix, built on the
    device by spmm_dev_plan_build once per draw.  ``cap_items`` / ``cap_slots`` / ``cap_split``, ``split``, ``max_d``;
    read() -> (items [cap_items x 4], split_rows [cap_split x 4], totals [3]) as uint32 host arrays, after a synchronisation."""

    def __init__(self, lib, handle: int, n_rows: int):
        self.lib, self.handle, self.n_rows = lib, handle, int(n_rows)
        d = np.zeros(5, dtype=np.uint32)
        lib.mggcn_spmm_dev_plan_describe(handle, d.ctypes.data)
        self.cap_items, self.cap_slots, self.cap_split, self.split, self.max_d = (int(x) for x in d)
        self.built = False

    def nbytes(self) -> int: return self.lib.mggcn_spmm_dev_plan_bytes(self.handle)

    def read(self):
        items = np.zeros((self.cap_items, 4), dtype=np.uint32)
        rows = np.zeros((self.cap_split, 4), dtype=np.uint32)
        totals = np.zeros(3, dtype=np.uint32)
        self.lib.mggcn_spmm_dev_plan_read(self.handle, items.ctypes.data if items.size else None,
                                          rows.ctypes.data if rows.size else None, totals.ctypes.data)
        return items, rows, totals

    def __del__(self):
        try:
            if self.handle:
                self.lib.mggcn_spmm_dev_plan_destroy(self.handle)
                self.handle = 0
        except Exception:
            pass


def spmm_dev_plan(ctx: context, parent_indptr, max_d: int, split: int = 0) -> spmm_dev_buffer:
    """capacity for the device-built row-split plan of every sample of the matrix with the HOST row pointer ``parent_indptr``
    (mggcn_spmm_dev_plan_create); nothing is built.  max_d: the widest feature width it will multiply at."""
    ip = np.ascontiguousarray(parent_indptr, dtype=np.uint32)
    _req(ip.ndim == 1 and ip.size >= 1, "spmm dev plan: indptr of n_rows + 1 words")
    _req(isinstance(max_d, numbers.Integral) and max_d >= 1, "spmm dev plan: max_d must be positive")
    _req(isinstance(split, numbers.Integral) and 0 <= split < 1 << 32, "spmm dev plan: split must fit 32 bits")
    ctx.set()
    return spmm_dev_buffer(ctx.lib, ctx.lib.mggcn_spmm_dev_plan_create(ip.size - 1, ip.ctypes.data, int(max_d), int(split)),
                           ip.size - 1)


def spmm_dev_plan_build(ctx: context, plan: spmm_dev_buffer, indptr, timer: Optional[str] = None) -> None:
    """builds ``plan`` for the device CSR whose row pointer is ``indptr`` (n_rows + 1 4-byte integers on the device): enqueue-only,
    no host read (mggcn_spmm_dev_plan_build).  No row may be longer than the parent's."""
    _req(isinstance(plan, spmm_dev_buffer) and plan.handle, "spmm dev plan build: a spmm_dev_buffer")
    _req_u32(indptr, plan.n_rows + 1, "spmm dev plan build: indptr")
    ctx.set()
    _gat_timed(ctx, timer, lambda: ctx.lib.mggcn_spmm_dev_plan_build(ctx.stream(0), plan.handle, indptr.data_ptr()))
    plan.built = True


def spmm_dev(ctx: context, A, B, C: dn_matrix, plan: spmm_dev_buffer, alpha: float = 1.0, beta: float = 0.0, flags: int = 0,
             slope: float = 0.01) -> None:
    """C = alpha A B + beta C over a device-resident CSR with values (``A``: an edge_sample.sampled_csr, or anything with n(),
    m() and device() -> (indptr, indices, values)) and its built device plan; B: a dn_matrix (mggcn_spmm_csr_dev_f32) or a 2-D
    bf16 device tensor of A.m() x C.m(), any row stride (mggcn_spmm_csr_dev_bf16).  The bits of matmul with a host row-split
    plan of the same split on the same matrix."""
    what = "spmm dev"
    _req(isinstance(plan, spmm_dev_buffer) and plan.handle and plan.built, f"{what}: the plan has not been built")
    ip, ix, dv = A.device(ctx.device)
    _req(dv is not None, f"{what}: the matrix carries no values")
    _req(plan.n_rows == A.n() == C.n(), f"{what}: the plan was made for another matrix")
    _req_u32(ip, A.n() + 1, f"{what}: indptr")
    _req_u32(ix, 0, f"{what}: indices")
    _req_f32(dv, 0, f"{what}: values")
    if isinstance(B, dn_matrix):
        b_ptr, bn, bm, ldb, fn = B.buffer(), B.n(), B.m(), B.m(), ctx.lib.mggcn_spmm_csr_dev_f32
    elif hasattr(B, "element_size") and B.element_size() == 4:              # a 2-D fp32 device tensor, any row stride
        _req(B.dim() == 2 and B.is_cuda and B.dtype.is_floating_point and (B.stride(1) == 1 or B.shape[1] <= 1),
             f"{what} B: a dn_matrix, a 2-D fp32 device tensor or a 2-D bf16 device tensor")
        b_ptr, bn, bm, ldb = B.data_ptr(), int(B.shape[0]), int(B.shape[1]), int(max(B.stride(0), B.shape[1]))
        fn = ctx.lib.mggcn_spmm_csr_dev_f32
    else:
        b_ptr, bn, bm, ldb = _bf16_view(B, f"{what} B")
        fn = ctx.lib.mggcn_spmm_csr_dev_bf16
    _req(A.m() == bn and bm == C.m(), "SpMM shape mismatch")
    _req(bm <= plan.max_d or plan.cap_slots == 0, f"{what}: feature width exceeds the plan's max_d")
    _req(b_ptr != C.buffer(), f"{what}: C must not alias B")
    ctx.set()
    fn(ctx.stream(0), plan.handle, A.n(), A.m(), ip.data_ptr(), ix.data_ptr(), dv.data_ptr(), b_ptr, ldb, C.buffer(), C.m(), bm,
       alpha, beta, flags, slope)


# ---- the stable segmented radix sort (csrc/radix_sort.hip) and the ROC-AUC integers on top of it (csrc/roc_auc.hip) ---------
RADIX_SORT_TILE = 4096              # MGGCN_RADIX_SORT_TILE: pairs per workgroup of a digit pass
ROC_AUC_CHUNK = 1024                # MGGCN_ROC_AUC_CHUNK: pairs per wave of the statistic
ROC_AUC_VIEWS = ("train", "val", "test", "other", "all")        # the k of stats[c][k]: SPLIT_NAMES, then every row


def _req_count(v, what: str) -> int:
    _req(isinstance(v, numbers.Integral) and not isinstance(v, bool) and v >= 0, f"{what} must be a non-negative integer")
    return int(v)


def radix_sort_work_bytes(n_seg: int, seg_len: int) -> int:
    """mggcn_radix_sort_work_bytes restated on the host (a digit histogram per tile and its scan, one word more)"""
    n_seg, seg_len = _req_count(n_seg, "radix sort: n_seg"), _req_count(seg_len, "radix sort: seg_len")
    if n_seg == 0 or seg_len == 0:
        return 0
    return 4 * (2 * n_seg * 256 * (-(-seg_len // RADIX_SORT_TILE)) + 1)


def _req_work(work, least: int, what: str) -> None:
    _req(work is not None and hasattr(work, "data_ptr") and work.is_cuda and work.is_contiguous()
         and work.numel() * work.element_size() >= least and work.data_ptr() % 8 == 0,
         f"{what}: work_bytes too small: work must be a contiguous, 8-byte aligned device tensor of at least {least} bytes")


def radix_sort_pairs(ctx: context, n_seg: int, seg_len: int, keys, vals, keys_alt, vals_alt, work, begin_bit: int = 0,
                     end_bit: int = 32, timer: Optional[str] = None) -> None:
    """Sorts n_seg segments of seg_len (key, value) pairs each, every segment on its own, ascending on the key bits
    [begin_bit, end_bit), equal keys in their input order (mggcn_radix_sort_pairs_u32: a stable LSD radix sort, one pass per
    8-bit digit; the same bits on every call).  The four arrays are device tensors of 4-byte integers, at least
    n_seg * seg_len long, none overlapping another; the result is in keys / vals, the _alt pair is scratch.  work: a device
    tensor of radix_sort_work_bytes(n_seg, seg_len) bytes.  Enqueue-only.  Refused with ValueError before the library:
    begin_bit / end_bit outside 0 <= begin_bit < end_bit <= 32, n_seg * seg_len >= 2^31, a work that is too small, any overlap."""
    what = "radix sort"
    for name, b in (("begin_bit", begin_bit), ("end_bit", end_bit)):
        _req(isinstance(b, numbers.Integral) and not isinstance(b, bool), f"{what}: {name} must be an integer")
    _req(0 <= begin_bit < end_bit <= 32, f"{what}: 0 <= begin_bit < end_bit <= 32, got begin_bit {begin_bit}, end_bit {end_bit}")
    n_seg, seg_len = _req_count(n_seg, f"{what}: n_seg"), _req_count(seg_len, f"{what}: seg_len")
    total = n_seg * seg_len
    _req(total < 1 << 31, f"{what}: n_seg * seg_len must be below 2^31, got {total}")
    if total == 0:
        return
    arrays = (("keys", keys), ("vals", vals), ("keys_alt", keys_alt), ("vals_alt", vals_alt))
    for name, t in arrays:
        _req_u32(t, total, f"{what}: {name}")
    for i, (na, a) in enumerate(arrays):
        for nb, b in arrays[i + 1:]:
            _req(a.data_ptr() + 4 * total <= b.data_ptr() or b.data_ptr() + 4 * total <= a.data_ptr(),
                 f"{what}: {na} and {nb} must not alias (overlap)")
    need = radix_sort_work_bytes(n_seg, seg_len)
    _req_work(work, need, what)
    _gat_timed(ctx, timer, lambda: ctx.lib.mggcn_radix_sort_pairs_u32(
        ctx.stream(0), n_seg, seg_len, keys.data_ptr(), vals.data_ptr(), keys_alt.data_ptr(), vals_alt.data_ptr(),
        int(begin_bit), int(end_bit), work.data_ptr(), work.numel() * work.element_size()))


def _dense_window(M, dtype_float: bool, what: str):
    """(pointer, leading dimension, rows, columns) of a row-major operand of 4-byte elements: a dn_matrix, or a 2-D device
    tensor with unit column stride (a column window of a wider matrix)"""
    t = M.t if isinstance(M, dn_matrix) else M
    _req(hasattr(t, "dim") and t.dim() == 2 and t.element_size() == 4 and t.dtype.is_floating_point == dtype_float,
         f"{what} must be a 2-D {'fp32' if dtype_float else 'int32'} matrix (a dn_matrix or a column window of one)")
    _req(t.shape[1] <= 1 or t.stride(1) == 1, f"{what}: columns must be contiguous")
    _req(t.is_cuda, f"{what} must be on the device")
    n, m = int(t.shape[0]), int(t.shape[1])
    return t.data_ptr(), (max(int(t.stride(0)), m) if n > 1 else max(m, 1)), n, m


def roc_auc_keys(ctx: context, logits, targets, sets: Optional[dn_matrix], c0: int, nc: int, keys, vals,
                 timer: Optional[str] = None) -> None:
    """keys[(c - c0) n + i], vals[...] of columns [c0, c0 + nc) of the logits (mggcn_roc_auc_keys_f32): key = the logit's
    bits made sortable (-0.0 ties with +0.0; a NaN falls where the map puts its bit pattern), value = slot << 1 |
    (target != 0), slot as SPLIT_NAMES (sets None: every row is slot 0).  logits (fp32) / targets (int32): a dn_matrix or a
    2-D device tensor with unit column stride, n rows and the same number of columns; keys / vals: device tensors of at
    least n * nc 4-byte integers."""
    what = "roc-auc keys"
    lp, ldl, n, m = _dense_window(logits, True, f"{what}: logits")
    tp, ldt, tn, tm = _dense_window(targets, False, f"{what}: targets")
    _req((tn, tm) == (n, m), f"{what}: targets must be {n} x {m} like the logits, got {tn} x {tm}")
    c0, nc = _req_count(c0, f"{what}: c0"), _req_count(nc, f"{what}: nc")
    _req(c0 + nc <= m, f"{what}: columns [{c0}, {c0 + nc}) exceed the {m} of the logits")
    _req(n < 1 << 31 and n * nc < 1 << 31, f"{what}: n * nc must be below 2^31")
    if sets is not None:
        _req_sets(sets, n, what)
    _req_u32(keys, n * nc, f"{what}: keys")
    _req_u32(vals, n * nc, f"{what}: vals")
    _req(keys.data_ptr() != vals.data_ptr() or n * nc == 0, f"{what}: keys must not alias vals")
    _gat_timed(ctx, timer, lambda: ctx.lib.mggcn_roc_auc_keys_f32(
        ctx.stream(0), lp, ldl, tp, ldt, sets.buffer() if sets is not None else None, n, c0, nc, keys.data_ptr(),
        vals.data_ptr()))


def roc_auc_stats_work_bytes(n: int, nc: int) -> int:
    """mggcn_roc_auc_stats_work_bytes restated on the host: per class and chunk eight u32 counts and five i64 partials, eight
    u32 totals per class, each table rounded up to 256 bytes"""
    n, nc = _req_count(n, "roc-auc stats: n"), _req_count(nc, "roc-auc stats: nc")
    if n == 0 or nc == 0:
        return 0
    chunks = -(-n // ROC_AUC_CHUNK)
    return sum(-(-b // 256) * 256 for b in (nc * chunks * 32, nc * 32, nc * chunks * 40))


def roc_auc_stats(ctx: context, keys, vals, n: int, nc: int, stats, work, timer: Optional[str] = None) -> None:
    """stats[c][k] = (2U, P, N) as int64 words, k over ROC_AUC_VIEWS, from nc segments of n pairs SORTED on the key
    (mggcn_roc_auc_stats_u64): P / N the positives / negatives of the view, 2U = 2 #{(p, n): key_n < key_p} + #{key_n ==
    key_p}.  stats: a device tensor of at least nc * 15 8-byte integers; work: roc_auc_stats_work_bytes(n, nc) bytes."""
    what = "roc-auc stats"
    n, nc = _req_count(n, f"{what}: n"), _req_count(nc, f"{what}: nc")
    _req(n < 1 << 31 and n * nc < 1 << 31, f"{what}: n * nc must be below 2^31")
    if nc == 0:
        return
    _req_u32(keys, n * nc, f"{what}: keys")
    _req_u32(vals, n * nc, f"{what}: vals")
    _req(hasattr(stats, "data_ptr") and stats.is_cuda and stats.is_contiguous() and stats.element_size() == 8
         and not stats.dtype.is_floating_point and stats.numel() >= nc * 15,
         f"{what}: stats must be a contiguous device tensor of at least {nc * 15} 8-byte integers")
    need = roc_auc_stats_work_bytes(n, nc)
    if need:
        _req_work(work, need, what)
    _gat_timed(ctx, timer, lambda: ctx.lib.mggcn_roc_auc_stats_u64(
        ctx.stream(0), keys.data_ptr(), vals.data_ptr(), n, nc, stats.data_ptr(), work.data_ptr() if need else None,
        work.numel() * work.element_size() if need else 0))


def abssum(ctx: context, A: dn_matrix, result_device) -> None:
    """cublasSasum (src/cuda_utils.hpp:362-371).  ``result_device``: 1-element float32
    device tensor; enqueue-only (the reference's call blocks the host)."""
    ctx.lib.mggcn_abssum_f32(ctx.stream(0), A.buffer(), A.size(), result_device.data_ptr())


# ---- fused tail ------------------------------------------------
XENT_FUSED_MAX_CLASSES = 1024       # 64 lanes x kXentMaxPerLane logits per lane (elementwise.hip)


def softmax_xent_fused(ctx: context, H: dn_matrix, Y: dn_matrix, grad_scale: float, sums_device,
                       out: Optional[dn_matrix] = None) -> None:
    """softmax + argmax + log-prob + gradient in one pass; in place on H, or H -> out (the loss layer's copy = True:
    the pass is the copy).  1 <= H.m() <= XENT_FUSED_MAX_CLASSES: the kernel keeps a row in the registers of one wave
    (the library would print and exit, not raise)"""
    _req(H.n() == Y.n() and Y.m() == 1, "labels must be n x 1")
    _req(1 <= H.m() <= XENT_FUSED_MAX_CLASSES, f"fused loss supports 1 <= m <= {XENT_FUSED_MAX_CLASSES} classes, got {H.m()}")
    if out is None:
        out = H
    _req(out.n() == H.n() and out.m() == H.m(), "fused loss: gradient matrix must have the logits' shape")
    ctx.lib.mggcn_softmax_xent_fused_from_f32(ctx.stream(0), H.buffer(), out.buffer(), Y.buffer(), H.n(), H.m(),
                                              grad_scale, sums_device.data_ptr())


TRAIN_SETS = (0, 1, 2)              # sets.bin: 0 train / 1 validation / 2 test; any other value is "other" (slot 3)
SPLIT_NAMES = ("train", "val", "test", "other")


def _req_sets(S: dn_matrix, n: int, what: str) -> None:
    _req(isinstance(S, dn_matrix) and S.t.dtype == __import__("torch").int32, f"{what}: the sets must be an int32 dn_matrix")
    _req(S.n() == n and S.m() == 1, f"{what}: the sets must be {n} x 1, got {S.n()} x {S.m()}")


def softmax_xent_split(ctx: context, H: dn_matrix, Y: dn_matrix, S: dn_matrix, train_set: int, grad_scale: float,
                       sums_device, out: Optional[dn_matrix] = None) -> None:
    """The split-aware fused loss (mggcn_softmax_xent_split_from_f32): rows with S != train_set get a zero gradient row;
    sums_device holds eight floats, a (loss sum, correct count) pair per slot train / val / test / other, zeroed by the
    caller.  The same width limit and the same check before the library as softmax_xent_fused."""
    _req(H.n() == Y.n() and Y.m() == 1, "labels must be n x 1")
    _req(1 <= H.m() <= XENT_FUSED_MAX_CLASSES, f"fused loss supports 1 <= m <= {XENT_FUSED_MAX_CLASSES} classes, got {H.m()}")
    _req(train_set in TRAIN_SETS, f"train_set must be one of {TRAIN_SETS}, got {train_set!r}")
    _req_sets(S, H.n(), "split-aware fused loss")
    if out is None:
        out = H
    _req(out.n() == H.n() and out.m() == H.m(), "fused loss: gradient matrix must have the logits' shape")
    _req(sums_device.numel() >= 8, "split-aware fused loss: sums must hold eight floats")
    ctx.lib.mggcn_softmax_xent_split_from_f32(ctx.stream(0), H.buffer(), out.buffer(), Y.buffer(), S.buffer(), H.n(),
                                              H.m(), int(train_set), grad_scale, sums_device.data_ptr())


BCE_SUMS = 16                       # MGGCN_BCE_SUMS: (loss sum, TP, FP, FN) per slot train / val / test / other


def sigmoid_bce(ctx: context, H: dn_matrix, T: dn_matrix, S: Optional[dn_matrix], train_set: int, grad_scale: float,
                sums_device, out: Optional[dn_matrix] = None) -> None:
    """The multi-label loss (mggcn_sigmoid_bce_from_f32): sigmoid + binary cross-entropy + gradient + the micro-F1 counts
    in one pass, in place on H or H -> out.  T: int32 targets of H's shape (non-zero = positive); S: the sets or None
    (every row trains and counts as slot 0); sums_device holds BCE_SUMS floats, zeroed by the caller.  Any width >= 1."""
    torch = __import__("torch")
    _req(H.m() >= 1, "sigmoid-BCE loss: the width must be positive")
    _req(isinstance(T, dn_matrix) and T.t.dtype == torch.int32, "sigmoid-BCE loss: the targets must be an int32 dn_matrix")
    _req(T.n() == H.n() and T.m() == H.m(),
         f"sigmoid-BCE loss: the targets must be {H.n()} x {H.m()} like the logits, got {T.n()} x {T.m()}")
    _req(train_set in TRAIN_SETS, f"train_set must be one of {TRAIN_SETS}, got {train_set!r}")
    if S is not None:
        _req_sets(S, H.n(), "sigmoid-BCE loss")
    if out is None:
        out = H
    _req(out.n() == H.n() and out.m() == H.m(), "sigmoid-BCE loss: gradient matrix must have the logits' shape")
    _req(sums_device.numel() >= BCE_SUMS, f"sigmoid-BCE loss: sums must hold {BCE_SUMS} floats")
    ctx.lib.mggcn_sigmoid_bce_from_f32(ctx.stream(0), H.buffer(), out.buffer(), T.buffer(),
                                       S.buffer() if S is not None else None, H.n(), H.m(), int(train_set), grad_scale,
                                       sums_device.data_ptr())


def select_rows_by_set(ctx: context, mat: dn_matrix, S: dn_matrix, set_: int) -> None:
    """mat[i, :] = +0.0 where S[i] != set_ (mggcn_select_rows_by_set_f32)"""
    _req(mat.m() >= 1, "row width must be positive")
    _req_sets(S, mat.n(), "select_rows_by_set")
    ctx.lib.mggcn_select_rows_by_set_f32(ctx.stream(0), mat.buffer(), S.buffer(), int(set_), mat.size(), mat.m())


def abssum_by_set(ctx: context, x: dn_matrix, S: dn_matrix, result_device) -> None:
    """result_device[k] = sum of |x[i]| over the rows of slot k (train / val / test / other): four floats, overwritten
    (mggcn_abssum_by_set_f32); x is n x 1.  Enqueue-only, like abssum."""
    _req(x.m() == 1, "abssum_by_set: x must be n x 1")
    _req_sets(S, x.n(), "abssum_by_set")
    _req(result_device.numel() >= 4, "abssum_by_set: the result must hold four floats")
    ctx.lib.mggcn_abssum_by_set_f32(ctx.stream(0), x.buffer(), S.buffer(), x.n(), result_device.data_ptr())


# ---- Correct and Smooth (smoothing.py): the row kernels around the two propagation loops ---------------------------------
CS_FIX_TRAIN = 1                    # MGGCN_CS_FIX_TRAIN: a training row of the step's output is R's, unclamped
CS_AUTOSCALE = 2                    # MGGCN_CS_AUTOSCALE: s_i = sigma / sum |E[i]| (1 where not finite or above 1000)
CS_SET_LABELS = 4                   # MGGCN_CS_SET_LABELS: a training row of the corrected output is onehot(y)
CS_MAX_WIDTH = 1024                 # MGGCN_CS_MAX_WIDTH: a row lives in the registers of at most one wave


def _req_cs(mats, what: str) -> None:
    """every (name, dn_matrix) of ``mats`` is fp32 and has the shape of the first, 1 <= m <= CS_MAX_WIDTH"""
    torch = __import__("torch")
    (_, first) = mats[0]
    _req(1 <= first.m() <= CS_MAX_WIDTH, f"{what} supports 1 <= m <= {CS_MAX_WIDTH} columns, got {first.m()}")
    for name, M in mats:
        _req(M.n() == first.n() and M.m() == first.m(),
             f"{what}: {name} must be {first.n()} x {first.m()}, got {M.n()} x {M.m()}")
        _req(isinstance(M, dn_matrix) and M.t.dtype == torch.float32 and M.t.is_contiguous(),
             f"{what}: {name} must be a contiguous fp32 dn_matrix")


def _req_cs_labels(Y, S, n: int, train_set: int, what: str) -> None:
    _req(train_set in TRAIN_SETS, f"train_set must be one of {TRAIN_SETS}, got {train_set!r}")
    _req(isinstance(Y, dn_matrix) and Y.t.dtype == __import__("torch").int32, f"{what}: the labels must be an int32 dn_matrix")
    _req(Y.n() == n and Y.m() == 1, f"{what}: the labels must be {n} x 1, got {Y.n()} x {Y.m()}")
    _req_sets(S, n, what)


def cs_residual(ctx: context, logits: dn_matrix, Y: dn_matrix, S: dn_matrix, train_set: int, P: dn_matrix, E0: dn_matrix,
                sums_device) -> None:
    """P = softmax(logits) row-wise, E0 = onehot(Y) - P on the rows with S == train_set and +0.0 elsewhere,
    sums_device[0] = sum |E0| (mggcn_cs_residual_f32).  The labels of the training rows must lie in [0, m): the caller's
    check (correct_and_smooth does it on the host), the kernel does not look."""
    _req_cs([("logits", logits), ("P", P), ("E0", E0)], "cs_residual")
    _req_cs_labels(Y, S, logits.n(), train_set, "cs_residual")
    _req(sums_device.numel() >= 1, "cs_residual: sums must hold one float")
    ctx.lib.mggcn_cs_residual_f32(ctx.stream(0), logits.buffer(), Y.buffer(), S.buffer(), logits.n(), logits.m(),
                                  int(train_set), P.buffer(), E0.buffer(), sums_device.data_ptr())


def cs_step(ctx: context, T: dn_matrix, R: dn_matrix, S: Optional[dn_matrix], alpha: float, beta: float, lo: float, hi: float,
            train_set: int = 0, flags: int = 0, out: Optional[dn_matrix] = None) -> None:
    """out = clamp(fma(alpha, T, beta R), lo, hi), in place on T by default (mggcn_cs_step_f32); with CS_FIX_TRAIN the rows
    with S == train_set are R's.  out must not be R."""
    if out is None:
        out = T
    _req_cs([("T", T), ("R", R), ("out", out)], "cs_step")
    _req(flags & ~CS_FIX_TRAIN == 0, f"cs_step: unknown flags {flags:#x}")
    _req(not lo > hi, f"cs_step: lo {lo} is above hi {hi}")
    _req(out is not R and out.buffer() != R.buffer(), "cs_step: out must not alias R")
    if flags & CS_FIX_TRAIN:
        _req(train_set in TRAIN_SETS, f"train_set must be one of {TRAIN_SETS}, got {train_set!r}")
        _req(S is not None, "cs_step: CS_FIX_TRAIN needs the sets")
    if S is not None:
        _req_sets(S, T.n(), "cs_step")
    ctx.lib.mggcn_cs_step_f32(ctx.stream(0), T.buffer(), R.buffer(), S.buffer() if S is not None else None, T.n(), T.m(),
                              alpha, beta, lo, hi, int(train_set), int(flags), out.buffer())


def cs_correct(ctx: context, P: dn_matrix, E: dn_matrix, Y: Optional[dn_matrix], S: Optional[dn_matrix], train_set: int,
               sums_device, inv_T: float, scale: float, flags: int, out: Optional[dn_matrix] = None) -> None:
    """out = P + s E row by row, in place on P by default (mggcn_cs_correct_f32): s = (sums_device[0] inv_T) / sum |E[i]|
    with CS_AUTOSCALE (1 where that is not finite or above 1000), else ``scale``; with CS_SET_LABELS the rows with
    S == train_set are onehot(Y)."""
    if out is None:
        out = P
    _req_cs([("P", P), ("E", E), ("out", out)], "cs_correct")
    _req(flags & ~(CS_AUTOSCALE | CS_SET_LABELS) == 0, f"cs_correct: unknown flags {flags:#x}")
    if flags & CS_AUTOSCALE:
        _req(sums_device is not None and sums_device.numel() >= 1, "cs_correct: CS_AUTOSCALE needs the residual's sum")
        _req(math.isfinite(inv_T) and inv_T > 0, f"cs_correct: inv_T must be positive and finite, got {inv_T}")
    else:
        _req(math.isfinite(scale), f"cs_correct: scale must be finite, got {scale}")
    if flags & CS_SET_LABELS:
        _req(Y is not None and S is not None, "cs_correct: CS_SET_LABELS needs the labels and the sets")
        _req_cs_labels(Y, S, P.n(), train_set, "cs_correct")
    ctx.lib.mggcn_cs_correct_f32(ctx.stream(0), P.buffer(), E.buffer(), Y.buffer() if Y is not None else None,
                                 S.buffer() if S is not None else None, P.n(), P.m(), int(train_set),
                                 sums_device.data_ptr() if sums_device is not None else None, inv_T, scale, int(flags),
                                 out.buffer())


def adam_fused(ctx: context, param: dn_matrix, grad: dn_matrix, m: dn_matrix, v: dn_matrix, lr: float,
               beta1: float, beta2: float, weight_decay: float, c1: float, c2: float, eps: float) -> None:
    _req(param.shape() == grad.shape() == m.shape() == v.shape(), "shape mismatch")
    ctx.lib.mggcn_adam_fused_f32(ctx.stream(0), param.buffer(), grad.buffer(), m.buffer(), v.buffer(), lr,
                                 beta1, beta2, weight_decay, c1, c2, eps, param.size())


class adam_table:
    """Device table of every (param, grad, m, v) quadruple of a model for mggcn_adam_multi_f32: built once
    (the buffers of a model never move), one launch per epoch instead of two per layer."""

    def __init__(self, ctx: context, tensors) -> None:
        """tensors: [(param, grad, m, v, weight_decay_on)] of dn_matrix"""
        torch = __import__("torch")
        dt = np.dtype([("param", "<u8"), ("grad", "<u8"), ("m", "<u8"), ("v", "<u8"), ("size", "<u8"),
                       ("wd", "<f4"), ("first_block", "<u4")])
        assert dt.itemsize == 48
        tab = np.zeros(len(tensors), dtype=dt)
        blocks = 0
        for k, (p, g, m, v, wd) in enumerate(tensors):
            _req(p.shape() == g.shape() == m.shape() == v.shape(), "shape mismatch")
            tab[k] = (p.buffer(), g.buffer(), m.buffer(), v.buffer(), p.size(), wd, blocks)
            blocks += ctx.lib.mggcn_adam_multi_blocks(p.size())
        self.n, self.blocks = len(tensors), blocks
        self.keep = tensors                                       # the table holds raw pointers
        self.dev = torch.from_numpy(tab.view(np.uint8).copy()).to(ctx.device)
        torch.cuda.current_stream(self.dev.device).synchronize()

    def step(self, ctx: context, lr: float, beta1: float, beta2: float, c1: float, c2: float, eps: float) -> None:
        ctx.lib.mggcn_adam_multi_f32(ctx.stream(0), self.dev.data_ptr(), self.n, self.blocks, lr, beta1, beta2, c1, c2, eps)
