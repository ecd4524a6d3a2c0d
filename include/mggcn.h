/*
 * mggcn.h -- C ABI of libmggcn_hip.so, the MI355X (gfx950) engine behind the
 * MG-GCN hot path: CSR SpMM aggregation (A.H forward, A^T.dH backward), the
 * dense H.W transform and the element-wise / loss / optimiser kernels of one
 * training epoch, plus the host-side graph preprocessing that feeds them.
 *
 * The reference has no FFI: it is a header-only C++ template library whose device
 * code is reached through forward-declared launchers
 *     void f(cudaStream_t, T* ..., size_t size, size_t m, ...)
 * (src/cuda_utils.hpp:398-468  <->  src/cuda_utils.cu:229-451) and through
 * cusparseSpMM / cublasSgemm handles bound to a stream (src/matrix.hpp:86-87).
 * That host-header <-> device-TU seam is the boundary this file replaces: every
 * entry point below names the reference interface it stands in for.
 *
 * Conventions (same as the reference):
 *  - plain pointers and sizes; no HIP, torch or C++ types.  A stream is an opaque
 *    void* (a hipStream_t; NULL = the device's default stream).  torch users pass
 *    torch.cuda.current_stream().cuda_stream.
 *  - enqueue-only: nothing here synchronises or allocates on the launch path
 *    (the *_create / *_malloc / *_host functions are the exceptions, by name).
 *  - the callee never takes ownership of a buffer.
 *  - fail-fast: a HIP error or a violated precondition prints
 *    "MGGCN ... failed at file:line" and calls exit(EXIT_FAILURE), exactly like
 *    CHECK_CUDA / CHECK_CUSPARSE (src/mg_gcn.hpp:31-68).  No status codes.
 *  - dense matrices are row-major fp32 with an explicit leading dimension
 *    (CUSPARSE_ORDER_ROW, src/matrix.hpp:508); CSR is u32 indptr / u32 indices /
 *    f32 values, zero-based (src/matrix.hpp:217-221, :271).
 *  - "size" is the element count n*m and "m" the row width, as in the launchers.
 *
 * All citations are relative to the reference tree (GT-TDAlab/MG-GCN).
 */
#ifndef MGGCN_H_
#define MGGCN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGGCN_ABI_VERSION 1

typedef void *mggcn_stream_t; /* hipStream_t */
typedef void *mggcn_event_t;  /* hipEvent_t  */

/* ======================================================================== *
 * Runtime: the per-GPU `context` (src/matrix.hpp:69-158)
 * ======================================================================== */
int mggcn_abi_version(void);
/* cudaGetDeviceCount / cudaSetDevice (context::set, src/matrix.hpp:90-92) */
int mggcn_device_count(void);
void mggcn_set_device(int device);
int mggcn_get_device(void);
/* context::sync = cudaDeviceSynchronize (src/matrix.hpp:94-97) */
void mggcn_device_synchronize(void);
/* stream_create(i, priority) (src/matrix.hpp:53-60): high_priority != 0 asks for the
 * highest priority the device offers (the reference's comm stream), 0 for the lowest
 * (its compute stream). */
mggcn_stream_t mggcn_stream_create(int high_priority);
void mggcn_stream_destroy(mggcn_stream_t stream);
/* Frees the per-(device, stream) reduction scratch that mggcn_abssum_f32 / the fused loss / mggcn_cs_residual_f32, and the partials that
 * mggcn_layer_norm_backward_f32, mggcn_gated_skip_backward_f32, mggcn_label_input_backward_f32 and mggcn_gat_scores_backward_f32, allocate on first use (synchronises that stream).  mggcn_stream_destroy calls it; a
 * host layer that brings its own streams (e.g. torch's) calls it when it drops one. */
void mggcn_stream_release_scratch(mggcn_stream_t stream);
void mggcn_stream_synchronize(mggcn_stream_t stream);
/* event_create / context::record / context::wait / context::measure
 * (src/matrix.hpp:62-67, :107-117, :138-144) */
mggcn_event_t mggcn_event_create(void);
void mggcn_event_destroy(mggcn_event_t event);
void mggcn_event_record(mggcn_event_t event, mggcn_stream_t stream);
void mggcn_stream_wait_event(mggcn_stream_t stream, mggcn_event_t event);
void mggcn_event_synchronize(mggcn_event_t event);
float mggcn_event_elapsed_ms(mggcn_event_t begin, mggcn_event_t end);
/* cuda_malloc / cudaFree deleter (src/mg_gcn.hpp:84-90).  The reference's
 * cudaMallocManaged buffers (src/mg_gcn.hpp:74-82) become device memory plus an
 * explicit pinned host mirror: managed memory needs XNACK, which this pool lacks. */
void *mggcn_malloc(size_t bytes);
void mggcn_free(void *device_ptr);
void *mggcn_malloc_host(size_t bytes);
void mggcn_free_host(void *host_ptr);
/* cudaMemcpyAsync / cudaMemsetAsync (dn_matrix::copy_to, ::zero, src/matrix.hpp:547-566) */
void mggcn_memcpy_h2d(void *dst, const void *src, size_t bytes, mggcn_stream_t stream);
void mggcn_memcpy_d2h(void *dst, const void *src, size_t bytes, mggcn_stream_t stream);
void mggcn_memcpy_d2d(void *dst, const void *src, size_t bytes, mggcn_stream_t stream);
void mggcn_memset_zero(void *dst, size_t bytes, mggcn_stream_t stream);

/* ======================================================================== *
 * SpMM  C = alpha * A * B + beta * C     (the hot kernel)
 * replaces matmul(context, csr_matrix, dn_matrix B, dn_matrix C, ext_buffer,
 * alpha, beta, alg) = cusparseSpMM op N/N (src/cuda_utils.hpp:15-32) and its
 * workspace query get_matmul_buffer (src/cuda_utils.hpp:94-102).
 * ======================================================================== */

/* The "external buffer" of the reference becomes a plan, built once per matrix from
 * the HOST copy of the CSR arrays; it holds only device memory it allocated itself:
 *  - row-split metadata that load-balances heavy-tailed degree distributions (rows
 *    longer than the split threshold are cut into work items whose partial sums are
 *    combined in a fixed order -> bitwise reproducible) and the partial-sum workspace
 *    for feature widths up to max_d;
 *  - when host_indices / host_values are given and the matrix is large (>= 2^20
 *    non-zeros), the column-panel "sweep" form: the non-zeros re-cut into equal-work
 *    per-wave streams sorted by column panel, so that every wave on the chip walks B
 *    in the same order and the active panel stays L2-resident (a private device copy
 *    of the matrix, 8 B per non-zero).  Pass NULL for both to skip it.
 * The arrays later passed to mggcn_spmm_csr_f32 with a plan must hold the matrix the
 * plan was built for (the sweep form reads its own copy).
 * No input order is assumed: rows may or may not be sorted by column (heavy rows are cut into interleaved slices), and
 * a vertex order with locality (an unpermuted community graph: most non-zeros near the diagonal) is detected at plan
 * time -- the sweep form then works on a fixed pseudo-random relabelling of the columns and copies B into a plan-owned
 * scratch in that order at the start of every call (the caller's B is never written).
 * Re-entrancy: every entry point of this header is enqueue-only and may be called from any stream, but a
 * PLAN owns mutable device scratch (partial-sum slots of sliced rows, the re-pitched copy of B of the narrow
 * form): one plan may be in flight on ONE stream at a time.  Calls on the same stream are ordered and safe;
 * to multiply by the same matrix on two streams concurrently, build two plans.  (mggcn_abssum_f32 keeps its
 * reduction scratch per stream: concurrent sums on different streams are safe.)
 * Plan CREATION is re-entrant: several host threads may build plans at the same time (each thread makes its target
 * device current first, mggcn_set_device) -- the host layers build a model's four plans side by side that way. */
typedef struct mggcn_spmm_plan mggcn_spmm_plan;

mggcn_spmm_plan *mggcn_spmm_plan_create(uint32_t n_rows, uint32_t n_cols,
                                        const uint32_t *host_indptr, const uint32_t *host_indices,
                                        const float *host_values, uint32_t max_d);
/* Same, with the feature width the plan will mostly be used at (the reference sizes its cuSPARSE
 * workspace per (A, B, C) triple as well, src/cuda_utils.hpp:94-102, and caches it per width,
 * src/gcn.hpp:28-31).  d_hint in 1..64 builds the sweep form for NARROW rows (four entries per
 * gather instruction, B re-pitched to 16-byte rows in a plan-owned scratch); 0 or > 64 is the
 * form mggcn_spmm_plan_create builds.  Any plan serves any width <= max_d; the hint only picks
 * which one is fast. */
mggcn_spmm_plan *mggcn_spmm_plan_create_for(uint32_t n_rows, uint32_t n_cols,
                                            const uint32_t *host_indptr, const uint32_t *host_indices,
                                            const float *host_values, uint32_t max_d, uint32_t d_hint);
void mggcn_spmm_plan_destroy(mggcn_spmm_plan *plan);
/* A caller that builds n plans side by side (one host thread each) says so before it starts: every builder then threads
 * its own passes over cores / n instead of all the cores (MGGCN_HOST_THREADS in the environment still wins).  Set it back
 * to 1 afterwards.  Process-wide. */
void mggcn_spmm_plan_concurrent_builders(uint32_t n);
/* Plans built from now on leave at least n compute units' worth of wave slots free in EVERY launch round: for SpMMs that run
 * while a collective kernel (RCCL) shares the device -- a round of exactly the resident set would end in a second, nearly empty
 * pass for the workgroups the foreign kernel displaced (+57 % measured).  A minimum, not a cut: a matrix
 * whose tasks leave that room anyway (one round, not full) keeps the full round size; only plans whose rounds would be full are
 * built on smaller rounds (fewer waves in flight: -5 % when nobody shares the device).  The distributed host layers set 12
 * around their plan builds and 0 afterwards; MGGCN_SPMM_RESERVED_CUS in the environment overrides.  Process-wide. */
void mggcn_spmm_plan_reserved_cus(uint32_t n);
/* introspection (tests, DESIGN.md figures) */
uint32_t mggcn_spmm_plan_num_items(const mggcn_spmm_plan *plan);
uint32_t mggcn_spmm_plan_num_split_rows(const mggcn_spmm_plan *plan);
uint32_t mggcn_spmm_plan_num_sweep_tasks(const mggcn_spmm_plan *plan); /* 0: no sweep form */
uint32_t mggcn_spmm_plan_num_launches(const mggcn_spmm_plan *plan, uint32_t d); /* kernel launches per SpMM call at width d */
size_t mggcn_spmm_plan_bytes(const mggcn_spmm_plan *plan);
uint32_t mggcn_spmm_plan_num_slices(const mggcn_spmm_plan *plan);      /* column slices of the sweep form (0: none) */
/* One line of text with what the plan builder measured and decided: form (rowsplit / sweep / sweep-narrow), share of the
 * non-zeros in the 1 % most popular columns and the flag derived from it, mean (panel,row) run length, column slices,
 * device bytes, host build seconds, then per slice: tasks, launch rounds, panel rows, run padding, lanes per entry,
 * padded entry count.  snprintf semantics (returns the length written).  MGGCN_SPMM_PLAN_LOG=1 in the environment
 * prints the same line to stderr whenever a plan is created.  The tuning knobs (MGGCN_SPMM_*) are read once, here,
 * never on the launch path. */
int mggcn_spmm_plan_describe(const mggcn_spmm_plan *plan, char *out, size_t cap);
/* diagnostics (experiments only): n_blocks workgroups of 256 threads that hold their wave slots until *stop_flag (device memory, or mapped
 * pinned host memory) is non-zero or max_microseconds have passed -- a stand-in for the channels of a collective
 * kernel sharing the device with the SpMM (profiles/experiments/coresident_r04.py). */
void mggcn_debug_occupy_cus(mggcn_stream_t stream, uint32_t n_blocks, uint32_t max_microseconds, const uint32_t *stop_flag);
/* diagnostics: with MGGCN_SPMM_STAMPS=1 in the environment at plan creation the d >= 96 sweep kernel records, per
 * one-wave task of column slice `slice`, {start, end} on the 100 MHz constant clock and {HW_ID << 32 | blockIdx << 4 | XCC id} of
 * its LAST launch; this copies them out (3 x u64 per task, blocking) and returns the task count.  Never set in a
 * timed run. */
uint32_t mggcn_spmm_plan_read_stamps(const mggcn_spmm_plan *plan, uint32_t slice, uint64_t *host_out,
                                     uint32_t capacity_tasks);

/* flags */
#define MGGCN_SPMM_DEFAULT 0u
/* fused epilogue: C = leaky_relu(alpha*A*B + beta*C, slope) -- folds the
 * leaky_relu_forward launch of gcn_layer::operator() (src/gcn.hpp:447-452) */
#define MGGCN_SPMM_LEAKY_RELU 1u

/* A: n_rows x n_cols CSR (device pointers), B: n_cols x d (ldb >= d), C: n_rows x d
 * (ldc >= d).  beta == 0 never reads C.  C must not alias B.  plan may be NULL
 * (one wave per row in row order: correct for any input, slow on skewed degrees).
 * slope is only read with MGGCN_SPMM_LEAKY_RELU.
 * A non-finite row of B reaches exactly the rows of C that have an entry in its column, possibly as NaN where Inf is
 * expected: the sweep form pads runs with zero-valued copies of a real entry, and 0 * Inf = NaN. */
void mggcn_spmm_csr_f32(mggcn_stream_t stream, const mggcn_spmm_plan *plan, uint32_t n_rows,
                        uint32_t n_cols, const uint32_t *indptr, const uint32_t *indices,
                        const float *values, const float *B, size_t ldb, float *C, size_t ldc,
                        uint32_t d, float alpha, float beta, uint32_t flags, float slope);

/* bf16 aggregation: the gathered operand B stored as bf16 (uint16_t bit patterns), half the bytes per row.
 *   C = alpha * A * widen(B) + beta * C
 * Everything else is mggcn_spmm_csr_f32's contract: A's values, the products, the sums, C and the fused
 * leaky-ReLU epilogue are fp32; ldb is counted in ELEMENTS (ldb >= d); beta == 0 never reads C; C must not
 * alias B; plan may be NULL.  The same plan serves both entries (a plan built for mggcn_spmm_csr_f32 is used as
 * is; the bf16 copies of B that a narrow or relabelled plan makes are allocated by the first bf16 call that
 * needs one).  Every form multiplies the exactly widened bf16 values in the order the fp32 form uses, so the
 * result equals mggcn_spmm_csr_f32 on the widened B bit for bit, with the same plan and equally aligned
 * operands. */
void mggcn_spmm_csr_bf16(mggcn_stream_t stream, const mggcn_spmm_plan *plan, uint32_t n_rows,
                         uint32_t n_cols, const uint32_t *indptr, const uint32_t *indices,
                         const float *values, const uint16_t *B, size_t ldb, float *C, size_t ldc,
                         uint32_t d, float alpha, float beta, uint32_t flags, float slope);
/* dst = bf16(src): n_rows x n_cols, row-major, leading dimensions in elements (ld_src, ld_dst >= n_cols).
 * Round to nearest even; a NaN stays a NaN, overflow goes to +-inf.  src and dst must not overlap. */
void mggcn_convert_f32_bf16(mggcn_stream_t stream, const float *src, size_t ld_src, uint16_t *dst, size_t ld_dst,
                            size_t n_rows, size_t n_cols);
/* dst[k, 0:d] = src[indices[k], 0:d] on bf16 bit patterns: mggcn_gather_rows_f32 for a shard that has already been
 * rounded (the halo pack of the row-partitioned model with bf16 aggregation).  A pure copy: every bit pattern
 * survives.  Leading dimensions in ELEMENTS (ld_src, ld_dst >= d); indices: device, uint32; src and dst must not
 * overlap.  16 bytes per lane when d and both leading dimensions are multiples of 8 and both bases 16-byte aligned,
 * 4 bytes when all are even and 4-byte aligned, 2 bytes otherwise.  n_indices == 0 or d == 0: no launch. */
void mggcn_gather_rows_bf16(mggcn_stream_t stream, const uint16_t *src, size_t ld_src, const uint32_t *indices,
                            size_t n_indices, uint32_t d, uint16_t *dst, size_t ld_dst);

/* ======================================================================== *
 * Dense GEMM  C = alpha * op(A) * op(B) + beta * C, row-major  (the MFMA path)
 * replaces matmul(context, dn A, dn B, dn C, alpha, beta, A_T, B_T) =
 * cublasSgemm with swapped operands (src/cuda_utils.hpp:149-172).
 * op(A) is M x K, op(B) is K x N; lda/ldb/ldc are the STORED leading dimensions.
 * fp32 in, fp32 accumulate on v_mfma_f32_32x32x2_f32 (exact fp32 products).
 * Tall reductions (K >> M*N, e.g. G_W = X^T G) are split over K; the partial
 * sums are combined in a fixed order inside `workspace` (bitwise reproducible).
 * workspace may be NULL when mggcn_gemm_workspace_bytes(...) == 0.
 * ======================================================================== */
size_t mggcn_gemm_workspace_bytes(int trans_a, int trans_b, uint32_t M, uint32_t N, uint32_t K);
void mggcn_gemm_f32(mggcn_stream_t stream, int trans_a, int trans_b, uint32_t M, uint32_t N,
                    uint32_t K, float alpha, const float *A, size_t lda, const float *B, size_t ldb,
                    float beta, float *C, size_t ldc, void *workspace, size_t workspace_bytes);
/* C = alpha * op(A) * op(B) + 1 * bias^T   (bias: N floats added to every row of C).
 * The reference's linear forward is broadcast_rows(b -> XW) followed by an sgemm with beta = 1
 * (src/gcn.hpp:116-123); this is the same sum in one pass: no broadcast kernel, no read of C.
 * Workspace as for mggcn_gemm_f32. */
void mggcn_gemm_bias_f32(mggcn_stream_t stream, int trans_a, int trans_b, uint32_t M, uint32_t N,
                         uint32_t K, float alpha, const float *A, size_t lda, const float *B, size_t ldb,
                         const float *bias, float *C, size_t ldc, void *workspace, size_t workspace_bytes);
/* C = alpha * A^T * B  AND  colsum = alpha * 1^T B  in one pass (A stored [K x M], B stored [K x N]).
 * The reference's linear::backward runs G_b = 1^T G as an sgemm with a ones vector and then G_W = X^T G
 * (src/gcn.hpp:125-134): two passes over G.  Here the workgroups of the first M-tile add up the B tiles they stage for
 * the MFMAs anyway -- no second read of G, no extra launch.  Split-K slabs carry the sums as one extra row; combined in
 * the same fixed order (reproducible).  Workspace: mggcn_gemm_tn_colsum_workspace_bytes. */
size_t mggcn_gemm_tn_colsum_workspace_bytes(uint32_t M, uint32_t N, uint32_t K);
void mggcn_gemm_tn_colsum_f32(mggcn_stream_t stream, uint32_t M, uint32_t N, uint32_t K, float alpha, const float *A,
                              size_t lda, const float *B, size_t ldb, float *C, size_t ldc, float *colsum,
                              void *workspace, size_t workspace_bytes);
/* C = (alpha * op(A) * op(B)) .* (Z > 0 ? 1 : slope)   (Z: M x N, ldz >= N; C is never read).
 * Folds the NEXT leaky_relu_backward launch into the GEMM that produces its gradient operand: the reference
 * runs G_out = G . W^T in layer i+1 (src/gcn.hpp:135-137) and then, in layer i, leaky_relu_backward(Z_i, G_out)
 * (src/gcn.hpp:462-468, src/cuda_utils.cu:33-38) -- a pass that reads Z_i and G_out and writes T.  Z_i is layer
 * i+1's own input X, so the mask is applied on the accumulator tile in this GEMM's epilogue: one read of Z, no
 * extra pass, no extra write.  Same products and the same single multiply as the two launches -> bitwise equal. */
void mggcn_gemm_lrelu_bwd_f32(mggcn_stream_t stream, int trans_a, int trans_b, uint32_t M, uint32_t N,
                              uint32_t K, float alpha, const float *A, size_t lda, const float *B, size_t ldb,
                              const float *Z, size_t ldz, float slope, float *C, size_t ldc, void *workspace,
                              size_t workspace_bytes);

/* ======================================================================== *
 * Element-wise / row kernels: one entry point per live launcher of
 * src/cuda_utils.cu (declared src/cuda_utils.hpp:398-468).  Same argument
 * order as the launcher it replaces, stream first.  In-place use (out == in)
 * is legal wherever the reference uses it (src/gcn.hpp:449, :464).
 * ======================================================================== */
/* leaky_relu_forward  (src/cuda_utils.cu:26-31, :229-234)  out = max(in, alpha*in) */
void mggcn_leaky_relu_forward_f32(mggcn_stream_t stream, const float *in, float *out, size_t size,
                                  float alpha);
/* leaky_relu_backward (src/cuda_utils.cu:33-38, :236-241)  G_out = in > 0 ? G_in : alpha*G_in */
void mggcn_leaky_relu_backward_f32(mggcn_stream_t stream, const float *in, const float *G_in,
                                   float *G_out, size_t size, float alpha);
/* broadcast_rows (src/cuda_utils.cu:40-51, :243-248)  mat[i,:] = row (discard) or += row */
void mggcn_broadcast_rows_f32(mggcn_stream_t stream, const float *row, float *mat, size_t size,
                              size_t m, int discard);
/* scale_rows (src/cuda_utils.cu:75-79, :264-269)  mat[i,:] /= scalar[i] */
void mggcn_scale_rows_f32(mggcn_stream_t stream, float *mat, const float *scalar, size_t size,
                          size_t m);
/* max_rows (src/cuda_utils.cu:95-104, :271-276) */
void mggcn_max_rows_f32(mggcn_stream_t stream, const float *mat, float *maxs, size_t size, size_t m);
/* max_row_indices (src/cuda_utils.cu:119-133, :285-290): first maximum wins */
void mggcn_max_row_indices_f32(mggcn_stream_t stream, const float *mat, int32_t *maxs, size_t size,
                               size_t m);
/* index_log_rows (src/cuda_utils.cu:142-150, :299-304)  values[i] = log(mat[i, indices[i]]) */
void mggcn_index_log_rows_f32(mggcn_stream_t stream, const float *mat, const int32_t *indices,
                              float *values, size_t size, size_t m);
/* add_indexed_rows (src/cuda_utils.cu:159-164, :313-319)  mat[i, indices[i]] += alpha */
void mggcn_add_indexed_rows_f32(mggcn_stream_t stream, float *mat, const int32_t *indices,
                                float alpha, size_t size, size_t m);
/* is_equal (src/cuda_utils.cu:180-184, :336-341)  out[i] = (a[i] == b[i]) */
void mggcn_is_equal_i32(mggcn_stream_t stream, const int32_t *a, const int32_t *b, float *out,
                        size_t size);
/* subtract_rows_exp (src/cuda_utils.cu:192-200, :350-355)  out = exp(mat - scalar[row]) */
void mggcn_subtract_rows_exp_f32(mggcn_stream_t stream, const float *mat, const float *scalar,
                                 float *out, size_t size, size_t m);
/* axpby (src/cuda_utils.cu:81-86, :364-369)   B = alpha*A + beta*B */
void mggcn_axpby_f32(mggcn_stream_t stream, const float *A, float *B, float alpha, float beta,
                     size_t size);
/* aaxpby (src/cuda_utils.cu:88-93, :371-376)  B = alpha*A*A + beta*B */
void mggcn_aaxpby_f32(mggcn_stream_t stream, const float *A, float *B, float alpha, float beta,
                      size_t size);
/* adam_final (src/cuda_utils.cu:208-218, :378-383)  p -= (lr/c1) * m / (sqrt(v/c2) + eps) */
void mggcn_adam_final_f32(mggcn_stream_t stream, float *param, const float *m, const float *v,
                          float lr, float c1, float c2, float eps, size_t size);
/* cublasSaxpy   (src/cuda_utils.hpp:326-340)  B += alpha*A */
void mggcn_axpy_f32(mggcn_stream_t stream, const float *A, float *B, float alpha, size_t size);
/* cublasSscal   (src/cuda_utils.hpp:373-381)  mat *= scalar */
void mggcn_scale_mat_f32(mggcn_stream_t stream, float *mat, float scalar, size_t size);
/* Dropout with a mask that is never stored (opt-in; the reference has no dropout).  The matrix is [size / m x m],
 * contiguous; in == out is allowed; row0 is the GLOBAL index of its first row.  Element (global row r, column c):
 *   words = Philox4x32-10(counter = (c >> 2, r & 0xffffffff, r >> 32, dropout_stream), key = (seed & 0xffffffff, seed >> 32))
 *   out   = words[c & 3] >= threshold ? in * scale : +0.0f      (+0.0 also where in is NaN or +-inf; one fp32 multiply)
 * with the usual constants (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85; ten rounds).
 * The host computes threshold = (uint32) floor(p * 2^32) and scale = (float)(1 / (1 - p)) in double for 0 <= p < 1; the
 * kernel never sees p.  The mask is a pure function of (seed, dropout_stream, r, c): it does not depend on the grid, on
 * the alignment of the pointers (a float4 path when m % 4 == 0 and both are 16-byte aligned, an element path otherwise)
 * or on row0's split of the rows -- the call on rows [a, b) with row0 = a gives rows [a, b) of the whole call -- and the
 * backward pass of dropout is the same call on the gradient.  size == 0 returns; m > 0 and size % m == 0. */
void mggcn_dropout_f32(mggcn_stream_t stream, const float *in, float *out, size_t size, size_t m, uint64_t row0,
                       uint32_t threshold, float scale, uint64_t seed, uint32_t dropout_stream);
/* Layer normalisation over the rows of a contiguous [n_rows x m] matrix, 1 <= m <= MGGCN_LN_MAX_WIDTH (opt-in; the
 * reference has no normalisation).  Forward, per row:
 *   mean = sum(x) / m;  var = sum((x - mean)^2) / m  (biased, two passes);  rstd = 1 / sqrt(var + eps)
 *   xhat = (x - mean) * rstd;  z = xhat * gamma + beta;  y = flags & MGGCN_LN_LEAKY_RELU ? leaky_relu(z, 0.01) : z
 * and y, xhat [n_rows x m] and rstd [n_rows] are written; gamma and beta hold m floats; x == y is allowed.  Backward:
 *   dz = flags & MGGCN_LN_LEAKY_RELU ? (act > 0 ? G : 0.01 G) : G   (act is a sign source only and may be null without the flag)
 *   g = dz . gamma;  G_in = rstd (g - mean(g) - xhat mean(g . xhat));  G_gamma[c] = sum_r dz xhat;  G_beta[c] = sum_r dz
 * G_in may be G or act.  The column sums use no atomics: per-workgroup partials in a per-(device, stream) scratch (grown on
 * first use, freed by mggcn_stream_release_scratch) are added in a fixed order, so two calls on the same input give the
 * same bits.  A row's results do not depend on the other rows of the call: rows [a, b) alone give the bits they have in
 * the whole call, for the same width and pointer alignment (m % 4 == 0 with every operand 16-byte aligned takes a float4 path,
 * anything else an element path).  n_rows == 0 returns; the backward still writes zeros to G_gamma / G_beta. */
#define MGGCN_LN_LEAKY_RELU 1u
#define MGGCN_LN_MAX_WIDTH 1024u
void mggcn_layer_norm_forward_f32(mggcn_stream_t stream, const float *x, float *y, float *xhat, float *rstd,
                                  const float *gamma, const float *beta, size_t n_rows, size_t m, float eps,
                                  uint32_t flags);
void mggcn_layer_norm_backward_f32(mggcn_stream_t stream, const float *G, const float *act, const float *xhat,
                                   const float *rstd, const float *gamma, float *G_in, float *G_gamma, float *G_beta,
                                   size_t n_rows, size_t m, uint32_t flags);
/* The skip connection of an attention layer (opt-in; PyG's GATConv(residual=True) and TransformerConv(beta=True)), row by
 * row over [n_rows x m] operands, 1 <= m <= MGGCN_GS_MAX_WIDTH.  o is the attention output, r the skip linear's output, w
 * the gate's parameter ([3 x m] contiguous), gate one float per row.  Forward:
 *   without MGGCN_GS_GATE  t = o + r
 *   with    MGGCN_GS_GATE  s = sum_c (w[0,c] o[c] + w[1,c] r[c] + w[2,c] (o[c] - r[c]));  g = 1 / (1 + exp(-s));
 *                          t = g r + (1 - g) o;  gate[row] = g
 *   y = flags & MGGCN_GS_LEAKY_RELU ? leaky_relu(t, 0.01) : t
 * Backward, with dy = flags & MGGCN_GS_LEAKY_RELU ? (act > 0 ? G : 0.01 G) : G  (act is a sign source only -- the forward's y
 * -- and may be null without the flag):
 *   without MGGCN_GS_GATE  G_o = G_r = dy  (o, r, w, gate and G_w are not read or written and may be null)
 *   with    MGGCN_GS_GATE  dg = sum_c dy[c] (r[c] - o[c]);  ds = dg g (1 - g);
 *                          G_o[c] = (1 - g) dy[c] + ds (w[0,c] + w[2,c]);  G_r[c] = g dy[c] + ds (w[1,c] - w[2,c]);
 *                          G_w[0,c] = sum_i ds_i o_i[c];  G_w[1,c] = sum_i ds_i r_i[c];  G_w[2,c] = sum_i ds_i (o_i[c] - r_i[c])
 * Every [n_rows x m] operand has a leading dimension of its own (ld >= m), so r may be a column block of a wider matrix.
 * The sigmoid is evaluated from exp(-|s|): no finite s gives NaN, and g is exactly 1 or 0 where fp32 saturates (then ds = 0).
 * Aliasing: y aliases neither o nor r (the backward pass reads both).  G_o may be G or act.  Without MGGCN_GS_GATE G_r may be
 * G_o (one store); with it G_r is distinct from every other operand and G_o from o and r.  w and gate need the flag and
 * are null without it; with it they and G_w must not be null.
 * A row's y, gate, G_o and G_r depend on that row alone: rows [a, b) alone give the bits they have in the whole call, for
 * the same width and alignment (m % 4 == 0 with every operand 16-byte aligned and every leading dimension a multiple of 4
 * takes a float4 path, anything else an element path).  G_w uses no atomics: per-workgroup partials in the per-(device,
 * stream) scratch of mggcn_layer_norm_backward_f32 are added in a fixed order, so the same arguments give the same bits on
 * every call.  n_rows == 0 launches nothing in the forward; the backward still writes zeros to G_w (with MGGCN_GS_GATE). */
#define MGGCN_GS_GATE 1u
#define MGGCN_GS_LEAKY_RELU 2u
#define MGGCN_GS_MAX_WIDTH 1024u
void mggcn_gated_skip_forward_f32(mggcn_stream_t stream, const float *o, size_t ldo, const float *r, size_t ldr,
                                  const float *w, float *y, size_t ldy, float *gate, size_t n_rows, size_t m, uint32_t flags);
void mggcn_gated_skip_backward_f32(mggcn_stream_t stream, const float *G, size_t ldg, const float *act, size_t lda,
                                   const float *o, size_t ldo, const float *r, size_t ldr, const float *w, const float *gate,
                                   float *G_o, size_t ldgo, float *G_r, size_t ldgr, float *G_w, size_t n_rows, size_t m,
                                   uint32_t flags);
/* Masked label inputs of the attention models (opt-in; the "label trick" of UniMP): a trained table E [n_classes x width]
 * whose row E[y_i] is added to row i of layer 0's Z for the training rows that are FED this forward, and its gradient.
 * Both calls walk the training rows only, as three device lists the host builds once: rows[t], the local row numbers, and
 * cls[t], their classes, t < n_train, sorted by (class, row) without duplicates, and cls_ptr[n_classes + 1], the segment
 * of each class (cls_ptr[0] = 0, cls_ptr[n_classes] = n_train).  Entry t is fed iff
 *   feed_all != 0, or  Philox4x32-10(counter = (0xFFFFFFFF, r & 0xffffffff, r >> 32, epoch),
 *                                    key = (seed & 0xffffffff, seed >> 32)).w[0] < threshold,   r = row0 + rows[t]
 * (threshold = (uint32) floor(rate * 2^32), from the host).  The mask is never stored: both calls regenerate it, it does not
 * depend on how the rows are split (row0 is the global number of local row 0), and the first counter word is a column
 * group mggcn_dropout_f32 never draws, so a seed shared with dropout shares no bits.
 *   forward    fed: Z[rows[t], :] += E[cls[t], :], one fp32 add per element, and S_out[rows[t]] = fed_set;
 *              otherwise S_out[rows[t]] = kept_set.  S_out may be null.  Rows that are not listed are not touched, in Z or
 *              in S_out; every listed row of S_out is written on every call.
 *   backward   G_E[c, :] = the sum of G_Z[rows[t], :] over the fed entries of class c; a class without one gets +0.0
 *              (written, not skipped).  No atomics: each segment is cut into chunks of 64 entries, whatever the grid is,
 *              one partial per chunk goes to the per-(device, stream) scratch of mggcn_layer_norm_backward_f32 and the
 *              partials of a class are added in a fixed order, so the same arguments give the same bits on every call.
 * Z and G_Z have n_rows rows; an entry whose row is not below n_rows or whose class is not below n_classes is skipped and
 * never dereferenced.  1 <= n_classes <= MGGCN_LABEL_INPUT_MAX_CLASSES, 1 <= width <= MGGCN_LABEL_INPUT_MAX_WIDTH (three
 * times MGGCN_GAT_MAX_WIDTH: the Z of a dot-product layer), every leading dimension >= width.  width % 4 == 0 with every
 * dense operand 16-byte aligned and every leading dimension a multiple of 4 takes a float4 path, anything else an element
 * path.  n_train == 0: the forward launches nothing, the backward writes +0.0 to all of G_E (the lists may be null). */
#define MGGCN_LABEL_INPUT_MAX_CLASSES 256u
#define MGGCN_LABEL_INPUT_MAX_WIDTH 3072u
void mggcn_label_input_forward_f32(mggcn_stream_t stream, const uint32_t *rows, const uint32_t *cls, size_t n_train,
                                   const float *E, size_t lde, size_t n_classes, size_t width, uint32_t threshold,
                                   int feed_all, uint64_t seed, uint32_t epoch, uint64_t row0, int32_t kept_set,
                                   int32_t fed_set, float *Z, size_t ldz, size_t n_rows, int32_t *S_out);
void mggcn_label_input_backward_f32(mggcn_stream_t stream, const uint32_t *rows, const uint32_t *cls,
                                    const uint32_t *cls_ptr, size_t n_train, size_t n_classes, size_t width,
                                    uint32_t threshold, int feed_all, uint64_t seed, uint32_t epoch, uint64_t row0,
                                    const float *G_Z, size_t ldg, size_t n_rows, float *G_E, size_t ldge);
/* Correct and Smooth (opt-in post-processing of a trained model's logits; Huang et al. 2021, PyG's CorrectAndSmooth): the
 * row kernels around the two label-propagation loops, whose products are mggcn_spmm_csr_f32's.  Every dense operand is
 * contiguous [n_rows x m] fp32, 1 <= m <= MGGCN_CS_MAX_WIDTH; Y (labels) and S (sets) are n_rows int32; a training row is
 * one with S[i] == train_set.  No atomics: the same arguments give the same bits on every call.  n_rows == 0 returns
 * before any pointer is looked at.  Labels are not checked here: Y[i] outside [0, m) on a training row gives a row
 * without a one.
 *   residual   P[i, :] = softmax(logits[i, :]) (max-subtracted, e / sum);  E0[i, c] = (c == Y[i] ? 1 : 0) - P[i, c] on the
 *              training rows and +0.0 (written, not skipped) elsewhere;  sums_device[0] = the sum of |E0| (overwritten;
 *              per-workgroup partials in the per-(device, stream) scratch, added in a fixed order).
 *   step       out = min(max(fmaf(alpha, T, beta * R), lo), hi) element by element, beta * R rounded to fp32 once, with
 *              max(v, lo) = v < lo ? lo : v and min(v, hi) = v > hi ? hi : v (so -0.0 stays -0.0 at lo = 0, a NaN stays a
 *              NaN, and lo = -inf, hi = +inf clamp nothing).  With MGGCN_CS_FIX_TRAIN a training row of out is R's,
 *              unchanged and unclamped; without it S may be NULL.  out may be T; it must not be R.  m % 4 == 0 with T, R
 *              and out 16-byte aligned takes a float4 path, anything else an element path; both give the same bits.
 *   correct    out[i, c] = fmaf(s_i, E[i, c], P[i, c]).  With MGGCN_CS_AUTOSCALE s_i = (sums_device[0] * inv_T) / l1_i,
 *              l1_i = sum_c |E[i, c]| in fp32, and 1 where that quotient is not finite or above 1000 (a row of zeros in
 *              E is P's row); sums_device is read on the device.  Without it s_i = scale and sums_device may be NULL.
 *              With MGGCN_CS_SET_LABELS a training row of out is onehot(Y[i]) instead; without it Y and S may be NULL.
 *              out may be P. */
#define MGGCN_CS_FIX_TRAIN 1u
#define MGGCN_CS_AUTOSCALE 2u
#define MGGCN_CS_SET_LABELS 4u
#define MGGCN_CS_MAX_WIDTH 1024u
void mggcn_cs_residual_f32(mggcn_stream_t stream, const float *logits, const int32_t *Y, const int32_t *S, size_t n_rows,
                           size_t m, int32_t train_set, float *P, float *E0, float *sums_device);
void mggcn_cs_step_f32(mggcn_stream_t stream, const float *T, const float *R, const int32_t *S, size_t n_rows, size_t m,
                       float alpha, float beta, float lo, float hi, int32_t train_set, uint32_t flags, float *out);
void mggcn_cs_correct_f32(mggcn_stream_t stream, const float *P, const float *E, const int32_t *Y, const int32_t *S,
                          size_t n_rows, size_t m, int32_t train_set, const float *sums_device, float inv_T, float scale,
                          uint32_t flags, float *out);
/* Graph attention (GAT; opt-in, the reference has no attention layer).  F is a CSR PATTERN of n_rows destinations x n_cols
 * sources (u32 indptr / indices on the device; there is no values array, and a duplicate (i, j) entry counts as two edges),
 * K = heads, dh = width per head, 1 <= K <= MGGCN_GAT_MAX_HEADS and K * dh <= MGGCN_GAT_MAX_WIDTH; head k owns columns
 * [k dh, (k + 1) dh) of every dense operand, att is [2 x K dh] contiguous (row 0: destination vector, row 1: source
 * vector), and s_dst / s_src / lse / D / ds_dst / ds_src are contiguous [rows x K].  With x_ijk = s_dst[i, k] + s_src[j, k],
 * e = x > 0 ? x : slope x and alpha_ijk = exp(e_ijk - lse[i, k]):
 *   scores          s_dst[r, k] = sum_c Z[r, k dh + c] att[0, k dh + c];  s_src likewise with att[1]  (either may be NULL)
 *   forward         lse[i, k] = log sum_j exp(e_ijk) (max-subtracted);  out[i, k dh + c] = sum_j alpha_ijk Z[j, k dh + c];
 *                   a row without entries gets lse = 0 and an out row of +0.0 (written, not skipped)
 *   backward_dst    over the rows of F:  D[i, k] = sum_c G[i, k dh + c] out[i, k dh + c];
 *                   ds_dst[i, k] = sum_j ds_ijk,  ds_ijk = alpha_ijk (sum_c G[i, k dh + c] Z[j, k dh + c] - D[i, k]) (x_ijk > 0 ? 1 : slope)
 *   backward_src    over the rows of F^T (n_rows sources x n_cols destinations; call it after backward_dst):
 *                   ds_src[j, k] = sum_i ds_ijk;
 *                   G_Z[j, k dh + c] = sum_i alpha_ijk G[i, k dh + c] + ds_dst[j, k] att[0, k dh + c] + ds_src[j, k] att[1, k dh + c]
 *                   -- ds_dst here is indexed by SOURCE: the square case, where vertex j is destination j too, passes
 *                   backward_dst's; NULL leaves that term out (a rectangular block whose destinations live elsewhere)
 *   scores_backward G_att[0, c] = sum_i ds_dst[i, k(c)] Z_dst[i, c];  G_att[1, c] = sum_j ds_src[j, k(c)] Z_src[j, c]
 *                   (n_dst / n_src rows; the square case passes the same Z twice).  n_dst == n_src == 0 writes zeros.
 * Nothing of nnz x K is stored or read: alpha is recomputed from s_dst, s_src and lse where it is needed.  No atomics:
 * sums over sources run over F's rows, sums over destinations over F^T's, and the column sums of G_att go through
 * per-workgroup partials in the per-(device, stream) scratch of mggcn_layer_norm_backward_f32, added in a fixed order --
 * two calls on the same input give the same bits in every output.  One wave per row in row order, no plan: correct for
 * any input, slow on rows of many thousand entries.  16-byte loads when dh % 4 == 0 and every dense operand of the call
 * is 16-byte aligned with a leading dimension that is a multiple of 4; single elements otherwise.  out must not alias Z;
 * G_Z must not alias G or Z.  n_rows == 0 returns.  Leading dimensions are checked against K dh. */
#define MGGCN_GAT_MAX_HEADS 16u
#define MGGCN_GAT_MAX_WIDTH 1024u
void mggcn_gat_scores_f32(mggcn_stream_t stream, const float *Z, size_t ldz, const float *att, float *s_dst, float *s_src,
                          size_t n_rows, uint32_t K, uint32_t dh);
void mggcn_gat_forward_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                           const uint32_t *indices, const float *Z, size_t ldz, const float *s_dst, const float *s_src,
                           uint32_t K, uint32_t dh, float slope, float *out, size_t ldo, float *lse);
void mggcn_gat_backward_dst_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                const uint32_t *indices, const float *Z, size_t ldz, const float *s_dst, const float *s_src,
                                const float *lse, const float *G, size_t ldg, const float *out, size_t ldo, uint32_t K,
                                uint32_t dh, float slope, float *D, float *ds_dst);
void mggcn_gat_backward_src_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                                const uint32_t *t_indices, const float *Z, size_t ldz, const float *s_dst, const float *s_src,
                                const float *lse, const float *D, const float *G, size_t ldg, const float *att,
                                const float *ds_dst, uint32_t K, uint32_t dh, float slope, float *ds_src, float *G_Z,
                                size_t ldgz);
void mggcn_gat_scores_backward_f32(mggcn_stream_t stream, const float *ds_dst, const float *Z_dst, size_t ldzd, size_t n_dst,
                                   const float *ds_src, const float *Z_src, size_t ldzs, size_t n_src, uint32_t K, uint32_t dh,
                                   float *G_att);
/* Attention dropout: the three sparse GAT calls with a mask on the normalised coefficients that is never stored (opt-in).
 * Each takes the operands of its plain twin plus (threshold, scale, seed, dropout_stream, dst0, src0), threshold and scale
 * as mggcn_dropout_f32 takes them (threshold = (uint32) floor(p * 2^32), scale = (float)(1 / (1 - p)), from the host).  Entry
 * (global destination i = dst0 + local destination, global source j = src0 + local source, head k):
 *   words = Philox4x32-10(counter = (j, i, 0x80000000 | (k >> 2), dropout_stream), key = (seed & 0xffffffff, seed >> 32))
 *   q_ijk = words[k & 3] >= threshold ? scale : 0
 * The set top bit of the third counter word keeps these words apart from the ones mggcn_dropout_f32 draws with the same
 * (seed, dropout_stream), whose third word is row >> 32.  lse and alpha are the plain call's -- the softmax runs over ALL
 * entries of a row -- and only the gathered weight carries q (one fp32 multiply of the weight by q):
 *   forward         out[i, k dh + c] = sum_j (alpha_ijk q_ijk) Z[j, k dh + c];  a row whose entries are all dropped gets +0.0
 *   backward_dst    D[i, k] = sum_c G out (unchanged: out is the dropped forward's);
 *                   ds_ijk = alpha_ijk (q_ijk sum_c G[i, k dh + c] Z[j, k dh + c] - D[i, k]) (x_ijk > 0 ? 1 : slope)
 *   backward_src    G_Z[j, k dh + c] = sum_i (alpha_ijk q_ijk) G[i, k dh + c] + ds_dst[j, k] att[0, ..] + ds_src[j, k] att[1, ..]
 * For backward_src the rows of F^T are sources (offset src0) and its entries destinations (offset dst0).  The mask is a pure
 * function of (seed, dropout_stream, i, j, k): it does not depend on the grid, on the position of the entry in its row, on
 * the float4 or element path, on which of F or F^T is walked, or on how the rows are split between calls -- rows [a, b) of
 * F with dst0 = a give rows [a, b) of the whole call, bit for bit.  Duplicate entries (i, j) share one bit: both are kept or
 * both dropped.  dst0 + destinations and src0 + sources must not exceed 2^32 (refused otherwise).  threshold == 0 launches
 * the plain kernels: the plain twin's bits in every output (scale is not used then).  No atomics, the same bits on every
 * call, nothing of nnz x K stored. */
void mggcn_gat_forward_drop_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                const uint32_t *indices, const float *Z, size_t ldz, const float *s_dst, const float *s_src,
                                uint32_t K, uint32_t dh, float slope, float *out, size_t ldo, float *lse, uint32_t threshold,
                                float scale, uint64_t seed, uint32_t dropout_stream, uint32_t dst0, uint32_t src0);
void mggcn_gat_backward_dst_drop_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                     const uint32_t *indices, const float *Z, size_t ldz, const float *s_dst,
                                     const float *s_src, const float *lse, const float *G, size_t ldg, const float *out,
                                     size_t ldo, uint32_t K, uint32_t dh, float slope, float *D, float *ds_dst,
                                     uint32_t threshold, float scale, uint64_t seed, uint32_t dropout_stream, uint32_t dst0,
                                     uint32_t src0);
void mggcn_gat_backward_src_drop_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                                     const uint32_t *t_indices, const float *Z, size_t ldz, const float *s_dst,
                                     const float *s_src, const float *lse, const float *D, const float *G, size_t ldg,
                                     const float *att, const float *ds_dst, uint32_t K, uint32_t dh, float slope,
                                     float *ds_src, float *G_Z, size_t ldgz, uint32_t threshold, float scale, uint64_t seed,
                                     uint32_t dropout_stream, uint32_t dst0, uint32_t src0);
/* The packed destination record of backward_src (opt-in).  mggcn_gat_pack_dst_f32 writes, per destination i and head k,
 *   rec[(i K + k) 4 + {0, 1, 2, 3}] = s_dst[i, k], lse[i, k], D[i, k], 0
 * from the three contiguous [n_rows x K] arrays; rec holds n_rows K 4 floats and must be 16-byte aligned.  The _rec twins
 * of backward_src take the operands of mggcn_gat_backward_src_f32 / _drop_f32 with rec in the place of s_dst, lse and D
 * ([n_cols x K] records, 16-byte aligned): the lane that owns an entry issues one 16-byte load where the plain kernel
 * gathers three 4-byte scalars, the fourth float is never read, and the arithmetic is the plain kernel's -- ds_src and G_Z
 * are bit for bit those of the plain call on the arrays the record was packed from.  On a row partition the record is also
 * what a rank needs of every other rank's destinations: one collective of 16 K bytes per vertex. */
void mggcn_gat_pack_dst_f32(mggcn_stream_t stream, const float *s_dst, const float *lse, const float *D, size_t n_rows,
                            uint32_t K, float *rec);
void mggcn_gat_backward_src_rec_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                                    const uint32_t *t_indices, const float *Z, size_t ldz, const float *rec,
                                    const float *s_src, const float *G, size_t ldg, const float *att, const float *ds_dst,
                                    uint32_t K, uint32_t dh, float slope, float *ds_src, float *G_Z, size_t ldgz);
void mggcn_gat_backward_src_rec_drop_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                                         const uint32_t *t_indices, const float *Z, size_t ldz, const float *rec,
                                         const float *s_src, const float *G, size_t ldg, const float *att,
                                         const float *ds_dst, uint32_t K, uint32_t dh, float slope, float *ds_src,
                                         float *G_Z, size_t ldgz, uint32_t threshold, float scale, uint64_t seed,
                                         uint32_t dropout_stream, uint32_t dst0, uint32_t src0);
/* Edge features in the GAT score (opt-in; PyG's GATConv(edge_dim=de) with lin_edge and att_edge folded into one [K x de]
 * matrix).  Each _efeat entry takes the argument list of its twin of the same name without _efeat (plain or _drop),
 * followed by (E, lde, att_edge, de), and backward_dst by (P_e, ldp) after those:
 *   E         [entries x de] fp32, lde >= de counted in elements: row p belongs to indices[p] of the CSR the call walks,
 *             with the same base as indices -- a call on a block of rows (indptr + r0, the row operands moved by r0 rows)
 *             passes the SAME E pointer as the call on all rows.  backward_src walks F^T and takes E in F^T's entry order.
 *   att_edge  [K x de] contiguous;  1 <= de <= MGGCN_GAT_MAX_EDGE_DIM
 * The score is defined to the bit: with p the entry (i, j),
 *   t_pk = fmaf(E[p, de - 1], att_edge[k, de - 1], ... fmaf(E[p, 0], att_edge[k, 0], 0.f))      (c ascending)
 *   x_ijk = (s_dst[i, k] + s_src[j, k]) + t_pk
 * and everything after x is the twin's: e = x > 0 ? x : slope x, the one-pass softmax, lse, alpha, D, ds, the gather, and
 * the q of the _drop forms (the same Philox words).  The three calls therefore recompute the same x and the same alpha for
 * an edge whichever copy of E they read, provided both copies hold the same row for it.  With att_edge = 0 (and a finite
 * E) every output shared with the twin has the twin's bits.  The edge term enters the score only; the message stays
 * alpha Z[j].  backward_dst additionally writes row i's share of the gradient of att_edge,
 *   P_e[i ldp + k de + c] = sum_j ds_ijk E[p, c]   over the entries of row i (+0.0 for a row without entries), ldp >= K de,
 * from the ds it already forms (under _drop the sum carries q), on the lane that owns the entry: a lane's entries in row
 * order, then the 64 lanes folded in a fixed order; mggcn_gatv2_att_grad_f32 on P_e (width = K de) gives G_att_edge [K x de].  Nothing of
 * nnz x K is stored.  No atomics; every output has the same bits on every call, and every row-local output (out, lse, D,
 * ds_dst, ds_src, G_Z, P_e) the same bits for every split of the rows between calls.  A row of E is read with 16-byte loads
 * when de % 4 == 0, E is 16-byte aligned and lde % 4 == 0, and element by element otherwise; the (VEC, NT, U) variant is
 * chosen as the twin chooses it.  P_e must not alias an input.  There is no record (_rec_) and no bf16 form.  The _drop
 * forms with threshold == 0 launch the plain efeat kernels. */
#define MGGCN_GAT_MAX_EDGE_DIM 16u
void mggcn_gat_forward_efeat_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                 const uint32_t *indices, const float *Z, size_t ldz, const float *s_dst, const float *s_src,
                                 uint32_t K, uint32_t dh, float slope, float *out, size_t ldo, float *lse, const float *E,
                                 size_t lde, const float *att_edge, uint32_t de);
void mggcn_gat_backward_dst_efeat_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                      const uint32_t *indices, const float *Z, size_t ldz, const float *s_dst,
                                      const float *s_src, const float *lse, const float *G, size_t ldg, const float *out,
                                      size_t ldo, uint32_t K, uint32_t dh, float slope, float *D, float *ds_dst,
                                      const float *E, size_t lde, const float *att_edge, uint32_t de, float *P_e, size_t ldp);
void mggcn_gat_backward_src_efeat_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                                      const uint32_t *t_indices, const float *Z, size_t ldz, const float *s_dst,
                                      const float *s_src, const float *lse, const float *D, const float *G, size_t ldg,
                                      const float *att, const float *ds_dst, uint32_t K, uint32_t dh, float slope,
                                      float *ds_src, float *G_Z, size_t ldgz, const float *E, size_t lde,
                                      const float *att_edge, uint32_t de);
void mggcn_gat_forward_efeat_drop_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                      const uint32_t *indices, const float *Z, size_t ldz, const float *s_dst,
                                      const float *s_src, uint32_t K, uint32_t dh, float slope, float *out, size_t ldo,
                                      float *lse, uint32_t threshold, float scale, uint64_t seed, uint32_t dropout_stream,
                                      uint32_t dst0, uint32_t src0, const float *E, size_t lde, const float *att_edge,
                                      uint32_t de);
void mggcn_gat_backward_dst_efeat_drop_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                           const uint32_t *indices, const float *Z, size_t ldz, const float *s_dst,
                                           const float *s_src, const float *lse, const float *G, size_t ldg, const float *out,
                                           size_t ldo, uint32_t K, uint32_t dh, float slope, float *D, float *ds_dst,
                                           uint32_t threshold, float scale, uint64_t seed, uint32_t dropout_stream,
                                           uint32_t dst0, uint32_t src0, const float *E, size_t lde, const float *att_edge,
                                           uint32_t de, float *P_e, size_t ldp);
void mggcn_gat_backward_src_efeat_drop_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                                           const uint32_t *t_indices, const float *Z, size_t ldz, const float *s_dst,
                                           const float *s_src, const float *lse, const float *D, const float *G, size_t ldg,
                                           const float *att, const float *ds_dst, uint32_t K, uint32_t dh, float slope,
                                           float *ds_src, float *G_Z, size_t ldgz, uint32_t threshold, float scale,
                                           uint64_t seed, uint32_t dropout_stream, uint32_t dst0, uint32_t src0,
                                           const float *E, size_t lde, const float *att_edge, uint32_t de);
/* Dynamic graph attention (GATv2; opt-in).  F, K, dh, the limits and the column layout of a head are those of the GAT block
 * above; Zs is the source transform (one row per source: the row that gets aggregated), Zd the destination transform (one
 * row per destination), att is [1 x K dh] contiguous, and lse / D are contiguous [destinations x K].  With
 * t_ijk[c] = Zd[i, k dh + c] + Zs[j, k dh + c], u = t > 0 ? t : slope t, lrelu' = t > 0 ? 1 : slope,
 * e_ijk = sum_c att[k dh + c] u_ijk[c] and alpha_ijk = exp(e_ijk - lse[i, k]):
 *   forward       lse[i, k] = log sum_j exp(e_ijk) (max-subtracted);  out[i, k dh + c] = sum_j alpha_ijk Zs[j, k dh + c];
 *                 a row without entries gets lse = 0 and an out row of +0.0 (written, not skipped); a row of one entry
 *                 copies its source's row bit for bit
 *   backward_dst  over the rows of F:  D[i, k] = sum_c G[i, k dh + c] out[i, k dh + c];
 *                 ds_ijk = alpha_ijk (sum_c G[i, k dh + c] Zs[j, k dh + c] - D[i, k]);
 *                 G_Zd[i, k dh + c] = att[k dh + c] sum_j ds_ijk lrelu'(t_ijk[c]);  P[i, k dh + c] = sum_j ds_ijk u_ijk[c]
 *                 (row i's share of G_att; a row without entries gets +0.0 in both, whatever the sign of att)
 *   att_grad      G_att[c] = sum_i P[i, c] over n_rows rows of `width` columns (1 <= width <= MGGCN_GAT_MAX_WIDTH);
 *                 n_rows == 0 writes zeros
 *   backward_src  over the rows of F^T (n_rows sources x n_cols destinations; call it after backward_dst, whose D it reads):
 *                 G_Zs[j, k dh + c] = sum_i (alpha_ijk G[i, k dh + c] + ds_ijk att[k dh + c] lrelu'(t_ijk[c]))
 * The score of an entry exists only once the source's head-row has been gathered, so each sparse call computes e on the
 * rows it gathers; nothing of nnz x K is stored or read.  No atomics: sums over sources run over F's rows, sums over
 * destinations over F^T's, the softmax folds its lane groups in a fixed order, and att_grad goes through per-workgroup
 * partials in the per-(device, stream) scratch of mggcn_gat_scores_backward_f32, added in a fixed order -- two calls on the
 * same input give the same bits in every output, and rows [r0, r1) of a sparse call passed as a call of their own (indptr +
 * r0, the row operands moved by r0 rows) give the whole call's rows bit for bit.  One wave per row, no plan: correct for any
 * input, slow on rows of many thousand entries.  16-byte loads when dh % 4 == 0 and every dense operand of the call,
 * att included, is 16-byte aligned with a leading dimension that is a multiple of 4; single elements otherwise.  Zs and Zd
 * may be the two halves of one [rows x 2 K dh] buffer (ld = 2 K dh), and so may G_Zs and G_Zd.  out must not alias Zs or Zd;
 * G_Zd, P and G_Zs must not alias an input.  n_rows == 0 returns.  Leading dimensions are checked against K dh. */
void mggcn_gatv2_forward_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                             const uint32_t *indices, const float *Zs, size_t ldzs, const float *Zd, size_t ldzd,
                             const float *att, uint32_t K, uint32_t dh, float slope, float *out, size_t ldo, float *lse);
void mggcn_gatv2_backward_dst_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                  const uint32_t *indices, const float *Zs, size_t ldzs, const float *Zd, size_t ldzd,
                                  const float *att, const float *lse, const float *G, size_t ldg, const float *out,
                                  size_t ldo, uint32_t K, uint32_t dh, float slope, float *D, float *G_Zd, size_t ldgzd,
                                  float *P, size_t ldp);
void mggcn_gatv2_att_grad_f32(mggcn_stream_t stream, const float *P, size_t ldp, size_t n_rows, uint32_t width,
                              float *G_att);
void mggcn_gatv2_backward_src_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                                  const uint32_t *t_indices, const float *Zs, size_t ldzs, const float *Zd, size_t ldzd,
                                  const float *att, const float *lse, const float *D, const float *G, size_t ldg,
                                  uint32_t K, uint32_t dh, float slope, float *G_Zs, size_t ldgzs);
/* The packed destination record of the GATv2 backward_src (opt-in).  mggcn_gatv2_pack_dst_f32 writes, per destination i and
 * head k,
 *   rec[(i K + k) 2 + {0, 1}] = lse[i, k], D[i, k]
 * from the two contiguous [n_rows x K] arrays (bit patterns are copied as they are); rec holds n_rows K 2 floats and must be
 * 8-byte aligned; n_rows == 0 returns.  mggcn_gatv2_backward_src_rec_f32 takes the operands of mggcn_gatv2_backward_src_f32
 * with rec in the place of lse and D ([n_cols x K] records, 8-byte aligned): the lane that owns an entry issues one 8-byte
 * load where the plain kernel gathers two 4-byte scalars, one chunk ahead as there, and the arithmetic and the choice of the
 * variant are the plain kernel's -- G_Zs is bit for bit that of the plain call on the arrays the record was packed from, and
 * a row range passed as a call of its own gives the whole call's rows.  On a row partition the record is what a rank needs
 * of every other rank's destinations: one collective of 8 K bytes per vertex. */
void mggcn_gatv2_pack_dst_f32(mggcn_stream_t stream, const float *lse, const float *D, size_t n_rows, uint32_t K, float *rec);
void mggcn_gatv2_backward_src_rec_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                                      const uint32_t *t_indices, const float *Zs, size_t ldzs, const float *Zd, size_t ldzd,
                                      const float *att, const float *rec, const float *G, size_t ldg, uint32_t K,
                                      uint32_t dh, float slope, float *G_Zs, size_t ldgzs);
/* The export of the attention coefficients (opt-in: the one place where something of nnz x K is written, and no training
 * call reads it).  Both take F as the calls above and the state a forward left behind -- s_dst, s_src, lse of
 * mggcn_gat_scores_f32 / mggcn_gat_forward_f32, or Zs, Zd, att, lse of mggcn_gatv2_forward_f32 -- and write, for entry p of
 * the indices array (row i, source j = indices[p]) and head k,
 *   alpha[p lda + k] = exp(e_ijk - lse[i, k]),   lda >= K, offsets in size_t,
 * which is the float expression the backward kernels of the same file evaluate: the exported value is the coefficient the
 * model trains with (after a forward with attention dropout: the coefficient BEFORE the factor q, the softmax over all
 * entries).  indptr values are used as they are: a call over rows [r0, r1) (indptr + r0, the row operands moved by r0 rows,
 * alpha unmoved) writes exactly the positions the whole call writes for those rows.  Columns [K, lda) are never written and
 * rows without entries write nothing.  No atomics, no reduction between entries: a value depends on its own entry and its
 * row's lse alone, so it has the same bits on every call and for every split of the rows between calls.  v1 stores 16 bytes
 * per (entry, four heads) when K % 4 == 0 and alpha is 16-byte aligned with lda % 4 == 0, single elements otherwise; v2
 * picks its variant as mggcn_gatv2_forward_f32 does (from dh, Zs, Zd and att) and stores single elements.  alpha must not
 * alias an input.  n_rows == 0 returns. */
void mggcn_gat_alpha_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                         const uint32_t *indices, const float *s_dst, const float *s_src, const float *lse, uint32_t K,
                         float slope, float *alpha, size_t lda);
void mggcn_gatv2_alpha_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                           const uint32_t *indices, const float *Zs, size_t ldzs, const float *Zd, size_t ldzd,
                           const float *att, const float *lse, uint32_t K, uint32_t dh, float slope, float *alpha,
                           size_t lda);
/* Dot-product (transformer) graph attention (opt-in; PyG's TransformerConv without root weight, gate and edge features).  F,
 * K, dh, the limits and the column layout of a head are those of the GAT block above; Zq is the query transform (one row per
 * destination), Zk the key and Zv the value transform (one row per source each), lse / D are contiguous [destinations x K],
 * and the attention has no parameter of its own.  With `scale` = c (the model passes fp32(1 / sqrt(dh))),
 * e_ijk = c sum_c Zq[i, k dh + c] Zk[j, k dh + c] and alpha_ijk = exp(e_ijk - lse[i, k]):
 *   forward       lse[i, k] = log sum_j exp(e_ijk) (max-subtracted);  out[i, k dh + c] = sum_j alpha_ijk Zv[j, k dh + c];
 *                 a row without entries gets lse = 0 and an out row of +0.0 (written, not skipped); a row of one entry
 *                 copies its source's Zv row bit for bit
 *   backward_dst  over the rows of F:  D[i, k] = sum_c G[i, k dh + c] out[i, k dh + c];
 *                 dalpha_ijk = sum_c G[i, k dh + c] Zv[j, k dh + c];  ds_ijk = alpha_ijk (dalpha_ijk - D[i, k]);
 *                 G_Zq[i, k dh + c] = c sum_j ds_ijk Zk[j, k dh + c]  (a row without entries gets +0.0)
 *   backward_src  over the rows of F^T (n_rows sources x n_cols destinations; call it after backward_dst, whose D it reads):
 *                 G_Zk[j, k dh + c] = c sum_i ds_ijk Zq[i, k dh + c];  G_Zv[j, k dh + c] = sum_i alpha_ijk G[i, k dh + c]
 *                 (a source nobody gathers gets +0.0 in both)
 * Each sparse call gathers two dense head-rows per entry and computes e on the rows it gathers; nothing of nnz x K is stored
 * or read.  No atomics: sums over sources run over F's rows, sums over destinations over F^T's, and the softmax folds its
 * lane groups in a fixed order -- two calls on the same input give the same bits in every output, and rows [r0, r1) of a call
 * passed as a call of their own (indptr + r0, the row operands moved by r0 rows) give the whole call's rows bit for bit.  One
 * wave per row, no plan.  Every dense operand has a leading dimension of its own: Zq, Zk and Zv may be the thirds of one
 * [rows x 3 K dh] buffer (ld = 3 K dh), and so may G_Zq, G_Zk and G_Zv.  16-byte loads when dh % 4 == 0 and every dense
 * operand of the call is 16-byte aligned with a leading dimension that is a multiple of 4; single elements otherwise.  out
 * must not alias Zq, Zk or Zv; G_Zq, G_Zk and G_Zv must not alias an input or each other.  n_rows == 0 returns.  Leading
 * dimensions are checked against K dh. */
void mggcn_gatdot_forward_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                              const uint32_t *indices, const float *Zq, size_t ldq, const float *Zk, size_t ldk,
                              const float *Zv, size_t ldv, uint32_t K, uint32_t dh, float scale, float *out, size_t ldo,
                              float *lse);
void mggcn_gatdot_backward_dst_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                   const uint32_t *indices, const float *Zq, size_t ldq, const float *Zk, size_t ldk,
                                   const float *Zv, size_t ldv, const float *lse, const float *G, size_t ldg, const float *out,
                                   size_t ldo, uint32_t K, uint32_t dh, float scale, float *D, float *G_Zq, size_t ldgzq);
void mggcn_gatdot_backward_src_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                                   const uint32_t *t_indices, const float *Zq, size_t ldq, const float *Zk, size_t ldk,
                                   const float *Zv, size_t ldv, const float *lse, const float *D, const float *G, size_t ldg,
                                   uint32_t K, uint32_t dh, float scale, float *G_Zk, size_t ldgzk, float *G_Zv,
                                   size_t ldgzv);
/* bf16 gathers of the attention kernels (opt-in; gat(agg_dtype="bf16")).  Every dense [rows x width] operand that a sparse
 * attention kernel indexes by an entry's COLUMN -- the gathered role -- is read from a bf16 image of the fp32 tensor
 * (uint16_t bit patterns, as mggcn_convert_f32_bf16 writes them: round to nearest even), half the bytes per gathered row.
 * Everything else stays fp32 and is read from the fp32 tensor: every operand indexed by the kernel's own row, the [n x K]
 * scalars (s_dst, s_src, lse, D, ds_*), all arithmetic and sums, every output.  The gathered roles:
 *              forward / backward_dst (rows of F)     backward_src (rows of F^T)
 *   gat        Z                                      G
 *   gatv2      Zs                                     Zd, G
 *   gatdot     Zk, Zv                                 Zq, G
 * so a self-loop entry meets the rounded row in the gathered role and the fp32 row in the own role.
 * Each entry below is the twin of the entry of the same name ending in _f32 (mggcn_gat_forward_bf16 of
 * mggcn_gat_forward_f32, mggcn_gat_forward_drop_bf16 of mggcn_gat_forward_drop_f32, ...): the same argument list with the
 * gathered operands as const uint16_t * and their leading dimensions counted in ELEMENTS, the same null-operand rules,
 * n_rows == 0 returns, the same aliasing rules, the same limits (MGGCN_GAT_MAX_HEADS, MGGCN_GAT_MAX_WIDTH).  The kernel is
 * the fp32 kernel with the gathered loads on the image -- one 8-byte load for a lane's four columns, one 2-byte load for a
 * single column -- and each value widened exactly (bits << 16: -0.0 and the denormals survive); the lane -> column map, the
 * summation order and the five (VEC, NT, U) variants are the fp32 entry's.  The variant follows the fp32 rule with the
 * alignment counted in elements: a bf16 operand qualifies for the four-column path when its base is 8-byte aligned and
 * its leading dimension is a multiple of 4 elements; the fp32 operands of the call keep the 16-byte rule.
 * CONTRACT: the result equals that of the _f32 entry called on the exactly widened images (equally aligned in elements),
 * bit for bit -- every output, for every variant, for a row range passed as a call of its own, and for the _drop forms with
 * any (threshold, seed, stream, dst0, src0).  There is no bf16 form of the record entries (_rec_), the pack, scores and
 * export entries. */
void mggcn_gat_forward_bf16(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                            const uint32_t *indices, const uint16_t *Z, size_t ldz, const float *s_dst, const float *s_src,
                            uint32_t K, uint32_t dh, float slope, float *out, size_t ldo, float *lse);
void mggcn_gat_backward_dst_bf16(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                 const uint32_t *indices, const uint16_t *Z, size_t ldz, const float *s_dst, const float *s_src,
                                 const float *lse, const float *G, size_t ldg, const float *out, size_t ldo, uint32_t K,
                                 uint32_t dh, float slope, float *D, float *ds_dst);
void mggcn_gat_backward_src_bf16(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                                 const uint32_t *t_indices, const float *Z, size_t ldz, const float *s_dst, const float *s_src,
                                 const float *lse, const float *D, const uint16_t *G, size_t ldg, const float *att,
                                 const float *ds_dst, uint32_t K, uint32_t dh, float slope, float *ds_src, float *G_Z,
                                 size_t ldgz);
void mggcn_gat_forward_drop_bf16(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                 const uint32_t *indices, const uint16_t *Z, size_t ldz, const float *s_dst, const float *s_src,
                                 uint32_t K, uint32_t dh, float slope, float *out, size_t ldo, float *lse, uint32_t threshold,
                                 float scale, uint64_t seed, uint32_t dropout_stream, uint32_t dst0, uint32_t src0);
void mggcn_gat_backward_dst_drop_bf16(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                      const uint32_t *indices, const uint16_t *Z, size_t ldz, const float *s_dst,
                                      const float *s_src, const float *lse, const float *G, size_t ldg, const float *out,
                                      size_t ldo, uint32_t K, uint32_t dh, float slope, float *D, float *ds_dst,
                                      uint32_t threshold, float scale, uint64_t seed, uint32_t dropout_stream, uint32_t dst0,
                                      uint32_t src0);
void mggcn_gat_backward_src_drop_bf16(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                                      const uint32_t *t_indices, const float *Z, size_t ldz, const float *s_dst,
                                      const float *s_src, const float *lse, const float *D, const uint16_t *G, size_t ldg,
                                      const float *att, const float *ds_dst, uint32_t K, uint32_t dh, float slope,
                                      float *ds_src, float *G_Z, size_t ldgz, uint32_t threshold, float scale, uint64_t seed,
                                      uint32_t dropout_stream, uint32_t dst0, uint32_t src0);
void mggcn_gatv2_forward_bf16(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                              const uint32_t *indices, const uint16_t *Zs, size_t ldzs, const float *Zd, size_t ldzd,
                              const float *att, uint32_t K, uint32_t dh, float slope, float *out, size_t ldo, float *lse);
void mggcn_gatv2_backward_dst_bf16(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                   const uint32_t *indices, const uint16_t *Zs, size_t ldzs, const float *Zd, size_t ldzd,
                                   const float *att, const float *lse, const float *G, size_t ldg, const float *out, size_t ldo,
                                   uint32_t K, uint32_t dh, float slope, float *D, float *G_Zd, size_t ldgzd, float *P,
                                   size_t ldp);
void mggcn_gatv2_backward_src_bf16(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                                   const uint32_t *t_indices, const float *Zs, size_t ldzs, const uint16_t *Zd, size_t ldzd,
                                   const float *att, const float *lse, const float *D, const uint16_t *G, size_t ldg, uint32_t K,
                                   uint32_t dh, float slope, float *G_Zs, size_t ldgzs);
void mggcn_gatdot_forward_bf16(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                               const uint32_t *indices, const float *Zq, size_t ldq, const uint16_t *Zk, size_t ldk,
                               const uint16_t *Zv, size_t ldv, uint32_t K, uint32_t dh, float scale, float *out, size_t ldo,
                               float *lse);
void mggcn_gatdot_backward_dst_bf16(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                    const uint32_t *indices, const float *Zq, size_t ldq, const uint16_t *Zk, size_t ldk,
                                    const uint16_t *Zv, size_t ldv, const float *lse, const float *G, size_t ldg,
                                    const float *out, size_t ldo, uint32_t K, uint32_t dh, float scale, float *D, float *G_Zq,
                                    size_t ldgzq);
void mggcn_gatdot_backward_src_bf16(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                                    const uint32_t *t_indices, const uint16_t *Zq, size_t ldq, const float *Zk, size_t ldk,
                                    const float *Zv, size_t ldv, const float *lse, const float *D, const uint16_t *G,
                                    size_t ldg, uint32_t K, uint32_t dh, float scale, float *G_Zk, size_t ldgzk, float *G_Zv,
                                    size_t ldgzv);

/* The max aggregator of GraphSAGE (no reference counterpart): the element-wise maximum over a vertex's neighbours and its
 * backward pass.  F is a CSR pattern as the attention entries take it (u32 indptr / indices on the device, no values), the
 * width is 1 <= d <= MGGCN_GAT_MAX_WIDTH, every dense operand has its own leading dimension >= d, and the kernels are the
 * one-wave-per-row layout of the attention kernels with their five (VEC, NT, U) variants: the four-column path when
 * d % 4 == 0 and every dense operand -- arg counts as one, of 4-byte elements -- has a 16-byte aligned base and a leading
 * dimension that is a multiple of 4, the element path otherwise.  n_rows == 0 returns.  No atomics.
 *   forward    out[i, c] = max over the entries j of row i of B[j, c], arg[i, c] = src0 + j of the winner (src0: the global
 *              index of column 0).  The order is total: the larger value wins, equal values (==, so -0.0 ties with +0.0) go
 *              to the smaller j; a NaN is never selected.  out carries the winner's bits exactly.  A row in which nothing is
 *              selected (no entry, or NaNs only) gives out = +0.0 and arg = MGGCN_AGG_NONE; a row of -inf entries selects its
 *              smallest j.  arg may be NULL (the value only).  The result does not depend on the lane geometry, the
 *              path, the order of a row's entries or duplicate entries.  out must not alias B; src0 + n_cols < 2^32 - 1.
 *   backward   over the rows j of F^T (n_rows sources, n_cols destinations; an entry is a destination i):
 *              G_B[j, c] = (flags & MGGCN_AGG_ACCUMULATE ? G_B[j, c] : 0) + sum_i [arg[i, c] == src0 + j] G[i, c].  An entry
 *              whose index equals its predecessor's in the same row is skipped, so a pair (i, j) that occurs more than once
 *              delivers its gradient once: equal indices of a row of F^T MUST be adjacent (rows in ascending order are, and
 *              mggcn_csr_transpose_host emits those).  The terms are added in a fixed order (a group's entries in row order,
 *              then the groups): every output has the same bits on every call and for every split of the rows between
 *              calls.  G_B must not alias G; an unknown flag fails the precondition check.
 *   pack       rec[i, 2c] = arg[i, c] and rec[i, 2c + 1] = the bits of G[i, c] for i < n_rows, c < d, both unchanged (a NaN
 *              keeps its payload): rows of 8-byte records, ldr >= 2 d in 32-bit words.  rec must be 8-byte aligned and ldr
 *              even (precondition check); the four-column path -- two 16-byte loads and two 16-byte stores per lane -- when
 *              d % 4 == 0 and arg, G and rec all have 16-byte rows, the element path (one 8-byte store per column) otherwise.
 *              Words of a row beyond 2 d are not written.  rec must not alias an input.
 *   backward_rec   the backward with arg and G of a destination read from its row of `rec` (as pack writes it: the one
 *              matrix a row-partitioned model exchanges).  The row walk, the skip rule, the select, the order of the sums
 *              and the flags are the backward's; a lane's four columns are 32 contiguous bytes (two adjacent 16-byte
 *              loads), the element path reads one 8-byte record per column.  The four-column path when d % 4 == 0 and rec
 *              and G_B have 16-byte rows: for operands aligned as the plain call's the same (VEC, NT, U) runs and G_B has
 *              the plain call's bits, on every call and for every split of the rows between calls.  rec 8-byte aligned,
 *              ldr even and >= 2 d, src0 + n_rows < 2^32 - 1, G_B must not alias rec. */
#define MGGCN_AGG_ACCUMULATE 1u
#define MGGCN_AGG_NONE 0xFFFFFFFFu
void mggcn_agg_max_forward_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                               const uint32_t *indices, const float *B, size_t ldb, uint32_t d, uint32_t src0, float *out,
                               size_t ldo, uint32_t *arg, size_t lda);
void mggcn_agg_max_backward_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                                const uint32_t *t_indices, const uint32_t *arg, size_t lda, const float *G, size_t ldg,
                                uint32_t d, uint32_t src0, uint32_t flags, float *G_B, size_t ldgb);
void mggcn_agg_max_pack_f32(mggcn_stream_t stream, const uint32_t *arg, size_t lda, const float *G, size_t ldg, size_t n_rows,
                            uint32_t d, uint32_t *rec, size_t ldr);
void mggcn_agg_max_backward_rec_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                                    const uint32_t *t_indices, const uint32_t *rec, size_t ldr, uint32_t d, uint32_t src0,
                                    uint32_t flags, float *G_B, size_t ldgb);

/* The per-epoch edge sample of gat / sage(aggr="max") (no reference counterpart), drawn on the device: count, scan, compact.
 * A CSR pattern (u32 indptr / indices on the device, no values) keeps entry (destination i, source j), both global vertex
 * numbers, iff
 *     i == j   or   thr_i == 0xFFFFFFFF   or   word 0 of Philox4x32-10(counter = (j, i, 0xC0000000, epoch),
 *                                                   key = (seed & 0xFFFFFFFF, seed >> 32)) < thr_i,
 * thr the destinations' thresholds (the host's floor(q_i 2^32), capped at 2^32 - 1).  The third counter word keeps the draw
 * apart from mggcn_dropout_f32 (row >> 32), attention dropout (0x80000000 | k >> 2) and the label mask (first word
 * 0xFFFFFFFF) under one seed.  The bit is a function of (seed, epoch, i, j) alone: duplicate entries share it, nothing of
 * size nnz is stored between count and compact, and a matrix and its transpose keep the same pairs, each in its own entry
 * order -- the two results are transposes of each other entry for entry.
 *   transposed = 0: row r is destination row0 + r with threshold thr[r], column c is source col0 + c.
 *   transposed = 1: row r is source row0 + r, column c is destination col0 + c with threshold thr[c] (gathered).
 * row0 / col0 enter the counter and the self-loop test only: a call over a row range (indptr + r0, thr + r0 when not
 * transposed, row0 = r0) gives the whole call's rows.
 *   count     counts[r] = the kept entries of row r.  One wave per row.
 *   scan      out_indptr[0] = 0, out_indptr[r + 1] = counts[0] + ... + counts[r] (mod 2^32), n_rows + 1 words, in three
 *             launches (sums per 256-block, one workgroup over the block sums, add): no workgroup waits on another.
 *             n_rows == 0 writes out_indptr[0].  out_indptr must not alias counts.
 *   compact   draws the same bits again and writes the kept columns of row r, in their original order, at
 *             out_indices + out_indptr[r]: one wave per row over 64-entry chunks, a ballot of the keep bits, a lane's rank
 *             the population count of the lanes below it.  No atomics, no scratch, the same bits on every call and for
 *             every split of the rows between calls; nothing is written at or beyond out_indptr[r + 1] for any row, so
 *             nothing beyond out_indptr[n_rows] entries.  out_indices must not alias indices.
 * n_rows == 0 returns (count, compact).  Values are not carried. */
void mggcn_edge_sample_count_u32(mggcn_stream_t stream, uint32_t n_rows, const uint32_t *indptr, const uint32_t *indices,
                                 const uint32_t *thr, int transposed, uint32_t row0, uint32_t col0, uint64_t seed,
                                 uint32_t epoch, uint32_t *counts);
void mggcn_edge_sample_scan_u32(mggcn_stream_t stream, const uint32_t *counts, size_t n_rows, uint32_t *out_indptr);
void mggcn_edge_sample_compact_u32(mggcn_stream_t stream, uint32_t n_rows, const uint32_t *indptr, const uint32_t *indices,
                                   const uint32_t *thr, int transposed, uint32_t row0, uint32_t col0, uint64_t seed,
                                   uint32_t epoch, const uint32_t *out_indptr, uint32_t *out_indices);
/* The sample WITH VALUES, for the weighted sums of gcn / sage(aggr="mean") (edge_rescale=).  The keep bit is the one above
 * (same counter, same domain word, same self-loop rule); a kept entry's value is multiplied by a factor of its DESTINATION,
 * read from one array by both sides, so the samples of F and of F^T hold the same pairs with the same value bits.
 *   rowscale     over F only (rows are destinations; row0 / col0 as in count): counts[r] with count's bits and
 *                scale[r] = S_r / S'_r, S_r the sum of the row's values and S'_r the sum over its kept entries, both summed in
 *                one walk and one fixed order (lane l adds entries l, l + 64, ...; one butterfly folds the lanes).  S'_r == 0
 *                gives 0 (never a NaN), a row kept whole exactly 1.  One wave per row; no atomics, no scratch; the result
 *                does not depend on the grid or on a split of the rows between calls.
 *   compact_val  compact, and beside the kept columns out_values = value * scale[destination]: scale[r] when transposed = 0,
 *                scale[c] (gathered) when transposed = 1, NULL = no factor; one fp32 multiply, skipped for i == j when
 *                scale_self == 0.  Nothing is written at or beyond out_indptr[r + 1] in either output.  out_values must not
 *                alias values. */
void mggcn_edge_sample_rowscale_f32(mggcn_stream_t stream, uint32_t n_rows, const uint32_t *indptr, const uint32_t *indices,
                                    const float *values, const uint32_t *thr, uint32_t row0, uint32_t col0, uint64_t seed,
                                    uint32_t epoch, uint32_t *counts, float *scale);
void mggcn_edge_sample_compact_val_f32(mggcn_stream_t stream, uint32_t n_rows, const uint32_t *indptr, const uint32_t *indices,
                                       const float *values, const uint32_t *thr, int transposed, uint32_t row0, uint32_t col0,
                                       uint64_t seed, uint32_t epoch, const float *scale, int scale_self,
                                       const uint32_t *out_indptr, uint32_t *out_indices, float *out_values);

/* The row-split SpMM over a device-resident CSR with a plan built ON THE DEVICE (csrc/spmm_dev.hip): what multiplies by the
 * edge sample above, a matrix the host never sees.
 *   capacity   out3 = (work items, partial-sum slots, split rows) of the row-split rule on a HOST indptr: a row of
 *              len <= split + split / 2 entries is one item, a longer one ceil(len / split) slices.  The rule is monotone in the
 *              row length, so the PARENT's three counts bound those of every sample of it.  split == 0: MGGCN_SPMM_SPLIT
 *              (default 512); the floor is 64.  Host only.
 *   create     allocates the tables, the partial sums (slots x max_d floats) and the builder's work space at the parent's
 *              capacity; nothing is built.  destroy / bytes; describe: out5 = (the three capacities, split, max_d).
 *   build      enqueue-only, no host read: per row the split flag and slice count, two exclusive scans
 *              (mggcn_edge_sample_scan_u32), then the item and split-row tables in ROW order with the host builder's slice
 *              boundaries (beg + len k / parts in 64-bit) and the three totals in device memory.  The host builder's
 *              longest-first order is not reproduced.  Nothing at or beyond a table's capacity is written.  The plan holds
 *              the row bounds of `indptr_dev` as they are at the build: build again after the matrix changes.
 *   read       tests and reports: synchronises and copies out the whole tables (capacity x 4 words each; NULL skips one) and
 *              the three totals (items, slots, split rows).
 *   csr_dev    C = alpha A B + beta C with the contract of mggcn_spmm_csr_f32 / _bf16 (flags, leading dimensions, the vector
 *              and the scalar path) over the built plan: launch geometry from the capacities, true counts from device memory.
 *              A row is cut and summed exactly as a host row-split plan of the same split cuts and sums it: the same bits.
 *              No atomics; the same bits on every call. */
typedef struct mggcn_spmm_dev_plan mggcn_spmm_dev_plan;
void mggcn_spmm_dev_plan_capacity(uint32_t n_rows, const uint32_t *host_parent_indptr, uint32_t split, uint32_t *out3);
mggcn_spmm_dev_plan *mggcn_spmm_dev_plan_create(uint32_t n_rows, const uint32_t *host_parent_indptr, uint32_t max_d,
                                                uint32_t split);
void mggcn_spmm_dev_plan_destroy(mggcn_spmm_dev_plan *plan);
size_t mggcn_spmm_dev_plan_bytes(const mggcn_spmm_dev_plan *plan);
void mggcn_spmm_dev_plan_describe(const mggcn_spmm_dev_plan *plan, uint32_t *out5);
void mggcn_spmm_dev_plan_build(mggcn_stream_t stream, mggcn_spmm_dev_plan *plan, const uint32_t *indptr_dev);
void mggcn_spmm_dev_plan_read(const mggcn_spmm_dev_plan *plan, uint32_t *host_items, uint32_t *host_split_rows,
                              uint32_t *host_totals);
void mggcn_spmm_csr_dev_f32(mggcn_stream_t stream, const mggcn_spmm_dev_plan *plan, uint32_t n_rows, uint32_t n_cols,
                            const uint32_t *indptr, const uint32_t *indices, const float *values, const float *B, size_t ldb,
                            float *C, size_t ldc, uint32_t d, float alpha, float beta, uint32_t flags, float slope);
void mggcn_spmm_csr_dev_bf16(mggcn_stream_t stream, const mggcn_spmm_dev_plan *plan, uint32_t n_rows, uint32_t n_cols,
                             const uint32_t *indptr, const uint32_t *indices, const float *values, const uint16_t *B, size_t ldb,
                             float *C, size_t ldc, uint32_t d, float alpha, float beta, uint32_t flags, float slope);

/* A stable segmented LSD radix sort of (u32 key, u32 value) pairs (csrc/radix_sort.hip; no reference counterpart): the one
 * way to put anything in order on the device.  Segment s is [s seg_len, (s + 1) seg_len) of each array; every segment is
 * sorted on its own, ascending on the key bits [begin_bit, end_bit) -- bits outside the range never influence the order --,
 * and equal keys keep their input order.  The result always ends in keys / vals (an odd number of passes ends with a
 * device-to-device copy); keys_alt / vals_alt are scratch of the same sizes.
 *   One pass per 8-bit digit: per-tile digit histograms (MGGCN_RADIX_SORT_TILE pairs per workgroup, integer LDS counters),
 *   ONE exclusive scan of the (segment, digit, tile) table with mggcn_edge_sample_scan_u32 -- every segment holds seg_len
 *   pairs, so the scanned word is the absolute position --, and a scatter in which a pair's place is the scanned word of its
 *   digit and tile plus its rank among the tile's equal digits, a rank made of ballots, population counts and prefix counts
 *   and never of an atomic's arrival order: the same bits on every call.  No workgroup waits on another; enqueue-only, no
 *   host read, no synchronisation, no scratch.
 * work: mggcn_radix_sort_work_bytes(n_seg, seg_len) bytes of device memory, 4-byte aligned.  n_seg == 0 or seg_len == 0
 * returns without a launch (work_bytes gives 0).  Refused before any launch: 0 <= begin_bit < end_bit <= 32 violated;
 * n_seg seg_len >= 2^31; a work_bytes below the function's; any overlap among the four arrays. */
#define MGGCN_RADIX_SORT_TILE 4096
size_t mggcn_radix_sort_work_bytes(size_t n_seg, size_t seg_len);
void mggcn_radix_sort_pairs_u32(mggcn_stream_t stream, size_t n_seg, size_t seg_len, uint32_t *keys, uint32_t *vals,
                                uint32_t *keys_alt, uint32_t *vals_alt, int begin_bit, int end_bit, void *work,
                                size_t work_bytes);

/* The integers behind ROC-AUC of a multi-label model (csrc/roc_auc.hip; no reference counterpart).
 *   keys    reads columns [c0, c0 + nc) of the row-major fp32 logits, of the int32 targets (non-zero = positive) and the
 *           int32 sets (NULL: every row is slot 0), n rows each, and writes class-major keys[(c - c0) n + i], vals likewise:
 *             key   = x = logit + 0.0f (so -0.0 ties with +0.0, as a float compare does), u = bits(x),
 *                     (u >> 31) ? ~u : (u | 0x80000000): monotone over every finite value and both infinities.  A NaN
 *                     falls where this map puts its bit pattern (sign clear: above +inf; sign set: below -inf).
 *             value = slot << 1 | (target != 0), slot 0 train / 1 val / 2 test / 3 anything else.
 *           The matrices are read along their rows and transposed through LDS; the stores are 64 consecutive rows of a
 *           class.  n nc < 2^31; c0 + nc within both leading dimensions.
 *   stats   over the nc segments of n pairs SORTED ascending on the key (mggcn_radix_sort_pairs_u32): stats[c][k] =
 *           (2U, P, N), three u64, k = train, val, test, other, all ("all": every row).  P / N: the positives / negatives of
 *           slot k; 2U = sum over the positives p of slot k of 2 #{negatives of slot k with key < key_p} + #{negatives of
 *           slot k with key == key_p}: ties count one half, AUC = 2U / (2 P N).  Tie groups of any length across any number
 *           of chunks (MGGCN_ROC_AUC_CHUNK pairs per wave) are exact.  Everything is an integer, summed in a fixed order
 *           (partials per chunk, one workgroup per class); 2U <= 2 P N < 2^63.  Four launches, no atomics, no host read.
 *           work: mggcn_roc_auc_stats_work_bytes(n, nc) bytes of device memory, 8-byte aligned.  n == 0 writes zeros. */
#define MGGCN_ROC_AUC_CHUNK 1024
void mggcn_roc_auc_keys_f32(mggcn_stream_t stream, const float *logits, size_t ld_logits, const int32_t *targets,
                            size_t ld_targets, const int32_t *sets, size_t n, size_t c0, size_t nc, uint32_t *keys,
                            uint32_t *vals);
size_t mggcn_roc_auc_stats_work_bytes(size_t n, size_t nc);
void mggcn_roc_auc_stats_u64(mggcn_stream_t stream, const uint32_t *keys, const uint32_t *vals, size_t n, size_t nc,
                             uint64_t *stats, void *work, size_t work_bytes);

/* cublasSasum(src/cuda_utils.hpp:362-371)  *result_device = sum |A[i]|.
 * Unlike cuBLAS' host-pointer mode this does NOT block: the sum lands in device
 * memory on `stream` (fixed-order two-level reduction -> reproducible); the host
 * wrapper copies it back after its own sync (src/gcn.hpp:816-817). */
void mggcn_abssum_f32(mggcn_stream_t stream, const float *A, size_t size, float *result_device);

/* Halo pack: dst[k, 0:d] = src[indices[k], 0:d] for k < n_indices.
 * The reference has no counterpart -- its exchange broadcasts whole shards
 * (src/dist_matrix.hpp:458-467); the rows packed here are the ones its data-prep script counts
 * as communication volume (test/data/prep.py:237-244).  indices: device, uint32. */
void mggcn_gather_rows_f32(mggcn_stream_t stream, const float *src, size_t ld_src, const uint32_t *indices,
                           size_t n_indices, uint32_t d, float *dst, size_t ld_dst);

/* ======================================================================== *
 * Fused tail kernels.  Same math as the chains above,
 * fewer passes over [n x C] / fewer launches.
 * ======================================================================== */
/* softmax + argmax + log-prob + gradient in one pass over the logits, in place:
 * the 8-launch chain of softmax::operator() (src/gcn.hpp:651-675) +
 * softmax_cross_entropy_loss::operator() (src/gcn.hpp:785-818):
 *   O = softmax(H) row-wise (max-subtracted); P = argmax (first wins);
 *   loss_terms[i] = log O[i, Y[i]];  correct[i] = (Y[i] == P[i]);
 *   H <- (O - onehot(Y)) * grad_scale           (grad_scale = 1 / n_global)
 *   sums[0] += sum_i |loss_terms[i]|, sums[1] += sum_i correct[i]  (the caller zeroes sums;
 *   workgroup partials are added in a fixed order by a one-workgroup second launch:
 *   bitwise reproducible, no atomics). */
void mggcn_softmax_xent_fused_f32(mggcn_stream_t stream, float *H, const int32_t *Y, size_t n_rows,
                                  size_t m, float grad_scale, float *sums_device);
/* The same pass out of place: reads `logits`, writes the gradient to G (G == logits is the call above).  With
 * copy = true the reference copies the logits before its in-place chain (src/gcn.hpp:653-656, :787): here the copy
 * is the pass itself. */
void mggcn_softmax_xent_fused_from_f32(mggcn_stream_t stream, const float *logits, float *G, const int32_t *Y,
                                       size_t n_rows, size_t m, float grad_scale, float *sums_device);
/* The split-aware form of the pass above.  The reference loads sets.bin (0 train / 1 validation /
 * 2 test) and ignores it, src/main.cpp:85: its loss, gradient and accuracy run over ALL vertices.  Here S[i] is row i's
 * set, train_set is 0, 1 or 2, and slot(s) = s for 0 <= s <= 2, 3 for every other value (rows in no split, padding):
 *   G[i, :] = (O[i, :] - onehot(Y[i])) * grad_scale  if S[i] == train_set, else +0.0 in EVERY column (written, not
 *             skipped: G may alias the logits, and the backward GEMMs read every row);
 *   sums[2k] += sum over slot(S[i]) == k of |loss_terms[i]|,  sums[2k+1] += the same of correct[i],  k = 0..3
 *   (eight floats, zeroed by the caller; grad_scale = 1 / the GLOBAL number of training rows).
 * 1 <= m <= 1024 and G == logits allowed, as above.  Same grid, row order and fixed-order final sum as
 * mggcn_softmax_xent_fused_from_f32 (four pairs of workgroup partials instead of one, no atomics): bitwise reproducible,
 * and with S == train_set everywhere G and the training slot's pair are bit for bit those of the call above. */
void mggcn_softmax_xent_split_from_f32(mggcn_stream_t stream, const float *logits, float *G, const int32_t *Y,
                                       const int32_t *S, size_t n_rows, size_t m, int32_t train_set, float grad_scale,
                                       float *sums_device);
/* Multi-label loss (no counterpart in the reference, whose vertices have exactly one class): sigmoid + binary
 * cross-entropy + gradient + the counts behind micro-F1 in one pass.  logits, G and T are contiguous [n_rows x m], any
 * m >= 1 (no row-wise reduction, so no 1024-column limit), G == logits allowed; T is int32, non-zero = positive.  S is the
 * split-aware form's n_rows x 1 set vector with the slots of the call above; S == NULL: every row is in slot 0 and trains.
 * Per element, with z the logit, t in {0, 1}, softplus(x) = max(x, 0) + log1pf(expf(-|x|)):
 *   loss = t ? softplus(-z) : softplus(z)            (never inf - inf: z = +-inf gives 0 or +inf, not NaN)
 *   p    = z >= 0 ? 1 / (1 + expf(-z)) : expf(z) / (1 + expf(z))
 *   G    = (p - t) * grad_scale if the row trains (S == NULL or S[i] == train_set), else +0.0 (written, not skipped)
 *   pred = z > 0                                     (+-0 and NaN predict negative)
 *   sums[4k + 0..3] += loss sum, TP, FP, FN counts over the rows of slot k   (MGGCN_BCE_SUMS floats, zeroed by the
 *   caller; grad_scale = 1 / (the GLOBAL number of training rows x m); micro-F1 = 2 TP / (2 TP + FP + FN)).
 * No atomics: sixteen partials per workgroup go to the per-(device, stream) scratch and a one-workgroup final pass adds
 * them in a fixed order, so two calls on the same input give the same bits.  A slot gets its contributions by selects: a
 * NaN or inf in a row of slot k reaches slot k's loss sum only.  The counts are sums of per-thread integers held in fp32:
 * every workgroup partial and the total are exact while a count stays below 2^24 per slot, an fp32-rounded sum above (like
 * the correct counts of the softmax form).  G is element-wise: an element's bits depend neither on the grid, nor on the
 * other rows (rows [a, b) alone give the bits they have in the whole call), nor on the load path -- 16-byte loads when
 * m % 4 == 0 and all three matrices are 16-byte aligned, single elements otherwise; the SUMS of the two paths may differ in
 * their last bits.  With S == NULL, G and sums[0..3] are bit for bit G and slot train_set's four sums of a call with
 * S[i] == train_set everywhere.  n_rows == 0 returns; m >= 1, non-null logits / G / T / sums and train_set in 0..2 are
 * checked. */
#define MGGCN_BCE_SUMS 16u
void mggcn_sigmoid_bce_from_f32(mggcn_stream_t stream, const float *logits, float *G, const int32_t *T, const int32_t *S,
                                size_t n_rows, size_t m, int32_t train_set, float grad_scale, float *sums_device);
/* The two steps the unfused chain (src/gcn.hpp:785-818) needs to do the same, next to sets.bin being loaded and ignored at
 * src/main.cpp:85.  select_rows_by_set: row i of the [size / m x m] matrix stays if S[i] == set, else becomes +0.0. */
void mggcn_select_rows_by_set_f32(mggcn_stream_t stream, float *mat, const int32_t *S, int32_t set, size_t size,
                                  size_t m);
/* abssum_by_set: result[k] = sum over slot(S[i]) == k of |x[i]|, k = 0..3 (four floats, overwritten): the per-split form
 * of mggcn_abssum_f32, the same fixed-order two-level reduction. */
void mggcn_abssum_by_set_f32(mggcn_stream_t stream, const float *x, const int32_t *S, size_t n, float *result_device);
/* One launch for linear::adam_update on a parameter tensor (src/gcn.hpp:146-172):
 *   g += wd*p; m = b1*m + (1-b1)*g; v = b2*v + (1-b2)*g*g;
 *   p -= (lr/c1) * m / (sqrt(v/c2) + eps)      (g is updated in place like the reference) */
void mggcn_adam_fused_f32(mggcn_stream_t stream, float *param, float *grad, float *m, float *v,
                          float lr, float beta1, float beta2, float weight_decay, float c1, float c2,
                          float eps, size_t size);

/* The same update for EVERY parameter tensor of a model in one launch (the reference runs seven launches per
 * layer, src/gcn.hpp:146-172: 28 per epoch on the 4-layer Reddit model; this is 1).  `table_device`: n_tensors
 * entries in DEVICE memory, built once (the pointers of a model never change); first_block = running sum of
 * mggcn_adam_multi_blocks(size) over the preceding entries, total_blocks = the sum over all.  lr / beta / c1 /
 * c2 / eps are shared (every layer takes the same step count); weight_decay is per tensor (0 for biases).
 * Element-wise math identical to mggcn_adam_fused_f32 -> bitwise equal results. */
typedef struct {
    float *param, *grad, *m, *v;
    uint64_t size;
    float weight_decay;
    uint32_t first_block;
} mggcn_adam_tensor;
uint32_t mggcn_adam_multi_blocks(uint64_t size);
void mggcn_adam_multi_f32(mggcn_stream_t stream, const mggcn_adam_tensor *table_device, uint32_t n_tensors,
                          uint32_t total_blocks, float lr, float beta1, float beta2, float c1, float c2, float eps);

/* ======================================================================== *
 * Host-side graph preprocessing (multi-threaded CPU code, runs once per dataset;
 * the reference does the same work on the host with parallel STL).
 * All pointers are HOST pointers.
 * ======================================================================== */
/* csr_matrix::normalize(axis) (src/matrix.hpp:340-390): axis==0 row-normalise,
 * axis!=0 column-normalise (what gcn uses, src/gcn.hpp:947).  Race-free and
 * deterministic (the reference's parallel column sums race, src/matrix.hpp:353-357). */
void mggcn_csr_normalize_host(uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                              const uint32_t *indices, float *values, int axis);
/* csr_matrix::transpose() (src/matrix.hpp:392-453).  Outputs: t_indptr[n_cols+1],
 * t_indices[nnz], t_values[nnz].  Within a transposed row, entries are in increasing
 * source-row order (the reference's serial order; its parallel path is unordered). */
void mggcn_csr_transpose_host(uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                              const uint32_t *indices, const float *values, uint32_t *t_indptr,
                              uint32_t *t_indices, float *t_values);
/* dist_row_csr_matrix ctor for one row block (src/dist_matrix.hpp:215-259):
 * rows [row_begin,row_end) are cut at the column boundaries q[0..nq] into nq CSR
 * blocks with block-local column indices.
 *   count: blk_indptr is nq*(rows+1) u32, block j at offset j*(rows+1)
 *   fill : blk_indices[j] / blk_values[j] sized blk_indptr[j][rows] */
void mggcn_csr_block_split_count_host(const uint32_t *indptr, const uint32_t *indices,
                                      uint32_t row_begin, uint32_t row_end, const uint32_t *q,
                                      uint32_t nq, uint32_t *blk_indptr);
void mggcn_csr_block_split_fill_host(const uint32_t *indptr, const uint32_t *indices,
                                     const float *values, uint32_t row_begin, uint32_t row_end,
                                     const uint32_t *q, uint32_t nq, const uint32_t *blk_indptr,
                                     uint32_t *const *blk_indices, float *const *blk_values);
/* dn_matrix::init(gain) (src/matrix.hpp:539-545): std::default_random_engine(99),
 * U(-g, g) with g = gain*sqrt(3/n_rows), row-major fill.  gain < 0 selects the
 * reference default sqrt(2/(1+0.01^2)). */
void mggcn_init_uniform_host(float *buffer, size_t n_rows, size_t n_cols, float gain);

#ifdef __cplusplus
}
#endif
#endif /* MGGCN_H_ */
