// gat.hip -- graph attention (GAT) on gfx950: attention scores, the edge-softmax fused with the gather, and the
// backward pass (per-edge dot products + weighted transposed gather + the column sums behind G_att).
//
// Layout of the three sparse kernels: the row-split form of spmm.hip without a plan -- one wave per CSR row, the row's
// entries in 64-entry chunks, software-pipelined (entry_chunks of gat_internal.h is the walk).  The heads of a row are
// walked one after the other.  Within a head the wave is cut into G = 64 / LPR groups of LPR lanes (LPR: the power of two
// that covers one head's dh columns, 64 at the most): a group holds one head-row of a dense operand, VEC columns per lane
// and NT column tiles when dh > LPR * VEC, so one wave-instruction gathers the head-rows of G neighbours.
//   * per chunk, the lane that owns an entry has its index and its [rows x K] scalars (scores, lse, D) from the walk and
//     evaluates exp ONCE per (entry, head); the groups pick index and weight up through ds_bpermute (chunk_entry);
//   * the forward makes ONE pass over a row: a running maximum, the sum and the accumulators rescaled chunk by chunk;
//   * the per-edge dot product (SDDMM) is a butterfly over the LPR lanes of a group -- log2(LPR) steps per G edges;
//   * the sums over a row's entries fold the G groups in a fixed order at the end: no atomics anywhere, the same bits on
//     every call.
// No per-edge array exists: alpha is recomputed from s_dst, s_src and lse wherever it is needed.  The one exception is on
// request: gat_alpha_kernel (mggcn_gat_alpha_f32) runs the same walk and writes alpha out for the user; nothing reads it back.
// VEC = 4 (16-byte loads) when dh % 4 == 0 and every dense operand and leading dimension is 16-byte aligned -- a float4
// must not straddle two heads, so K * dh % 4 == 0 alone is not enough -- and VEC = 1 otherwise.
// Heavy rows are slow here (one wave walks a whole row, ~21 k entries on the Reddit-shaped graph) but correct: cutting
// them with a fixed-order combine is what the SpMM's plan does and is left to a plan for these kernels.
// Attention dropout (DROP = true, the mggcn_gat_*_drop_f32 entry points): the lane that owns an entry draws its keep bit
// from Philox on (source, destination, head) next to the exp, and the factor q = keep ? 1 / (1 - p) : 0 travels to the
// groups through the same __shfl as the weight.  The softmax itself (maximum, sum, lse) takes every entry.  Nothing is
// stored: the backward kernels draw the same words again, backward_src with the roles of row and entry swapped.  Duplicate
// entries (i, j) share one bit.  DROP = false compiles to the kernels as they were.
// The packed destination record (REC = true, the mggcn_gat_backward_src_rec*_f32 entry points): backward_src reads (s_dst,
// lse, D) of an entry's destination as ONE 16-byte load from rec[(i K + k) 4 + {0, 1, 2}] (gat_pack_dst_kernel writes it; the
// fourth float is padding nobody reads) where the plain kernel gathers three 4-byte scalars.  Only the loads differ: the
// arithmetic, and so every bit of ds_src and G_Z, is the plain kernel's.  REC = false compiles to the kernels as they were.
#include <algorithm>
#include <cmath>

// The three sparse kernels and the bodies of their entry points are the templates of gat_kernels.h; this file instantiates
// them on an fp32 gathered operand (mggcn_gat_*_f32) and gat_b16.hip on a bf16 image (mggcn_gat_*_bf16).
#include "common.h"
#include "gat_internal.h"
#include "gat_kernels.h"
#include "philox.h"
#include "reduce.h"

namespace {

// ---------------------------------------------------------------------------
// s_dst[r, k] = Z[r, head k] . att[0, head k],  s_src[r, k] = Z[r, head k] . att[1, head k]
// one wave per row, G heads at a time (one per group)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gat_scores_kernel(const float *__restrict__ Z, size_t ldz, const float *__restrict__ att,
                                                         float *__restrict__ s_dst, float *__restrict__ s_src, size_t n_rows,
                                                         uint32_t K, uint32_t dh, uint32_t lg) {
    MGGCN_GAT_WAVE_ROW(n_rows);
    const float *__restrict__ z = Z + row * ldz;
    const uint32_t width = K * dh;
    for (uint32_t k0 = 0; k0 < K; k0 += n_grp) {
        const uint32_t k = k0 + grp;
        float pd = 0.f, ps = 0.f;
        if (k < K)
            for (uint32_t c = sub; c < dh; c += lpr) {
                const float v = z[k * dh + c];
                pd = fmaf(v, att[k * dh + c], pd);
                ps = fmaf(v, att[width + k * dh + c], ps);
            }
        pd = group_sum(pd, lpr);
        ps = group_sum(ps, lpr);
        if (k < K && sub == 0) {
            if (s_dst) s_dst[row * K + k] = pd;
            if (s_src) s_src[row * K + k] = ps;
        }
    }
}

// ---------------------------------------------------------------------------
// rec[(i K + k) 4 + {0, 1, 2, 3}] = s_dst[i, k], lse[i, k], D[i, k], 0: one thread per (destination, head), one 16-byte store
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gat_pack_dst_kernel(const float *__restrict__ s_dst, const float *__restrict__ lse,
                                                           const float *__restrict__ D, size_t n, float4 *__restrict__ rec) {
    const size_t ik = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (ik < n) rec[ik] = make_float4(s_dst[ik], lse[ik], D[ik], 0.f);
}

// ---------------------------------------------------------------------------
// the export: alpha[p, k] = exp(lrelu(s_dst[i, k] + s_src[j, k]) - lse[i, k]) for entry p = (i, j) of the indices array --
// the float expression of the two backward kernels above.  The same walk, KV heads at a time: the lane that owns an entry
// has its KV source scores from the walk and stores its KV coefficients (KV = 4: one 16-byte store).  No groups, no
// reduction, no LDS; a value depends on its entry and its row's lse alone.
// ---------------------------------------------------------------------------
template <int KV>
__global__ __launch_bounds__(256) void gat_alpha_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                        const uint32_t *__restrict__ indices,
                                                        const float *__restrict__ s_dst, const float *__restrict__ s_src,
                                                        const float *__restrict__ lse, uint32_t K, float slope,
                                                        float *__restrict__ alpha, size_t lda) {
    const uint32_t lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (row >= n_rows) return;
    const uint32_t beg = indptr[row], end = indptr[row + 1];
    for (uint32_t k0 = 0; k0 < K; k0 += KV) {
        float sd[KV], ls[KV];
#pragma unroll
        for (int v = 0; v < KV; v++) {
            sd[v] = s_dst[row * K + k0 + v];
            ls[v] = lse[row * K + k0 + v];
        }
        const auto fetch = [&](uint32_t c, float *s) {          // the entry's scores of heads k0 .. k0 + KV
#pragma unroll
            for (int v = 0; v < KV; v++) s[v] = s_src[(size_t)c * K + k0 + v];
        };
        entry_chunks<KV> ch;
        ch.start(indices, beg, end, lane, fetch);
        for (uint32_t base = beg; base < end; base += 64) {
            ch.next(indices, base, end, lane, fetch);
            if (lane < ch.cnt) {
                float a[KV];
#pragma unroll
                for (int v = 0; v < KV; v++) a[v] = expf(gat_lrelu(sd[v] + ch.my_s[v], slope) - ls[v]);
                storev<KV>(alpha + ((size_t)base + lane) * lda + k0, a);
            }
        }
    }
}

// G_att[0, c] = sum_i ds_dst[i, k(c)] Z_dst[i, c],  G_att[1, c] = sum_j ds_src[j, k(c)] Z_src[j, c]: the term of
// gat_column_sums, side 0 the destinations and side 1 the sources
struct gat_scores_term {
    const float *ds[2], *Z[2];
    size_t ld[2], n[2];
    uint32_t K, dh;
    __device__ size_t rows(int side) const { return n[side]; }
    __device__ uint32_t head(uint32_t c) const { return c / dh; }
    __device__ float operator()(int side, size_t r, uint32_t c, uint32_t k, float acc) const {
        return fmaf(ds[side][r * K + k], Z[side][r * ld[side] + c], acc);
    }
};

}  // namespace

// ============================ C ABI =========================================
MGGCN_API void mggcn_gat_scores_f32(mggcn_stream_t stream, const float *Z, size_t ldz, const float *att, float *s_dst,
                                    float *s_src, size_t n_rows, uint32_t K, uint32_t dh) {
    require_heads(K, dh);
    MGGCN_REQUIRE(ldz >= (size_t)K * dh, "gat scores: ldz < heads * width per head");
    MGGCN_REQUIRE(n_rows <= 0xFFFFFFFFu, "gat scores: more than 2^32 - 1 rows");
    if (!n_rows || (!s_dst && !s_src)) return;
    MGGCN_REQUIRE(Z != nullptr && att != nullptr, "gat scores: null operand");
    const uint32_t lg = std::min(ceil_log2(dh), 6u);
    launch_rows(gat_scores_kernel, n_rows, stream, Z, ldz, att, s_dst, s_src, n_rows, K, dh, lg);
}

MGGCN_API void mggcn_gat_forward_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                     const uint32_t *indices, const float *Z, size_t ldz, const float *s_dst,
                                     const float *s_src, uint32_t K, uint32_t dh, float slope, float *out, size_t ldo,
                                     float *lse) {
    gat_forward(stream, n_rows, n_cols, indptr, indices, Z, ldz, s_dst, s_src, K, dh, slope, out, ldo, lse, nullptr);
}

MGGCN_API void mggcn_gat_backward_dst_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                          const uint32_t *indices, const float *Z, size_t ldz, const float *s_dst,
                                          const float *s_src, const float *lse, const float *G, size_t ldg, const float *out,
                                          size_t ldo, uint32_t K, uint32_t dh, float slope, float *D, float *ds_dst) {
    gat_backward_dst(stream, n_rows, n_cols, indptr, indices, Z, ldz, s_dst, s_src, lse, G, ldg, out, ldo, K, dh, slope, D, ds_dst,
                     nullptr);
}

MGGCN_API void mggcn_gat_backward_src_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                                          const uint32_t *t_indices, const float *Z, size_t ldz, const float *s_dst,
                                          const float *s_src, const float *lse, const float *D, const float *G, size_t ldg,
                                          const float *att, const float *ds_dst, uint32_t K, uint32_t dh, float slope,
                                          float *ds_src, float *G_Z, size_t ldgz) {
    gat_backward_src(stream, n_rows, n_cols, t_indptr, t_indices, Z, ldz, s_dst, s_src, lse, D, nullptr, G, ldg, att, ds_dst, K,
                     dh, slope, ds_src, G_Z, ldgz, nullptr);
}

// The _drop twins: threshold == 0 (p = 0: every entry kept, scale = 1) launches the plain kernels, so the bits are the plain
// entry point's by construction; the index ranges are still checked.
MGGCN_API void mggcn_gat_forward_drop_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                          const uint32_t *indices, const float *Z, size_t ldz, const float *s_dst,
                                          const float *s_src, uint32_t K, uint32_t dh, float slope, float *out, size_t ldo,
                                          float *lse, uint32_t threshold, float scale, uint64_t seed, uint32_t dropout_stream,
                                          uint32_t dst0, uint32_t src0) {
    const gat_drop dp = make_gat_drop(threshold, scale, seed, dropout_stream, dst0, n_rows, src0, n_cols);
    gat_forward(stream, n_rows, n_cols, indptr, indices, Z, ldz, s_dst, s_src, K, dh, slope, out, ldo, lse,
                threshold ? &dp : nullptr);
}

MGGCN_API void mggcn_gat_backward_dst_drop_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                               const uint32_t *indices, const float *Z, size_t ldz, const float *s_dst,
                                               const float *s_src, const float *lse, const float *G, size_t ldg,
                                               const float *out, size_t ldo, uint32_t K, uint32_t dh, float slope, float *D,
                                               float *ds_dst, uint32_t threshold, float scale, uint64_t seed,
                                               uint32_t dropout_stream, uint32_t dst0, uint32_t src0) {
    const gat_drop dp = make_gat_drop(threshold, scale, seed, dropout_stream, dst0, n_rows, src0, n_cols);
    gat_backward_dst(stream, n_rows, n_cols, indptr, indices, Z, ldz, s_dst, s_src, lse, G, ldg, out, ldo, K, dh, slope, D, ds_dst,
                     threshold ? &dp : nullptr);
}

// rows of F^T are sources (offset src0), its entries destinations (offset dst0)
MGGCN_API void mggcn_gat_backward_src_drop_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                                               const uint32_t *t_indices, const float *Z, size_t ldz, const float *s_dst,
                                               const float *s_src, const float *lse, const float *D, const float *G, size_t ldg,
                                               const float *att, const float *ds_dst, uint32_t K, uint32_t dh, float slope,
                                               float *ds_src, float *G_Z, size_t ldgz, uint32_t threshold, float scale,
                                               uint64_t seed, uint32_t dropout_stream, uint32_t dst0, uint32_t src0) {
    const gat_drop dp = make_gat_drop(threshold, scale, seed, dropout_stream, dst0, n_cols, src0, n_rows);
    gat_backward_src(stream, n_rows, n_cols, t_indptr, t_indices, Z, ldz, s_dst, s_src, lse, D, nullptr, G, ldg, att, ds_dst, K,
                     dh, slope, ds_src, G_Z, ldgz, threshold ? &dp : nullptr);
}

// The packed destination record: rec[(i K + k) 4 + {0, 1, 2, 3}] = s_dst[i, k], lse[i, k], D[i, k], 0
MGGCN_API void mggcn_gat_pack_dst_f32(mggcn_stream_t stream, const float *s_dst, const float *lse, const float *D,
                                      size_t n_rows, uint32_t K, float *rec) {
    MGGCN_REQUIRE(K >= 1 && K <= MGGCN_GAT_MAX_HEADS, "gat supports 1 <= heads <= 16");
    MGGCN_REQUIRE(n_rows <= 0xFFFFFFFFu, "gat pack: more than 2^32 - 1 rows");
    if (!n_rows) return;
    MGGCN_REQUIRE(s_dst != nullptr && lse != nullptr && D != nullptr && rec != nullptr, "gat pack: null operand");
    MGGCN_REQUIRE(aligned16(rec), "gat pack: rec must be 16-byte aligned");
    const size_t n = n_rows * K;
    hipLaunchKernelGGL(gat_pack_dst_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), s_dst, lse, D, n,
                       reinterpret_cast<float4 *>(rec));
    MGGCN_CHECK_LAUNCH();
}

// backward_src on the record: rec in the place of s_dst, lse and D; the bits of the plain call on the arrays it was packed from
MGGCN_API void mggcn_gat_backward_src_rec_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                                              const uint32_t *t_indices, const float *Z, size_t ldz, const float *rec,
                                              const float *s_src, const float *G, size_t ldg, const float *att,
                                              const float *ds_dst, uint32_t K, uint32_t dh, float slope, float *ds_src,
                                              float *G_Z, size_t ldgz) {
    MGGCN_REQUIRE(!n_rows || !n_cols || (rec != nullptr && aligned16(rec)), "gat backward: rec must be 16-byte aligned");
    gat_backward_src(stream, n_rows, n_cols, t_indptr, t_indices, Z, ldz, nullptr, s_src, nullptr, nullptr, rec, G, ldg, att,
                     ds_dst, K, dh, slope, ds_src, G_Z, ldgz, nullptr);
}

MGGCN_API void mggcn_gat_backward_src_rec_drop_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols,
                                                   const uint32_t *t_indptr, const uint32_t *t_indices, const float *Z,
                                                   size_t ldz, const float *rec, const float *s_src, const float *G, size_t ldg,
                                                   const float *att, const float *ds_dst, uint32_t K, uint32_t dh, float slope,
                                                   float *ds_src, float *G_Z, size_t ldgz, uint32_t threshold, float scale,
                                                   uint64_t seed, uint32_t dropout_stream, uint32_t dst0, uint32_t src0) {
    MGGCN_REQUIRE(!n_rows || !n_cols || (rec != nullptr && aligned16(rec)), "gat backward: rec must be 16-byte aligned");
    const gat_drop dp = make_gat_drop(threshold, scale, seed, dropout_stream, dst0, n_cols, src0, n_rows);
    gat_backward_src(stream, n_rows, n_cols, t_indptr, t_indices, Z, ldz, nullptr, s_src, nullptr, nullptr, rec, G, ldg, att,
                     ds_dst, K, dh, slope, ds_src, G_Z, ldgz, threshold ? &dp : nullptr);
}

// The export of the coefficients: the only GAT call that writes something of nnz x K, and nothing calls it but the user
MGGCN_API void mggcn_gat_alpha_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                   const uint32_t *indices, const float *s_dst, const float *s_src, const float *lse,
                                   uint32_t K, float slope, float *alpha, size_t lda) {
    MGGCN_REQUIRE(K >= 1 && K <= MGGCN_GAT_MAX_HEADS, "gat supports 1 <= heads <= 16");
    MGGCN_REQUIRE(lda >= K, "gat alpha: lda < heads");
    if (!n_rows) return;
    MGGCN_REQUIRE(indptr != nullptr && s_dst != nullptr && lse != nullptr, "gat alpha: null operand");
    MGGCN_REQUIRE(n_cols == 0 || (indices != nullptr && s_src != nullptr && alpha != nullptr), "gat alpha: null operand");
    MGGCN_REQUIRE(alpha != s_dst && alpha != s_src && alpha != lse, "gat alpha: alpha must not alias s_dst, s_src or lse");
    if (K % 4 == 0 && rows16(alpha, lda))
        launch_rows(gat_alpha_kernel<4>, n_rows, stream, n_rows, indptr, indices, s_dst, s_src, lse, K, slope, alpha, lda);
    else
        launch_rows(gat_alpha_kernel<1>, n_rows, stream, n_rows, indptr, indices, s_dst, s_src, lse, K, slope, alpha, lda);
}

MGGCN_API void mggcn_gat_scores_backward_f32(mggcn_stream_t stream, const float *ds_dst, const float *Z_dst, size_t ldzd,
                                             size_t n_dst, const float *ds_src, const float *Z_src, size_t ldzs, size_t n_src,
                                             uint32_t K, uint32_t dh, float *G_att) {
    require_heads(K, dh);
    const uint32_t width = K * dh;
    MGGCN_REQUIRE(ldzd >= width && ldzs >= width, "gat scores backward: leading dimension < heads * width per head");
    MGGCN_REQUIRE(G_att != nullptr, "gat scores backward: null gradient");
    MGGCN_REQUIRE(n_dst == 0 || (ds_dst != nullptr && Z_dst != nullptr), "gat scores backward: null operand");
    MGGCN_REQUIRE(n_src == 0 || (ds_src != nullptr && Z_src != nullptr), "gat scores backward: null operand");
    gat_column_sums<2>(stream, gat_scores_term{{ds_dst, ds_src}, {Z_dst, Z_src}, {ldzd, ldzs}, {n_dst, n_src}, K, dh},
                       std::max(n_dst, n_src), width, G_att);
}
