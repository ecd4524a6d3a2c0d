// gatv2.hip -- dynamic graph attention (GATv2; Brody, Alon, Yahav: "How Attentive are Graph Attention Networks?") on
// gfx950.  The score has its non-linearity INSIDE the dot product,
//     t_ijk[c] = Zd[i, k dh + c] + Zs[j, k dh + c],   e_ijk = sum_c att[k dh + c] lrelu(t_ijk[c]),
// so the score of an entry exists only after the source's head-row has been gathered: there are no [rows x K] score
// scalars to stream, and every sparse kernel computes e with the group butterfly on the rows it gathers anyway.
//
// Layout: gat.hip's -- one wave per CSR row, walked in 64-entry chunks by entry_chunks (gat_internal.h), the heads one
// after the other, G = 64 / LPR groups of LPR lanes that each hold one head-row of a neighbour, (VEC, NT, U) variants.
//   * forward: ONE pass over a row with one gather of Zs per entry.  The group that gathered a neighbour computes its score,
//     so the running maximum is kept PER GROUP and the groups meet at the wave's maximum at the end: group_softmax
//     (gat_internal.h) is that softmax, the kernel keeps its prologue loads, its gather and its partial score.
//   * backward_dst (rows of F): D, G_Zd and P[i] = sum_j ds_ijk u_ijk, row i's share of G_att; e and dalpha are two
//     butterflies over the same gathered row.
//   * backward_src (rows of F^T): gathers the destination's head-rows of Zd and G, recomputes e, dalpha, alpha and ds, and
//     accumulates alpha G_i + v.  lse and D of the destination are two 4-byte gathers by the lane that owns the entry
//     (the walk's scalars), or, in the REC form, one 8-byte load of the packed (lse, D) record that pack_dst writes: what
//     the row-partitioned model gathers from the other ranks in one collective.
//   * att_grad: the column sums of P through gat_column_sums (gat_internal.h).
//   * alpha (the export, on request): backward_dst cut down to its score, writing exp(e - lse) per (entry, head).
// Nothing of nnz x K is stored (but what the export is asked to write), no atomics, a row's result depends on that row
// alone: the same bits on every call and for every split of the rows between calls.
#include <algorithm>
#include <cmath>

// The three sparse kernels and the bodies of their entry points are the templates of gatv2_kernels.h; this file instantiates
// them on fp32 gathered operands (mggcn_gatv2_*_f32) and gatv2_b16.hip on bf16 images (mggcn_gatv2_*_bf16).
#include "common.h"
#include "gat_internal.h"
#include "gatv2_kernels.h"
#include "reduce.h"

namespace {

// ---------------------------------------------------------------------------
// rec[(i K + k) 2 + {0, 1}] = lse[i, k], D[i, k]: one thread per (destination, head), one 8-byte store
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gatv2_pack_dst_kernel(const float *__restrict__ lse, const float *__restrict__ D,
                                                             size_t n, float2 *__restrict__ rec) {
    const size_t ik = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (ik < n) rec[ik] = make_float2(lse[ik], D[ik]);
}

// ---------------------------------------------------------------------------
// the export: alpha[p, k] = exp(e_ijk - lse[i, k]) for entry p = (i, j) of the indices array -- backward_dst cut down to its
// score: the same gather of the source's head-row, the same partial products and butterfly, the same expf.  One lane of
// the group that holds the entry stores the value; a value depends on its entry and its row's lse alone.
// ---------------------------------------------------------------------------
template <int VEC, int NT, int U>
__global__ __launch_bounds__(256) void gatv2_alpha_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                          const uint32_t *__restrict__ indices,
                                                          const float *__restrict__ Zs, size_t ldzs,
                                                          const float *__restrict__ Zd, size_t ldzd,
                                                          const float *__restrict__ att, const float *__restrict__ lse,
                                                          uint32_t K, uint32_t dh, float slope, uint32_t lg,
                                                          float *__restrict__ alpha, size_t lda) {
    MGGCN_GAT_WAVE_ROW(n_rows);
    const uint32_t beg = indptr[row], end = indptr[row + 1];
    for (uint32_t k = 0; k < K; k++) {
        float zd[NT][VEC], a[NT][VEC];
        load_head_row<VEC, NT>(zd, Zd + row * ldzd + (size_t)k * dh, lpr, sub, dh);
        load_head_row<VEC, NT>(a, att + (size_t)k * dh, lpr, sub, dh);
        const float ls = lse[row * K + k];
        const float *__restrict__ Zk = Zs + (size_t)k * dh;
        entry_chunks<0> ch;                         // the indices alone
        ch.start(indices, beg, end, lane, no_scalars);
        for (uint32_t base = beg; base < end; base += 64) {
            ch.next(indices, base, end, lane, no_scalars);
            const uint32_t cnt = ch.cnt;
            for (uint32_t j = 0; j < cnt; j += n_grp * U) {
                float pe[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const chunk_entry en = ch.pick(j, u, n_grp, grp);
                    float z[NT][VEC];
                    load_head_row<VEC, NT>(z, Zk + (size_t)en.c * ldzs, lpr, sub, dh, en.ok);
                    pe[u] = score_head_row<VEC, NT>(a, zd, z, slope);
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const chunk_entry en = ch.pick(j, u, n_grp, grp);
                    const float e = group_sum(pe[u], lpr);
                    if (en.ok && sub == 0) alpha[((size_t)base + en.src) * lda + k] = expf(e - ls);
                }
            }
        }
    }
}

// G_att[0, c] = sum_i P[i, c]: the term of gat_column_sums, one side
struct gatv2_att_term {
    const float *P;
    size_t ldp, n;
    __device__ size_t rows(int) const { return n; }
    __device__ uint32_t head(uint32_t) const { return 0; }
    __device__ float operator()(int, size_t r, uint32_t c, uint32_t, float acc) const { return acc + P[r * ldp + c]; }
};

}  // namespace

// ============================ C ABI =========================================
MGGCN_API void mggcn_gatv2_forward_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                       const uint32_t *indices, const float *Zs, size_t ldzs, const float *Zd, size_t ldzd,
                                       const float *att, uint32_t K, uint32_t dh, float slope, float *out, size_t ldo,
                                       float *lse) {
    gatv2_forward(stream, n_rows, n_cols, indptr, indices, Zs, ldzs, Zd, ldzd, att, K, dh, slope, out, ldo, lse);
}

MGGCN_API void mggcn_gatv2_backward_dst_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                            const uint32_t *indices, const float *Zs, size_t ldzs, const float *Zd,
                                            size_t ldzd, const float *att, const float *lse, const float *G, size_t ldg,
                                            const float *out, size_t ldo, uint32_t K, uint32_t dh, float slope, float *D,
                                            float *G_Zd, size_t ldgzd, float *P, size_t ldp) {
    gatv2_backward_dst(stream, n_rows, n_cols, indptr, indices, Zs, ldzs, Zd, ldzd, att, lse, G, ldg, out, ldo, K, dh, slope, D, G_Zd,
                       ldgzd, P, ldp);
}

// The export of the coefficients: the only GATv2 call that writes something of nnz x K, and nothing calls it but the user.
// alpha is stored element by element, so its alignment plays no part in the choice of the variant: the bits of a value do
// not depend on where it lands.
MGGCN_API void mggcn_gatv2_alpha_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                     const uint32_t *indices, const float *Zs, size_t ldzs, const float *Zd, size_t ldzd,
                                     const float *att, const float *lse, uint32_t K, uint32_t dh, float slope, float *alpha,
                                     size_t lda) {
    require_heads(K, dh);
    const size_t width = (size_t)K * dh;
    MGGCN_REQUIRE(ldzs >= width && ldzd >= width, "gatv2 alpha: leading dimension < heads * width per head");
    MGGCN_REQUIRE(lda >= K, "gatv2 alpha: lda < heads");
    if (!n_rows) return;
    MGGCN_REQUIRE(indptr != nullptr && Zd != nullptr && att != nullptr && lse != nullptr, "gatv2 alpha: null operand");
    MGGCN_REQUIRE(n_cols == 0 || (indices != nullptr && Zs != nullptr && alpha != nullptr), "gatv2 alpha: null operand");
    MGGCN_REQUIRE(alpha != Zs && alpha != Zd && alpha != att && alpha != lse, "gatv2 alpha: alpha must not alias an input");
    const bool vec = dh % 4 == 0 && rows16(Zs, ldzs) && rows16(Zd, ldzd) && aligned16(att);
    const head_geometry hg = head_geometry_for(dh, vec);
    gat_dispatch(vec, hg.nt, [&](auto v) {
        launch_rows(gatv2_alpha_kernel<v.VEC, v.NT, v.U>, n_rows, stream, n_rows, indptr, indices, Zs, ldzs, Zd, ldzd, att, lse, K,
                    dh, slope, hg.lg, alpha, lda);
    });
}

MGGCN_API void mggcn_gatv2_att_grad_f32(mggcn_stream_t stream, const float *P, size_t ldp, size_t n_rows, uint32_t width,
                                        float *G_att) {
    MGGCN_REQUIRE(width >= 1 && width <= MGGCN_GAT_MAX_WIDTH, "gatv2 att grad supports 1 <= width <= 1024");
    MGGCN_REQUIRE(ldp >= width, "gatv2 att grad: ldp < width");
    MGGCN_REQUIRE(G_att != nullptr, "gatv2 att grad: null gradient");
    MGGCN_REQUIRE(n_rows == 0 || P != nullptr, "gatv2 att grad: null operand");
    gat_column_sums<1>(stream, gatv2_att_term{P, ldp, n_rows}, n_rows, width, G_att);
}

MGGCN_API void mggcn_gatv2_backward_src_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                                            const uint32_t *t_indices, const float *Zs, size_t ldzs, const float *Zd,
                                            size_t ldzd, const float *att, const float *lse, const float *D, const float *G,
                                            size_t ldg, uint32_t K, uint32_t dh, float slope, float *G_Zs, size_t ldgzs) {
    gatv2_backward_src(stream, n_rows, n_cols, t_indptr, t_indices, Zs, ldzs, Zd, ldzd, att, lse, D, nullptr, G, ldg, K, dh, slope,
                       G_Zs, ldgzs);
}

// The packed destination record: rec[(i K + k) 2 + {0, 1}] = lse[i, k], D[i, k]
MGGCN_API void mggcn_gatv2_pack_dst_f32(mggcn_stream_t stream, const float *lse, const float *D, size_t n_rows, uint32_t K,
                                        float *rec) {
    MGGCN_REQUIRE(K >= 1 && K <= MGGCN_GAT_MAX_HEADS, "gat supports 1 <= heads <= 16");
    MGGCN_REQUIRE(n_rows <= 0xFFFFFFFFu, "gatv2 pack: more than 2^32 - 1 rows");
    if (!n_rows) return;
    MGGCN_REQUIRE(lse != nullptr && D != nullptr && rec != nullptr, "gatv2 pack: null operand");
    MGGCN_REQUIRE(((uintptr_t)rec & 7) == 0, "gatv2 pack: rec must be 8-byte aligned");
    const size_t n = n_rows * K;
    hipLaunchKernelGGL(gatv2_pack_dst_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), lse, D, n,
                       reinterpret_cast<float2 *>(rec));
    MGGCN_CHECK_LAUNCH();
}

// backward_src on the record: rec in the place of lse and D; the bits of the plain call on the arrays it was packed from
MGGCN_API void mggcn_gatv2_backward_src_rec_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols,
                                                const uint32_t *t_indptr, const uint32_t *t_indices, const float *Zs,
                                                size_t ldzs, const float *Zd, size_t ldzd, const float *att, const float *rec,
                                                const float *G, size_t ldg, uint32_t K, uint32_t dh, float slope, float *G_Zs,
                                                size_t ldgzs) {
    MGGCN_REQUIRE(!n_rows || !n_cols || (rec != nullptr && ((uintptr_t)rec & 7) == 0), "gatv2 backward: rec must be 8-byte aligned");
    gatv2_backward_src(stream, n_rows, n_cols, t_indptr, t_indices, Zs, ldzs, Zd, ldzd, att, nullptr, nullptr, rec, G, ldg, K, dh,
                       slope, G_Zs, ldgzs);
}
