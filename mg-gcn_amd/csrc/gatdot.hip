// gatdot.hip -- dot-product (transformer) attention over a graph (Vaswani et al.; Shi et al.: UniMP; PyG's TransformerConv
// without root weight, gate and edge features) on gfx950.  The score is the scaled dot product of a query and a key,
//     e_ijk = c (Zq[i, head k] . Zk[j, head k]),   alpha_ijk = softmax over the entries j of row i,
//     out[i, head k] = sum_j alpha_ijk Zv[j, head k],
// so every entry needs TWO dense head-rows of its source -- the key it is scored with and the value it contributes -- and the
// attention has no parameter of its own.
//
// Layout: gatv2.hip's -- one wave per CSR row, walked in 64-entry chunks by entry_chunks (gat_internal.h), the heads one after
// the other, G = 64 / LPR groups of LPR lanes that each hold one head-row of a neighbour, (VEC, NT, U) variants.
//   * forward: ONE pass over a row.  The group that gathered a neighbour's key computes its score (dot_head_row against the
//     destination's query, group_sum) and hands it with the neighbour's value row to group_softmax (gat_internal.h): the
//     running maximum, sum and accumulators per group, the groups' meeting at the wave's maximum and the fold, gatv2.hip's
//     word for word.  Both gathers of the U unrolled entries are issued before the first butterfly.
//   * backward_dst (rows of F): D[i, k] = G . out, and per entry e and dalpha = G[i] . Zv[j] as two butterflies,
//     ds = exp(e - lse)(dalpha - D), accq += ds Zk[j]; G_Zq = c accq.
//   * backward_src (rows of F^T): the row's own key and value head-rows stay in registers, lse and D of the entry's
//     destination are the walk's two scalars, the destination's Zq and G head-rows are gathered; accK += ds Zq[i],
//     accV += alpha G[i]; G_Zk = c accK, G_Zv = accV.
// Every dense operand is a pointer with a leading dimension of its own: the model passes the thirds of one [n x 3 out]
// buffer.  Nothing of nnz x K is stored, no atomics, a row's result depends on that row alone: the same bits on every call and
// for every split of the rows between calls.
#include <algorithm>
#include <cmath>

// no parameter, so no G_att: the column-sum pass of gat_internal.h (and reduce.h's final kernel behind it) is never instantiated here
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"

// The three kernels and the bodies of their entry points are the templates of gatdot_kernels.h; this file instantiates them
// on fp32 gathered operands (mggcn_gatdot_*_f32) and gatdot_b16.hip on bf16 images (mggcn_gatdot_*_bf16).
#include "common.h"
#include "gat_internal.h"
#include "gatdot_kernels.h"
#include "reduce.h"

// ============================ C ABI =========================================
MGGCN_API void mggcn_gatdot_forward_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                        const uint32_t *indices, const float *Zq, size_t ldq, const float *Zk, size_t ldk,
                                        const float *Zv, size_t ldv, uint32_t K, uint32_t dh, float scale, float *out, size_t ldo,
                                        float *lse) {
    gatdot_forward(stream, n_rows, n_cols, indptr, indices, Zq, ldq, Zk, ldk, Zv, ldv, K, dh, scale, out, ldo, lse);
}

MGGCN_API void mggcn_gatdot_backward_dst_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                             const uint32_t *indices, const float *Zq, size_t ldq, const float *Zk, size_t ldk,
                                             const float *Zv, size_t ldv, const float *lse, const float *G, size_t ldg,
                                             const float *out, size_t ldo, uint32_t K, uint32_t dh, float scale, float *D,
                                             float *G_Zq, size_t ldgzq) {
    gatdot_backward_dst(stream, n_rows, n_cols, indptr, indices, Zq, ldq, Zk, ldk, Zv, ldv, lse, G, ldg, out, ldo, K, dh, scale, D,
                        G_Zq, ldgzq);
}

MGGCN_API void mggcn_gatdot_backward_src_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                                             const uint32_t *t_indices, const float *Zq, size_t ldq, const float *Zk, size_t ldk,
                                             const float *Zv, size_t ldv, const float *lse, const float *D, const float *G,
                                             size_t ldg, uint32_t K, uint32_t dh, float scale, float *G_Zk, size_t ldgzk,
                                             float *G_Zv, size_t ldgzv) {
    gatdot_backward_src(stream, n_rows, n_cols, t_indptr, t_indices, Zq, ldq, Zk, ldk, Zv, ldv, lse, D, G, ldg, K, dh, scale, G_Zk,
                        ldgzk, G_Zv, ldgzv);
}
