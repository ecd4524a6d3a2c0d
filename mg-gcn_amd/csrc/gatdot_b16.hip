// gatdot_b16.hip -- the three sparse kernels of dot-product attention on bf16 images of the gathered operands
// (mggcn_gatdot_*_bf16): the templates of gatdot_kernels.h instantiated with uint16_t where gatdot.hip instantiates them
// with float.  Zk and Zv are the images in forward and backward_dst, Zq and G in backward_src -- two gathered operands per
// call, so this is the variant that moves the most bytes per entry; lse, D, the row's own operands, the sums and every
// output stay fp32.  Each entry point is the twin of the _f32 one named next to it in mggcn.h: the same checks, the same
// (VEC, NT, U) for operands equally aligned in elements, and the bits of the _f32 call on the exactly widened images.
#include <algorithm>
#include <cmath>

// no parameter, so no G_att: the column-sum pass of gat_internal.h (and reduce.h's final kernel behind it) is never instantiated here
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"

#include "common.h"
#include "gat_internal.h"
#include "gatdot_kernels.h"

// ============================ C ABI =========================================
MGGCN_API void mggcn_gatdot_forward_bf16(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                         const uint32_t *indices, const float *Zq, size_t ldq, const uint16_t *Zk, size_t ldk,
                                         const uint16_t *Zv, size_t ldv, uint32_t K, uint32_t dh, float scale, float *out,
                                         size_t ldo, float *lse) {
    gatdot_forward(stream, n_rows, n_cols, indptr, indices, Zq, ldq, Zk, ldk, Zv, ldv, K, dh, scale, out, ldo, lse);
}

MGGCN_API void mggcn_gatdot_backward_dst_bf16(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                              const uint32_t *indices, const float *Zq, size_t ldq, const uint16_t *Zk,
                                              size_t ldk, const uint16_t *Zv, size_t ldv, const float *lse, const float *G,
                                              size_t ldg, const float *out, size_t ldo, uint32_t K, uint32_t dh, float scale,
                                              float *D, float *G_Zq, size_t ldgzq) {
    gatdot_backward_dst(stream, n_rows, n_cols, indptr, indices, Zq, ldq, Zk, ldk, Zv, ldv, lse, G, ldg, out, ldo, K, dh, scale, D,
                        G_Zq, ldgzq);
}

MGGCN_API void mggcn_gatdot_backward_src_bf16(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                                              const uint32_t *t_indices, const uint16_t *Zq, size_t ldq, const float *Zk,
                                              size_t ldk, const float *Zv, size_t ldv, const float *lse, const float *D,
                                              const uint16_t *G, size_t ldg, uint32_t K, uint32_t dh, float scale, float *G_Zk,
                                              size_t ldgzk, float *G_Zv, size_t ldgzv) {
    gatdot_backward_src(stream, n_rows, n_cols, t_indptr, t_indices, Zq, ldq, Zk, ldk, Zv, ldv, lse, D, G, ldg, K, dh, scale, G_Zk,
                        ldgzk, G_Zv, ldgzv);
}
