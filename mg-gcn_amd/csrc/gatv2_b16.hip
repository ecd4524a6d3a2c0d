// gatv2_b16.hip -- the three sparse GATv2 kernels on bf16 images of the gathered operands (mggcn_gatv2_*_bf16): the
// templates of gatv2_kernels.h instantiated with uint16_t where gatv2.hip instantiates them with float.  Zs is the image in
// forward and backward_dst, Zd and G in backward_src; att, lse, D, the row's own operands, the sums and every output stay
// fp32.  Each entry point is the twin of the _f32 one named next to it in mggcn.h: the same checks, the same (VEC, NT, U)
// for operands equally aligned in elements, and the bits of the _f32 call on the exactly widened images.  No record form,
// no export.
#include "common.h"
#include "gat_internal.h"
#include "gatv2_kernels.h"

// the column-sum pass behind G_att stays in gatv2.hip: nothing here instantiates it
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"

// ============================ C ABI =========================================
MGGCN_API void mggcn_gatv2_forward_bf16(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                        const uint32_t *indices, const uint16_t *Zs, size_t ldzs, const float *Zd, size_t ldzd,
                                        const float *att, uint32_t K, uint32_t dh, float slope, float *out, size_t ldo,
                                        float *lse) {
    gatv2_forward(stream, n_rows, n_cols, indptr, indices, Zs, ldzs, Zd, ldzd, att, K, dh, slope, out, ldo, lse);
}

MGGCN_API void mggcn_gatv2_backward_dst_bf16(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                             const uint32_t *indices, const uint16_t *Zs, size_t ldzs, const float *Zd,
                                             size_t ldzd, const float *att, const float *lse, const float *G, size_t ldg,
                                             const float *out, size_t ldo, uint32_t K, uint32_t dh, float slope, float *D,
                                             float *G_Zd, size_t ldgzd, float *P, size_t ldp) {
    gatv2_backward_dst(stream, n_rows, n_cols, indptr, indices, Zs, ldzs, Zd, ldzd, att, lse, G, ldg, out, ldo, K, dh, slope, D, G_Zd,
                       ldgzd, P, ldp);
}

MGGCN_API void mggcn_gatv2_backward_src_bf16(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                                             const uint32_t *t_indices, const float *Zs, size_t ldzs, const uint16_t *Zd,
                                             size_t ldzd, const float *att, const float *lse, const float *D, const uint16_t *G,
                                             size_t ldg, uint32_t K, uint32_t dh, float slope, float *G_Zs, size_t ldgzs) {
    gatv2_backward_src(stream, n_rows, n_cols, t_indptr, t_indices, Zs, ldzs, Zd, ldzd, att, lse, D, nullptr, G, ldg, K, dh, slope,
                       G_Zs, ldgzs);
}
