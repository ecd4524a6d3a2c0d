// gat_b16.hip -- the three sparse GAT kernels on a bf16 image of the gathered operand (mggcn_gat_*_bf16): the templates of
// gat_kernels.h instantiated with uint16_t where gat.hip instantiates them with float.  Z is the image in forward and
// backward_dst, G in backward_src; s_dst, s_src, lse, D, the row's own operands, the sums and every output stay fp32.  Each
// entry point is the twin of the _f32 one named next to it in mggcn.h: the same checks, the same (VEC, NT, U) for operands
// equally aligned in elements, and the bits of the _f32 call on the exactly widened image.  No record form.
#include "common.h"
#include "gat_internal.h"
#include "gat_kernels.h"

// the scores and the column-sum pass stay in gat.hip: nothing here instantiates them
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"

// ============================ C ABI =========================================
MGGCN_API void mggcn_gat_forward_bf16(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                      const uint32_t *indices, const uint16_t *Z, size_t ldz, const float *s_dst,
                                      const float *s_src, uint32_t K, uint32_t dh, float slope, float *out, size_t ldo,
                                      float *lse) {
    gat_forward(stream, n_rows, n_cols, indptr, indices, Z, ldz, s_dst, s_src, K, dh, slope, out, ldo, lse, nullptr);
}

MGGCN_API void mggcn_gat_backward_dst_bf16(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                           const uint32_t *indices, const uint16_t *Z, size_t ldz, const float *s_dst,
                                           const float *s_src, const float *lse, const float *G, size_t ldg, const float *out,
                                           size_t ldo, uint32_t K, uint32_t dh, float slope, float *D, float *ds_dst) {
    gat_backward_dst(stream, n_rows, n_cols, indptr, indices, Z, ldz, s_dst, s_src, lse, G, ldg, out, ldo, K, dh, slope, D, ds_dst,
                     nullptr);
}

MGGCN_API void mggcn_gat_backward_src_bf16(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                                           const uint32_t *t_indices, const float *Z, size_t ldz, const float *s_dst,
                                           const float *s_src, const float *lse, const float *D, const uint16_t *G, size_t ldg,
                                           const float *att, const float *ds_dst, uint32_t K, uint32_t dh, float slope,
                                           float *ds_src, float *G_Z, size_t ldgz) {
    gat_backward_src(stream, n_rows, n_cols, t_indptr, t_indices, Z, ldz, s_dst, s_src, lse, D, nullptr, G, ldg, att, ds_dst, K,
                     dh, slope, ds_src, G_Z, ldgz, nullptr);
}

// The _drop twins: threshold == 0 launches the plain kernels, as the _drop_f32 entry points do
MGGCN_API void mggcn_gat_forward_drop_bf16(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                           const uint32_t *indices, const uint16_t *Z, size_t ldz, const float *s_dst,
                                           const float *s_src, uint32_t K, uint32_t dh, float slope, float *out, size_t ldo,
                                           float *lse, uint32_t threshold, float scale, uint64_t seed, uint32_t dropout_stream,
                                           uint32_t dst0, uint32_t src0) {
    const gat_drop dp = make_gat_drop(threshold, scale, seed, dropout_stream, dst0, n_rows, src0, n_cols);
    gat_forward(stream, n_rows, n_cols, indptr, indices, Z, ldz, s_dst, s_src, K, dh, slope, out, ldo, lse,
                threshold ? &dp : nullptr);
}

MGGCN_API void mggcn_gat_backward_dst_drop_bf16(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                                const uint32_t *indices, const uint16_t *Z, size_t ldz, const float *s_dst,
                                                const float *s_src, const float *lse, const float *G, size_t ldg,
                                                const float *out, size_t ldo, uint32_t K, uint32_t dh, float slope, float *D,
                                                float *ds_dst, uint32_t threshold, float scale, uint64_t seed,
                                                uint32_t dropout_stream, uint32_t dst0, uint32_t src0) {
    const gat_drop dp = make_gat_drop(threshold, scale, seed, dropout_stream, dst0, n_rows, src0, n_cols);
    gat_backward_dst(stream, n_rows, n_cols, indptr, indices, Z, ldz, s_dst, s_src, lse, G, ldg, out, ldo, K, dh, slope, D, ds_dst,
                     threshold ? &dp : nullptr);
}

// rows of F^T are sources (offset src0), its entries destinations (offset dst0)
MGGCN_API void mggcn_gat_backward_src_drop_bf16(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols,
                                                const uint32_t *t_indptr, const uint32_t *t_indices, const float *Z, size_t ldz,
                                                const float *s_dst, const float *s_src, const float *lse, const float *D,
                                                const uint16_t *G, size_t ldg, const float *att, const float *ds_dst, uint32_t K,
                                                uint32_t dh, float slope, float *ds_src, float *G_Z, size_t ldgz,
                                                uint32_t threshold, float scale, uint64_t seed, uint32_t dropout_stream,
                                                uint32_t dst0, uint32_t src0) {
    const gat_drop dp = make_gat_drop(threshold, scale, seed, dropout_stream, dst0, n_cols, src0, n_rows);
    gat_backward_src(stream, n_rows, n_cols, t_indptr, t_indices, Z, ldz, s_dst, s_src, lse, D, nullptr, G, ldg, att, ds_dst, K,
                     dh, slope, ds_src, G_Z, ldgz, threshold ? &dp : nullptr);
}
