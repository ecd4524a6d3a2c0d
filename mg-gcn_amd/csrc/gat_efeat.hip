// gat_efeat.hip -- graph attention with edge features in the score: the mggcn_gat_*_efeat_f32 entry points and their _drop
// twins.  gat_edge.h states the edge term and how P_e is formed; the kernels and the bodies of the entry points are the
// templates of gat_kernels.h, which this file instantiates with a gat_edge -- fp32, no record -- where gat.hip instantiates
// them without.  A translation unit of its own: gat.hip's instantiations are not touched, and the build stays parallel.
// No atomics, the same bits on every call, and every row-local output the same bits for every split of the rows.
#include "common.h"
#include "gat_kernels.h"

namespace {

// the edge operands of an entry point, checked; has_entries: the call walks at least one entry
gat_edge make_gat_edge(const float *E, size_t lde, const float *att_edge, uint32_t de, bool has_entries) {
    MGGCN_REQUIRE(de >= 1 && de <= MGGCN_GAT_MAX_EDGE_DIM, "gat efeat supports 1 <= edge dimension <= 16");
    MGGCN_REQUIRE(lde >= de, "gat efeat: lde < edge dimension");
    MGGCN_REQUIRE(att_edge != nullptr && (!has_entries || E != nullptr), "gat efeat: null edge operand");
    return {E, att_edge, lde, de, de % 4 == 0 && rows16(E, lde)};
}

}  // namespace

// ============================ C ABI =========================================
MGGCN_API void mggcn_gat_forward_efeat_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                           const uint32_t *indices, const float *Z, size_t ldz, const float *s_dst,
                                           const float *s_src, uint32_t K, uint32_t dh, float slope, float *out, size_t ldo,
                                           float *lse, const float *E, size_t lde, const float *att_edge, uint32_t de) {
    gat_forward(stream, n_rows, n_cols, indptr, indices, Z, ldz, s_dst, s_src, K, dh, slope, out, ldo, lse, nullptr,
                make_gat_edge(E, lde, att_edge, de, n_rows && n_cols));
}

MGGCN_API void mggcn_gat_backward_dst_efeat_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                                const uint32_t *indices, const float *Z, size_t ldz, const float *s_dst,
                                                const float *s_src, const float *lse, const float *G, size_t ldg,
                                                const float *out, size_t ldo, uint32_t K, uint32_t dh, float slope, float *D,
                                                float *ds_dst, const float *E, size_t lde, const float *att_edge, uint32_t de,
                                                float *P_e, size_t ldp) {
    gat_backward_dst(stream, n_rows, n_cols, indptr, indices, Z, ldz, s_dst, s_src, lse, G, ldg, out, ldo, K, dh, slope, D, ds_dst,
                     nullptr, P_e, ldp, make_gat_edge(E, lde, att_edge, de, n_rows && n_cols));
}

MGGCN_API void mggcn_gat_backward_src_efeat_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols,
                                                const uint32_t *t_indptr, const uint32_t *t_indices, const float *Z, size_t ldz,
                                                const float *s_dst, const float *s_src, const float *lse, const float *D,
                                                const float *G, size_t ldg, const float *att, const float *ds_dst, uint32_t K,
                                                uint32_t dh, float slope, float *ds_src, float *G_Z, size_t ldgz, const float *E,
                                                size_t lde, const float *att_edge, uint32_t de) {
    gat_backward_src(stream, n_rows, n_cols, t_indptr, t_indices, Z, ldz, s_dst, s_src, lse, D, nullptr, G, ldg, att, ds_dst, K,
                     dh, slope, ds_src, G_Z, ldgz, nullptr, make_gat_edge(E, lde, att_edge, de, n_rows && n_cols));
}

// The _drop twins: threshold == 0 launches the plain efeat kernels, as the _drop twins of gat.hip do; the ranges are checked.
MGGCN_API void mggcn_gat_forward_efeat_drop_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                                const uint32_t *indices, const float *Z, size_t ldz, const float *s_dst,
                                                const float *s_src, uint32_t K, uint32_t dh, float slope, float *out, size_t ldo,
                                                float *lse, uint32_t threshold, float scale, uint64_t seed,
                                                uint32_t dropout_stream, uint32_t dst0, uint32_t src0, const float *E, size_t lde,
                                                const float *att_edge, uint32_t de) {
    const gat_drop dp = make_gat_drop(threshold, scale, seed, dropout_stream, dst0, n_rows, src0, n_cols);
    gat_forward(stream, n_rows, n_cols, indptr, indices, Z, ldz, s_dst, s_src, K, dh, slope, out, ldo, lse,
                threshold ? &dp : nullptr, make_gat_edge(E, lde, att_edge, de, n_rows && n_cols));
}

MGGCN_API void mggcn_gat_backward_dst_efeat_drop_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols,
                                                     const uint32_t *indptr, const uint32_t *indices, const float *Z, size_t ldz,
                                                     const float *s_dst, const float *s_src, const float *lse, const float *G,
                                                     size_t ldg, const float *out, size_t ldo, uint32_t K, uint32_t dh,
                                                     float slope, float *D, float *ds_dst, uint32_t threshold, float scale,
                                                     uint64_t seed, uint32_t dropout_stream, uint32_t dst0, uint32_t src0,
                                                     const float *E, size_t lde, const float *att_edge, uint32_t de, float *P_e,
                                                     size_t ldp) {
    const gat_drop dp = make_gat_drop(threshold, scale, seed, dropout_stream, dst0, n_rows, src0, n_cols);
    gat_backward_dst(stream, n_rows, n_cols, indptr, indices, Z, ldz, s_dst, s_src, lse, G, ldg, out, ldo, K, dh, slope, D, ds_dst,
                     threshold ? &dp : nullptr, P_e, ldp, make_gat_edge(E, lde, att_edge, de, n_rows && n_cols));
}

// rows of F^T are sources (offset src0), its entries destinations (offset dst0)
MGGCN_API void mggcn_gat_backward_src_efeat_drop_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols,
                                                     const uint32_t *t_indptr, const uint32_t *t_indices, const float *Z,
                                                     size_t ldz, const float *s_dst, const float *s_src, const float *lse,
                                                     const float *D, const float *G, size_t ldg, const float *att,
                                                     const float *ds_dst, uint32_t K, uint32_t dh, float slope, float *ds_src,
                                                     float *G_Z, size_t ldgz, uint32_t threshold, float scale, uint64_t seed,
                                                     uint32_t dropout_stream, uint32_t dst0, uint32_t src0, const float *E,
                                                     size_t lde, const float *att_edge, uint32_t de) {
    const gat_drop dp = make_gat_drop(threshold, scale, seed, dropout_stream, dst0, n_cols, src0, n_rows);
    gat_backward_src(stream, n_rows, n_cols, t_indptr, t_indices, Z, ldz, s_dst, s_src, lse, D, nullptr, G, ldg, att, ds_dst, K,
                     dh, slope, ds_src, G_Z, ldgz, threshold ? &dp : nullptr,
                     make_gat_edge(E, lde, att_edge, de, n_rows && n_cols));
}
