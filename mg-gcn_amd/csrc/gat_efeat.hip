// gat_efeat.hip -- the three sparse GAT kernels with edge features in the score (mggcn_gat_*_efeat_f32 and their _drop twins;
// PyG's GATConv(edge_dim = de) with lin_edge and att_edge folded into one [K x de] matrix U = att_edge):
//   t_pk = fmaf(E[p, de - 1], U[k, de - 1], ... fmaf(E[p, 0], U[k, 0], 0.f)),   x_ijk = (s_dst[i, k] + s_src[j, k]) + t_pk
// for entry p = (i, j) of the CSR the kernel walks; everything after x is gat_kernels.h's kernel of the same name, statement
// for statement: the one-pass softmax, lse, D, ds, the gather and DROP's q.  A translation unit of its own: the kernels of
// gat.hip and their instantiations are not touched, and the build stays parallel.
//   * The edge term belongs to a POSITION, not to an index: the lane that owns entry l of a chunk owns row base + l of E.  The
//     walk (entry_chunks of gat_internal.h, unchanged) calls its fetch for exactly one position per call -- beg + lane from
//     start(), base + 64 + lane from next() -- so the fetch reads that position from a variable the kernel sets before the
//     call (`pos`) and t rides as one more scalar of the walk, loaded and folded one chunk ahead like s_src.
//   * U[k, :] is wave-uniform per head and read through a uniform pointer; a row of E is read with 16-byte loads when
//     de % 4 == 0 and base and lde are aligned for them (a run-time, wave-uniform choice), element by element otherwise.
//     Both paths run the one fmaf chain, c ascending, so forward over F, backward_dst over F and backward_src over F^T give
//     an edge the same x, and so the same alpha, whichever copy of E they read.
//   * P_e[i, k de + c] = sum_j ds_ijk E[p, c], the row's share of G_att_edge (backward_dst): ds of an entry is formed by the
//     group that gathered it and handed BACK to the lane that owns the entry (one __shfl per step of a turn), and the owner
//     adds ds E[p, :] to its de accumulators once per chunk -- 64 lanes read 64 consecutive rows of E, the access of the
//     edge term itself.  A lane's entries in row order, then the lanes through wave_sum.  (Letting lane `sub` of the
//     gathering group add column sub of the entry's row, the obvious geometry, costs one scattered 4 de-byte read per
//     entry and group: 1.7 x the plain kernel at 128 columns / 4 heads and 3 x at 41 / 1, profiles/experiments/gat_efeat.log.)
//     The accumulators are a register array indexed by constants: no scratch.  The column sums of P_e are
//     mggcn_gatv2_att_grad_f32's.
// No atomics, the same bits on every call, and every row-local output the same bits for every split of the rows.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "gat_internal.h"
#include "gat_kernels.h"
#include "philox.h"
#include "reduce.h"

namespace {

constexpr int kEdgeSlots = MGGCN_GAT_MAX_EDGE_DIM;      // columns of E one lane can own: de <= 16 at LPR = 1

// the edge operands of a call; vec: a row of E may be read four columns at a time
struct gat_edge {
    const float *E, *U;
    size_t lde;
    uint32_t de;
    bool vec;
};

// t of position `pos` at the head whose row of U is Uk: the one chain of the contract, c ascending
__device__ __forceinline__ float edge_term(const gat_edge &eg, const float *__restrict__ Uk, size_t pos) {
    const float *__restrict__ Ep = eg.E + pos * eg.lde;
    float t = 0.f;
    if (eg.vec) {
        for (uint32_t c = 0; c < eg.de; c += 4) {
            const float4 e = *reinterpret_cast<const float4 *>(Ep + c);
            t = fmaf(e.x, Uk[c], t);
            t = fmaf(e.y, Uk[c + 1], t);
            t = fmaf(e.z, Uk[c + 2], t);
            t = fmaf(e.w, Uk[c + 3], t);
        }
    } else {
        for (uint32_t c = 0; c < eg.de; c++) t = fmaf(Ep[c], Uk[c], t);
    }
    return t;
}

// pe[c] += ds E[pos, c] for c < de: the share of one entry in its row's P_e, on the lane that owns the entry.  The loops are
// unrolled over all sixteen slots with a wave-uniform test each, so pe is indexed by constants and stays in registers.
__device__ __forceinline__ void edge_axpy(const gat_edge &eg, size_t pos, float ds, float (&pe)[kEdgeSlots]) {
    const float *__restrict__ Ep = eg.E + pos * eg.lde;
    if (eg.vec) {
#pragma unroll
        for (int c = 0; c < kEdgeSlots; c += 4) {
            if ((uint32_t)c < eg.de) {
                const float4 e = *reinterpret_cast<const float4 *>(Ep + c);
                pe[c] = fmaf(ds, e.x, pe[c]);
                pe[c + 1] = fmaf(ds, e.y, pe[c + 1]);
                pe[c + 2] = fmaf(ds, e.z, pe[c + 2]);
                pe[c + 3] = fmaf(ds, e.w, pe[c + 3]);
            }
        }
    } else {
#pragma unroll
        for (int c = 0; c < kEdgeSlots; c++)
            if ((uint32_t)c < eg.de) pe[c] = fmaf(ds, Ep[c], pe[c]);
    }
}

// ---------------------------------------------------------------------------
// forward: gat_forward_kernel with x = (s_dst + s_src) + t
// ---------------------------------------------------------------------------
template <int VEC, int NT, int U, bool DROP>
__global__ __launch_bounds__(256) void gat_forward_efeat_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                                const uint32_t *__restrict__ indices,
                                                                const float *__restrict__ Z, size_t ldz,
                                                                const float *__restrict__ s_dst,
                                                                const float *__restrict__ s_src, uint32_t K, uint32_t dh,
                                                                float slope, uint32_t lg, float *__restrict__ out, size_t ldo,
                                                                float *__restrict__ lse, gat_drop dp, gat_edge eg) {
    MGGCN_GAT_WAVE_ROW(n_rows);
    const uint32_t beg = indptr[row], end = indptr[row + 1];
    for (uint32_t k = 0; k < K; k++) {
        const float sd = s_dst[row * K + k];
        const float *__restrict__ Zk = Z + (size_t)k * dh;
        const float *__restrict__ Uk = eg.U + (size_t)k * eg.de;
        float m = -INFINITY, sum = 0.f;
        float acc[NT][VEC];
        zero_head_row<VEC, NT>(acc);
        size_t pos = (size_t)beg + lane;                    // the position the next fetch is for
        const auto fetch = [&](uint32_t c, float *s) {
            s[0] = s_src[(size_t)c * K + k];
            s[1] = edge_term(eg, Uk, pos);
        };
        entry_chunks<2> ch;
        ch.start(indices, beg, end, lane, fetch);
        for (uint32_t base = beg; base < end; base += 64) {
            pos = (size_t)base + 64 + lane;
            ch.next(indices, base, end, lane, fetch);
            const uint32_t cnt = ch.cnt;
            const float my_x = ch.my_s[0], my_t = ch.my_s[1];
            const float e = lane < cnt ? gat_lrelu((sd + my_x) + my_t, slope) : -INFINITY;
            const float m_new = fmaxf(m, wave_max(e));
            const float scale = expf(m - m_new);            // 0 at the first chunk (m = -inf), where sum and acc are 0
            float my_a = lane < cnt ? expf(e - m_new) : 0.f;
            sum = fmaf(sum, scale, wave_sum(my_a));
            m = m_new;
            if constexpr (DROP) {                            // after the sum: only the accumulator's weight carries q
                if (lane < cnt) my_a *= gat_keep_scale(dp, dp.dst0 + (uint32_t)row, dp.src0 + ch.my_c, k);
            }
            if (scale != 1.f) {                              // wave-uniform
#pragma unroll
                for (int t = 0; t < NT; t++)
#pragma unroll
                    for (int v = 0; v < VEC; v++) acc[t][v] *= scale;
            }
            for (uint32_t j = 0; j < cnt; j += n_grp * U) {
                float z[U][NT][VEC], a[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const chunk_entry en = ch.pick(j, u, n_grp, grp);
                    const float av = en.of(my_a);
                    a[u] = en.ok ? av : 0.f;
                    load_head_row<VEC, NT>(z[u], Zk + (size_t)en.c * ldz, lpr, sub, dh, en.ok);
                }
#pragma unroll
                for (int u = 0; u < U; u++) axpy_head_row<VEC, NT>(acc, a[u], z[u]);
            }
        }
        const float inv = beg < end ? 1.f / sum : 0.f;
        if (lane == 0) lse[row * K + k] = beg < end ? m + logf(sum) : 0.f;
        fold_store_head_row<VEC, NT>(out + row * ldo + (size_t)k * dh, acc, lpr, sub, grp, dh,
                                     [&](int, int, float x) { return x * inv; });      // an empty row: +0.0
    }
}

// ---------------------------------------------------------------------------
// backward over the rows of F: gat_backward_dst_kernel with the edge term in x, and P_e[i, k de + c] = sum_j ds_ijk E[p, c]
// ---------------------------------------------------------------------------
template <int VEC, int NT, int U, bool DROP>
__global__ __launch_bounds__(256) void gat_backward_dst_efeat_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                                     const uint32_t *__restrict__ indices,
                                                                     const float *__restrict__ Z, size_t ldz,
                                                                     const float *__restrict__ s_dst,
                                                                     const float *__restrict__ s_src,
                                                                     const float *__restrict__ lse, const float *__restrict__ G,
                                                                     size_t ldg, const float *__restrict__ out, size_t ldo,
                                                                     uint32_t K, uint32_t dh, float slope, uint32_t lg,
                                                                     float *__restrict__ D, float *__restrict__ ds_dst,
                                                                     gat_drop dp, gat_edge eg, float *__restrict__ P_e,
                                                                     size_t ldp) {
    MGGCN_GAT_WAVE_ROW(n_rows);
    const uint32_t beg = indptr[row], end = indptr[row + 1];
    for (uint32_t k = 0; k < K; k++) {
        float g[NT][VEC];
        load_head_row<VEC, NT>(g, G + row * ldg + (size_t)k * dh, lpr, sub, dh);
        const float Dk = head_row_D<VEC, NT>(g, out + row * ldo + (size_t)k * dh, lpr, sub, grp, dh);
        const float sd = s_dst[row * K + k], ls = lse[row * K + k];
        const float *__restrict__ Zk = Z + (size_t)k * dh;
        const float *__restrict__ Uk = eg.U + (size_t)k * eg.de;
        float acc = 0.f;
        float pe[kEdgeSlots];
#pragma unroll
        for (int q = 0; q < kEdgeSlots; q++) pe[q] = 0.f;
        size_t pos = (size_t)beg + lane;
        const auto fetch = [&](uint32_t c, float *s) {
            s[0] = s_src[(size_t)c * K + k];
            s[1] = edge_term(eg, Uk, pos);
        };
        entry_chunks<2> ch;
        ch.start(indices, beg, end, lane, fetch);
        for (uint32_t base = beg; base < end; base += 64) {
            pos = (size_t)base + 64 + lane;
            ch.next(indices, base, end, lane, fetch);
            const uint32_t cnt = ch.cnt;
            const float my_x = ch.my_s[0], my_t = ch.my_s[1];
            float my_w = 0.f;                       // alpha lrelu'(x) of my entry
            [[maybe_unused]] float my_q = 0.f;
            if (lane < cnt) {
                const float x = (sd + my_x) + my_t;
                my_w = expf(gat_lrelu(x, slope) - ls) * (x > 0.f ? 1.f : slope);
                if constexpr (DROP) my_q = gat_keep_scale(dp, dp.dst0 + (uint32_t)row, dp.src0 + ch.my_c, k);
            }
            float my_ds = 0.f;                      // ds of my entry, handed back by the group that formed it
            for (uint32_t j = 0; j < cnt; j += n_grp * U) {
                float p[U], ds[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const chunk_entry en = ch.pick(j, u, n_grp, grp);
                    float z[NT][VEC];
                    load_head_row<VEC, NT>(z, Zk + (size_t)en.c * ldz, lpr, sub, dh, en.ok);
                    p[u] = dot_head_row<VEC, NT>(g, z);
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const chunk_entry en = ch.pick(j, u, n_grp, grp);
                    const float w = en.of(my_w);
                    float da = group_sum(p[u], lpr);
                    if constexpr (DROP) da *= en.of(my_q);
                    ds[u] = en.ok ? w * (da - Dk) : 0.f;
                    acc += ds[u];
                }
                // entry j + u n_grp + g was formed by group g at step u, every lane of the group holding the same bits: its owner
                // lane reads it from the group's first lane
                const uint32_t rel = lane - j;      // my entry's number within this turn; beyond n_grp U (or wrapped): not in it
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const float v = __shfl(ds[u], (rel & (n_grp - 1)) << lg);
                    if (rel < n_grp * U && (rel >> (6 - lg)) == (uint32_t)u) my_ds = v;
                }
            }
            if (lane < cnt) edge_axpy(eg, (size_t)base + lane, my_ds, pe);     // my row of E exists: base + lane < end
        }
        acc = fold_groups(acc, lpr);                // every lane of a group holds the group's sum: one per group is added
        if (lane == 0) {
            D[row * K + k] = Dk;
            ds_dst[row * K + k] = acc;
        }
#pragma unroll
        for (int c = 0; c < kEdgeSlots; c++) {
            if ((uint32_t)c < eg.de) {              // wave-uniform
                const float s = wave_sum(pe[c]);
                if (lane == 0) P_e[row * ldp + (size_t)k * eg.de + c] = s;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// backward over the rows of F^T: gat_backward_src_kernel (REC = false) with the edge term in x; E is in F^T's entry order
// ---------------------------------------------------------------------------
template <int VEC, int NT, int U, bool DROP>
__global__ __launch_bounds__(256) void gat_backward_src_efeat_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                                     const uint32_t *__restrict__ indices,
                                                                     const float *__restrict__ Z, size_t ldz,
                                                                     const float *__restrict__ s_dst,
                                                                     const float *__restrict__ s_src,
                                                                     const float *__restrict__ lse, const float *__restrict__ D,
                                                                     const float *__restrict__ G, size_t ldg,
                                                                     const float *__restrict__ att,
                                                                     const float *__restrict__ ds_dst, uint32_t K, uint32_t dh,
                                                                     float slope, uint32_t lg, float *__restrict__ ds_src,
                                                                     float *__restrict__ G_Z, size_t ldgz, gat_drop dp,
                                                                     gat_edge eg) {
    MGGCN_GAT_WAVE_ROW(n_rows);
    const uint32_t beg = indptr[row], end = indptr[row + 1];
    const uint32_t width = K * dh;
    for (uint32_t k = 0; k < K; k++) {
        float zr[NT][VEC], acc[NT][VEC];
        load_head_row<VEC, NT>(zr, Z + row * ldz + (size_t)k * dh, lpr, sub, dh);
        zero_head_row<VEC, NT>(acc);
        const float ss = s_src[row * K + k];
        const float *__restrict__ Gk = G + (size_t)k * dh;
        const float *__restrict__ Uk = eg.U + (size_t)k * eg.de;
        float acc_ds = 0.f;
        size_t pos = (size_t)beg + lane;
        const auto fetch = [&](uint32_t c, float *s) {          // s_dst, lse and D of the entry's destination, t of its position
            const size_t ik = (size_t)c * K + k;
            s[0] = s_dst[ik]; s[1] = lse[ik]; s[2] = D[ik];
            s[3] = edge_term(eg, Uk, pos);
        };
        entry_chunks<4> ch;
        ch.start(indices, beg, end, lane, fetch);
        for (uint32_t base = beg; base < end; base += 64) {
            pos = (size_t)base + 64 + lane;
            ch.next(indices, base, end, lane, fetch);
            const uint32_t cnt = ch.cnt;
            const float my_x = ch.my_s[0], my_l = ch.my_s[1], my_D = ch.my_s[2], my_t = ch.my_s[3];
            float my_a = 0.f, my_w = 0.f;
            [[maybe_unused]] float my_q = 0.f;
            if (lane < cnt) {
                const float x = (my_x + ss) + my_t;             // s_dst[i] + s_src[j]: the forward's sum, then the edge term
                my_a = expf(gat_lrelu(x, slope) - my_l);
                my_w = my_a * (x > 0.f ? 1.f : slope);
                if constexpr (DROP) {
                    my_q = gat_keep_scale(dp, dp.dst0 + ch.my_c, dp.src0 + (uint32_t)row, k);
                    my_a *= my_q;                   // the gather's weight alpha q; my_w keeps the plain alpha
                }
            }
            for (uint32_t j = 0; j < cnt; j += n_grp * U) {
                float gv[U][NT][VEC], p[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const chunk_entry en = ch.pick(j, u, n_grp, grp);
                    load_head_row<VEC, NT>(gv[u], Gk + (size_t)en.c * ldg, lpr, sub, dh, en.ok);
                    p[u] = dot_head_row<VEC, NT>(zr, gv[u]);
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const chunk_entry en = ch.pick(j, u, n_grp, grp);
                    const float a = en.of(my_a), w = en.of(my_w), Dv = en.of(my_D);
                    float da = group_sum(p[u], lpr);
                    if constexpr (DROP) da *= en.of(my_q);
                    acc_ds += en.ok ? w * (da - Dv) : 0.f;
                    axpy_head_row<VEC, NT>(acc, en.ok ? a : 0.f, gv[u]);
                }
            }
        }
        acc_ds = fold_groups(acc_ds, lpr);
        if (lane == 0) ds_src[row * K + k] = acc_ds;
        const float dd = ds_dst ? ds_dst[row * K + k] : 0.f;
#pragma unroll
        for (int t = 0; t < NT; t++) {
#pragma unroll
            for (int v = 0; v < VEC; v++) acc[t][v] = fold_groups(acc[t][v], lpr);
            const uint32_t col = (t * lpr + sub) * VEC;
            if (grp == 0 && col < dh) {
                float a0[VEC], a1[VEC];
                loadv<VEC>(a0, att + (size_t)k * dh + col);
                loadv<VEC>(a1, att + width + (size_t)k * dh + col);
#pragma unroll
                for (int v = 0; v < VEC; v++) acc[t][v] = fmaf(acc_ds, a1[v], fmaf(dd, a0[v], acc[t][v]));
                storev<VEC>(G_Z + row * ldgz + (size_t)k * dh + col, acc[t]);
            }
        }
    }
}

// the edge operands of an entry point, checked; has_entries: the call walks at least one entry
gat_edge make_gat_edge(const float *E, size_t lde, const float *att_edge, uint32_t de, bool has_entries) {
    MGGCN_REQUIRE(de >= 1 && de <= MGGCN_GAT_MAX_EDGE_DIM, "gat efeat supports 1 <= edge dimension <= 16");
    MGGCN_REQUIRE(lde >= de, "gat efeat: lde < edge dimension");
    MGGCN_REQUIRE(att_edge != nullptr && (!has_entries || E != nullptr), "gat efeat: null edge operand");
    return {E, att_edge, lde, de, de % 4 == 0 && rows16(E, lde)};
}

void gat_forward_efeat(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr, const uint32_t *indices,
                       const float *Z, size_t ldz, const float *s_dst, const float *s_src, uint32_t K, uint32_t dh, float slope,
                       float *out, size_t ldo, float *lse, const gat_drop *dp, const float *E, size_t lde,
                       const float *att_edge, uint32_t de) {
    require_heads(K, dh);
    MGGCN_REQUIRE(ldz >= (size_t)K * dh && ldo >= (size_t)K * dh, "gat forward: leading dimension < heads * width per head");
    const gat_edge eg = make_gat_edge(E, lde, att_edge, de, n_rows && n_cols);
    if (!n_rows) return;
    MGGCN_REQUIRE(indptr != nullptr && s_dst != nullptr && out != nullptr && lse != nullptr, "gat forward: null operand");
    MGGCN_REQUIRE(n_cols == 0 || (indices != nullptr && Z != nullptr && s_src != nullptr), "gat forward: null operand");
    MGGCN_REQUIRE((const void *)out != (const void *)Z, "gat forward: out must not alias Z");
    const bool vec = dh % 4 == 0 && rows16(Z, ldz) && rows16(out, ldo);
    const head_geometry hg = head_geometry_for(dh, vec);
    const gat_drop d = dp ? *dp : gat_drop{};
    gat_dispatch(vec, hg.nt, [&](auto v) {
        with_flag(dp != nullptr, [&](auto drop) {
            launch_rows(gat_forward_efeat_kernel<v.VEC, v.NT, v.U, drop>, n_rows, stream, n_rows, indptr, indices, Z, ldz, s_dst,
                        s_src, K, dh, slope, hg.lg, out, ldo, lse, d, eg);
        });
    });
}

void gat_backward_dst_efeat(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                            const uint32_t *indices, const float *Z, size_t ldz, const float *s_dst, const float *s_src,
                            const float *lse, const float *G, size_t ldg, const float *out, size_t ldo, uint32_t K, uint32_t dh,
                            float slope, float *D, float *ds_dst, const gat_drop *dp, const float *E, size_t lde,
                            const float *att_edge, uint32_t de, float *P_e, size_t ldp) {
    require_heads(K, dh);
    const size_t width = (size_t)K * dh;
    MGGCN_REQUIRE(ldz >= width && ldg >= width && ldo >= width, "gat backward: leading dimension < heads * width per head");
    const gat_edge eg = make_gat_edge(E, lde, att_edge, de, n_rows && n_cols);
    MGGCN_REQUIRE(ldp >= (size_t)K * de, "gat efeat backward: ldp < heads * edge dimension");
    if (!n_rows) return;
    MGGCN_REQUIRE(indptr != nullptr && s_dst != nullptr && lse != nullptr && G != nullptr && out != nullptr && D != nullptr &&
                      ds_dst != nullptr && P_e != nullptr,
                  "gat backward: null operand");
    MGGCN_REQUIRE(n_cols == 0 || (indices != nullptr && Z != nullptr && s_src != nullptr), "gat backward: null operand");
    MGGCN_REQUIRE(P_e != E && P_e != att_edge && P_e != Z && P_e != G && P_e != out,
                  "gat efeat backward: P_e must not alias an input");
    const bool vec = dh % 4 == 0 && rows16(Z, ldz) && rows16(G, ldg) && rows16(out, ldo);
    const head_geometry hg = head_geometry_for(dh, vec);
    const gat_drop d = dp ? *dp : gat_drop{};
    gat_dispatch(vec, hg.nt, [&](auto v) {
        with_flag(dp != nullptr, [&](auto drop) {
            launch_rows(gat_backward_dst_efeat_kernel<v.VEC, v.NT, v.U, drop>, n_rows, stream, n_rows, indptr, indices, Z, ldz,
                        s_dst, s_src, lse, G, ldg, out, ldo, K, dh, slope, hg.lg, D, ds_dst, d, eg, P_e, ldp);
        });
    });
}

void gat_backward_src_efeat(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                            const uint32_t *t_indices, const float *Z, size_t ldz, const float *s_dst, const float *s_src,
                            const float *lse, const float *D, const float *G, size_t ldg, const float *att, const float *ds_dst,
                            uint32_t K, uint32_t dh, float slope, float *ds_src, float *G_Z, size_t ldgz, const gat_drop *dp,
                            const float *E, size_t lde, const float *att_edge, uint32_t de) {
    require_heads(K, dh);
    const size_t width = (size_t)K * dh;
    MGGCN_REQUIRE(ldz >= width && ldg >= width && ldgz >= width, "gat backward: leading dimension < heads * width per head");
    const gat_edge eg = make_gat_edge(E, lde, att_edge, de, n_rows && n_cols);
    if (!n_rows) return;
    MGGCN_REQUIRE(t_indptr != nullptr && Z != nullptr && s_src != nullptr && att != nullptr && ds_src != nullptr &&
                      G_Z != nullptr,
                  "gat backward: null operand");
    MGGCN_REQUIRE(n_cols == 0 || (t_indices != nullptr && G != nullptr && s_dst != nullptr && lse != nullptr && D != nullptr),
                  "gat backward: null operand");
    MGGCN_REQUIRE(G_Z != G && G_Z != Z, "gat backward: G_Z must not alias G or Z");
    const bool vec = dh % 4 == 0 && rows16(Z, ldz) && rows16(G, ldg) && rows16(G_Z, ldgz) && aligned16(att);
    const head_geometry hg = head_geometry_for(dh, vec);
    const gat_drop d = dp ? *dp : gat_drop{};
    gat_dispatch(vec, hg.nt, [&](auto v) {
        with_flag(dp != nullptr, [&](auto drop) {
            launch_rows(gat_backward_src_efeat_kernel<v.VEC, v.NT, v.U, drop>, n_rows, stream, n_rows, t_indptr, t_indices, Z,
                        ldz, s_dst, s_src, lse, D, G, ldg, att, ds_dst, K, dh, slope, hg.lg, ds_src, G_Z, ldgz, d, eg);
        });
    });
}

}  // namespace

// ============================ C ABI =========================================
MGGCN_API void mggcn_gat_forward_efeat_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                           const uint32_t *indices, const float *Z, size_t ldz, const float *s_dst,
                                           const float *s_src, uint32_t K, uint32_t dh, float slope, float *out, size_t ldo,
                                           float *lse, const float *E, size_t lde, const float *att_edge, uint32_t de) {
    gat_forward_efeat(stream, n_rows, n_cols, indptr, indices, Z, ldz, s_dst, s_src, K, dh, slope, out, ldo, lse, nullptr, E, lde,
                      att_edge, de);
}

MGGCN_API void mggcn_gat_backward_dst_efeat_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                                const uint32_t *indices, const float *Z, size_t ldz, const float *s_dst,
                                                const float *s_src, const float *lse, const float *G, size_t ldg,
                                                const float *out, size_t ldo, uint32_t K, uint32_t dh, float slope, float *D,
                                                float *ds_dst, const float *E, size_t lde, const float *att_edge, uint32_t de,
                                                float *P_e, size_t ldp) {
    gat_backward_dst_efeat(stream, n_rows, n_cols, indptr, indices, Z, ldz, s_dst, s_src, lse, G, ldg, out, ldo, K, dh, slope, D,
                           ds_dst, nullptr, E, lde, att_edge, de, P_e, ldp);
}

MGGCN_API void mggcn_gat_backward_src_efeat_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols,
                                                const uint32_t *t_indptr, const uint32_t *t_indices, const float *Z, size_t ldz,
                                                const float *s_dst, const float *s_src, const float *lse, const float *D,
                                                const float *G, size_t ldg, const float *att, const float *ds_dst, uint32_t K,
                                                uint32_t dh, float slope, float *ds_src, float *G_Z, size_t ldgz, const float *E,
                                                size_t lde, const float *att_edge, uint32_t de) {
    gat_backward_src_efeat(stream, n_rows, n_cols, t_indptr, t_indices, Z, ldz, s_dst, s_src, lse, D, G, ldg, att, ds_dst, K, dh,
                           slope, ds_src, G_Z, ldgz, nullptr, E, lde, att_edge, de);
}

// The _drop twins: threshold == 0 launches the plain efeat kernels, as the _drop twins of gat.hip do; the ranges are checked.
MGGCN_API void mggcn_gat_forward_efeat_drop_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                                const uint32_t *indices, const float *Z, size_t ldz, const float *s_dst,
                                                const float *s_src, uint32_t K, uint32_t dh, float slope, float *out, size_t ldo,
                                                float *lse, uint32_t threshold, float scale, uint64_t seed,
                                                uint32_t dropout_stream, uint32_t dst0, uint32_t src0, const float *E, size_t lde,
                                                const float *att_edge, uint32_t de) {
    const gat_drop dp = make_gat_drop(threshold, scale, seed, dropout_stream, dst0, n_rows, src0, n_cols);
    gat_forward_efeat(stream, n_rows, n_cols, indptr, indices, Z, ldz, s_dst, s_src, K, dh, slope, out, ldo, lse,
                      threshold ? &dp : nullptr, E, lde, att_edge, de);
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
    gat_backward_dst_efeat(stream, n_rows, n_cols, indptr, indices, Z, ldz, s_dst, s_src, lse, G, ldg, out, ldo, K, dh, slope, D,
                           ds_dst, threshold ? &dp : nullptr, E, lde, att_edge, de, P_e, ldp);
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
    gat_backward_src_efeat(stream, n_rows, n_cols, t_indptr, t_indices, Z, ldz, s_dst, s_src, lse, D, G, ldg, att, ds_dst, K, dh,
                           slope, ds_src, G_Z, ldgz, threshold ? &dp : nullptr, E, lde, att_edge, de);
}
