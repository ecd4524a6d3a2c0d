// gat_kernels.h -- the three sparse kernels of graph attention (GAT) and the bodies of their entry points, as templates on
// the element type of the GATHERED operand: float (gat.hip, the mggcn_gat_*_f32 entry points) or uint16_t, a bf16 image of
// the fp32 tensor (gat_b16.hip, mggcn_gat_*_bf16).  gat.hip describes the layout.  The gathered operand -- the one a kernel
// indexes by an entry's column -- is Z in forward and backward_dst and G in backward_src; every operand indexed by the
// kernel's own row, the [rows x K] scalars, all arithmetic and every output are fp32 in both forms.  Only load_head_row
// (gat_internal.h) knows the element type: a bf16 instantiation is the fp32 one with 8-byte (2-byte) gathers that widen
// exactly.  Internal linkage in each translation unit that includes it.  Not part of the ABI.
// The edge term of the score (gat_edge.h) is a compile-time option of all three, EG: an empty pack in gat.hip and
// gat_b16.hip, whose kernels have neither the parameter nor a statement for it, and gat_edge in gat_efeat.hip
// (mggcn_gat_*_efeat_f32), an fp32 operand without a record.
#pragma once

#include <algorithm>
#include <cmath>
#include <type_traits>

#include "common.h"
#include "gat_edge.h"
#include "gat_internal.h"
#include "philox.h"
#include "reduce.h"

namespace {

// what a DROP kernel needs to draw the mask: threshold = floor(p 2^32), scale = fp32(1 / (1 - p)), the key (seed low, seed
// high), the dropout stream and the global indices of the call's first destination and first source
struct gat_drop {
    uint32_t threshold;
    float scale;
    uint32_t k0, k1, stream, dst0, src0;
};

// q of entry (global destination i, global source j, head k): word k & 3 of Philox(counter = (j, i, 2^31 | k >> 2, stream)).
// The set top bit of the third word keeps these counters apart from mggcn_dropout_f32's (row >> 32 there) under one
// (seed, stream).  k is wave-uniform, so the word is picked by selects on a scalar condition.
__device__ __forceinline__ float gat_keep_scale(const gat_drop &dp, uint32_t i, uint32_t j, uint32_t k) {
    const philox4 r = philox4x32_10(j, i, 0x80000000u | (k >> 2), dp.stream, dp.k0, dp.k1);
    const uint32_t word = (k & 2) ? ((k & 1) ? r.w[3] : r.w[2]) : ((k & 1) ? r.w[1] : r.w[0]);
    return word >= dp.threshold ? dp.scale : 0.f;
}

// ---------------------------------------------------------------------------
// forward: lse[i, k] and out[i, head k] = sum_j alpha_ijk Z[j, head k] over the entries j of row i
// ---------------------------------------------------------------------------
// DROP: out[i, head k] = sum_j (alpha_ijk q_ijk) Z[j, head k]; lse, the maximum and the sum are those of DROP = false
// ZT: the element type of Z, the gathered operand
// EG: gat_edge for x = (s_dst + s_src) + t, E in the entry order of the matrix walked; nothing for x = s_dst + s_src
template <int VEC, int NT, int U, bool DROP, class ZT, class... EG>
__global__ __launch_bounds__(256) void gat_forward_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                          const uint32_t *__restrict__ indices, const ZT *__restrict__ Z,
                                                          size_t ldz, const float *__restrict__ s_dst,
                                                          const float *__restrict__ s_src, uint32_t K, uint32_t dh, float slope,
                                                          uint32_t lg, float *__restrict__ out, size_t ldo,
                                                          float *__restrict__ lse, gat_drop dp, EG... eg) {
    constexpr bool EDGE = sizeof...(EG) != 0;
    MGGCN_GAT_WAVE_ROW(n_rows);
    const uint32_t beg = indptr[row], end = indptr[row + 1];
    for (uint32_t k = 0; k < K; k++) {
        const float sd = s_dst[row * K + k];
        const ZT *__restrict__ Zk = Z + (size_t)k * dh;
        // One pass over the row with a running maximum (the softmax of flash attention): per chunk, lane l owns entry l,
        // m <- max(m, the chunk's scores), the sum and the accumulators are rescaled by exp(m_old - m_new), and the chunk is
        // gathered with the weights exp(e - m).  out = acc / sum at the end: the weights of a row add up to one within
        // rounding whatever the magnitude of the scores.  The walk fetches s_src of the entry and t of its position.
        float m = -INFINITY, sum = 0.f;
        float acc[NT][VEC];
        zero_head_row<VEC, NT>(acc);
        [[maybe_unused]] size_t pos = (size_t)beg + lane;   // EDGE: the position the next fetch is for
        const auto fetch = [&](uint32_t c, float *s) {
            s[0] = s_src[(size_t)c * K + k];
            if constexpr (EDGE) s[1] = edge_term(eg..., k, pos);
        };
        entry_chunks<1 + EDGE> ch;
        ch.start(indices, beg, end, lane, fetch);
        for (uint32_t base = beg; base < end; base += 64) {
            if constexpr (EDGE) pos = (size_t)base + 64 + lane;
            ch.next(indices, base, end, lane, fetch);
            const uint32_t cnt = ch.cnt;
            float x = sd + ch.my_s[0];
            if constexpr (EDGE) x += ch.my_s[1];
            const float e = lane < cnt ? gat_lrelu(x, slope) : -INFINITY;
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
// backward over the rows of F:  D[i, k] = G[i, head k] . out[i, head k]
//   ds_dst[i, k] = sum_j alpha_ijk (G[i, head k] . Z[j, head k] - D[i, k]) lrelu'(x_ijk)
// ---------------------------------------------------------------------------
// DROP: ds_ijk = alpha_ijk (q_ijk dalpha_ijk - D[i, k]) lrelu'(x_ijk); D = G . out as before (out is the dropped forward's)
// ZT: the element type of Z, the gathered operand; G and out are the row's own
// EG: gat_edge for the edge term in x and P_e[i, k de + c] = sum_j ds_ijk E[p, c]; nothing for neither.  P_e and ldp are
// packs of the length of EG: parameters of the instantiation with the edge term, absent from the one without.
template <class>
using edge_grad_rows = float *__restrict__;
template <class>
using edge_grad_ld = size_t;
template <int VEC, int NT, int U, bool DROP, class ZT, class... EG>
__global__ __launch_bounds__(256) void gat_backward_dst_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                               const uint32_t *__restrict__ indices,
                                                               const ZT *__restrict__ Z, size_t ldz,
                                                               const float *__restrict__ s_dst, const float *__restrict__ s_src,
                                                               const float *__restrict__ lse, const float *__restrict__ G,
                                                               size_t ldg, const float *__restrict__ out, size_t ldo, uint32_t K,
                                                               uint32_t dh, float slope, uint32_t lg, float *__restrict__ D,
                                                               float *__restrict__ ds_dst, gat_drop dp, EG... eg,
                                                               edge_grad_rows<EG>... P_e, edge_grad_ld<EG>... ldp) {
    constexpr bool EDGE = sizeof...(EG) != 0;
    MGGCN_GAT_WAVE_ROW(n_rows);
    const uint32_t beg = indptr[row], end = indptr[row + 1];
    for (uint32_t k = 0; k < K; k++) {
        float g[NT][VEC];
        load_head_row<VEC, NT>(g, G + row * ldg + (size_t)k * dh, lpr, sub, dh);
        const float Dk = head_row_D<VEC, NT>(g, out + row * ldo + (size_t)k * dh, lpr, sub, grp, dh);
        const float sd = s_dst[row * K + k], ls = lse[row * K + k];
        const ZT *__restrict__ Zk = Z + (size_t)k * dh;
        float acc = 0.f;
        [[maybe_unused]] float pe[kEdgeSlots];
        if constexpr (EDGE) {
#pragma unroll
            for (int q = 0; q < kEdgeSlots; q++) pe[q] = 0.f;
        }
        [[maybe_unused]] size_t pos = (size_t)beg + lane;   // EDGE: the position the next fetch is for
        const auto fetch = [&](uint32_t c, float *s) {      // the entry's score, t of its position
            s[0] = s_src[(size_t)c * K + k];
            if constexpr (EDGE) s[1] = edge_term(eg..., k, pos);
        };
        entry_chunks<1 + EDGE> ch;
        ch.start(indices, beg, end, lane, fetch);
        for (uint32_t base = beg; base < end; base += 64) {
            if constexpr (EDGE) pos = (size_t)base + 64 + lane;
            ch.next(indices, base, end, lane, fetch);
            const uint32_t cnt = ch.cnt;
            float my_w = 0.f;                       // alpha lrelu'(x) of my entry
            [[maybe_unused]] float my_q = 0.f;
            if (lane < cnt) {
                float x = sd + ch.my_s[0];
                if constexpr (EDGE) x += ch.my_s[1];
                my_w = expf(gat_lrelu(x, slope) - ls) * (x > 0.f ? 1.f : slope);
                if constexpr (DROP) my_q = gat_keep_scale(dp, dp.dst0 + (uint32_t)row, dp.src0 + ch.my_c, k);
            }
            [[maybe_unused]] float my_ds = 0.f;     // EDGE: ds of my entry, handed back by the group that formed it
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
                if constexpr (EDGE) {
                    // entry j + u n_grp + g was formed by group g at step u, every lane of the group holding the same bits:
                    // its owner lane reads it from the group's first lane
                    const uint32_t rel = lane - j;  // my entry's number within this turn; beyond n_grp U (or wrapped): not in it
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        const float v = __shfl(ds[u], (rel & (n_grp - 1)) << lg);
                        if (rel < n_grp * U && (rel >> (6 - lg)) == (uint32_t)u) my_ds = v;
                    }
                }
            }
            if constexpr (EDGE) {                   // my row of E exists: base + lane < end
                if (lane < cnt) edge_axpy(eg..., (size_t)base + lane, my_ds, pe);
            }
        }
        acc = fold_groups(acc, lpr);                // every lane of a group holds the group's sum: one per group is added
        if (lane == 0) {
            D[row * K + k] = Dk;
            ds_dst[row * K + k] = acc;
        }
        if constexpr (EDGE) edge_store(eg..., k, lane, pe, (P_e + row * ldp)...);
    }
}

// ---------------------------------------------------------------------------
// backward over the rows of F^T (row j lists the destinations i that gather j):
//   ds_src[j, k] = sum_i alpha_ijk (G[i, head k] . Z[j, head k] - D[i, k]) lrelu'(x_ijk)
//   G_Z[j, head k] = sum_i alpha_ijk G[i, head k] + ds_dst[j, k] att[0, head k] + ds_src[j, k] att[1, head k]
// ---------------------------------------------------------------------------
// DROP: the row is the source and the entry the destination, so the counter is (row, entry) here: the words of the forward
// REC: s_dst, lse and D are not read; the three scalars of destination i and head k come from rec + (i K + k) 4
// GT: the element type of G, the gathered operand; Z is the row's own
// EG: gat_edge for the edge term in x, E in F^T's entry order (not with REC); nothing for none
template <int VEC, int NT, int U, bool DROP, bool REC, class GT, class... EG>
__global__ __launch_bounds__(256) void gat_backward_src_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                               const uint32_t *__restrict__ indices,
                                                               const float *__restrict__ Z, size_t ldz,
                                                               const float *__restrict__ s_dst, const float *__restrict__ s_src,
                                                               const float *__restrict__ lse, const float *__restrict__ D,
                                                               const float *__restrict__ rec,
                                                               const GT *__restrict__ G, size_t ldg,
                                                               const float *__restrict__ att, const float *__restrict__ ds_dst,
                                                               uint32_t K, uint32_t dh, float slope, uint32_t lg,
                                                               float *__restrict__ ds_src, float *__restrict__ G_Z, size_t ldgz,
                                                               gat_drop dp, EG... eg) {
    constexpr bool EDGE = sizeof...(EG) != 0;
    static_assert(!(REC && EDGE), "the record form has no edge term");
    MGGCN_GAT_WAVE_ROW(n_rows);
    const uint32_t beg = indptr[row], end = indptr[row + 1];
    const uint32_t width = K * dh;
    for (uint32_t k = 0; k < K; k++) {
        float zr[NT][VEC], acc[NT][VEC];
        load_head_row<VEC, NT>(zr, Z + row * ldz + (size_t)k * dh, lpr, sub, dh);
        zero_head_row<VEC, NT>(acc);
        const float ss = s_src[row * K + k];
        const GT *__restrict__ Gk = G + (size_t)k * dh;
        float acc_ds = 0.f;
        [[maybe_unused]] size_t pos = (size_t)beg + lane;       // EDGE: the position the next fetch is for
        const auto fetch = [&](uint32_t c, float *s) {          // s_dst, lse and D of the entry's destination, t of its position
            const size_t ik = (size_t)c * K + k;
            if constexpr (REC) {
                const float4 t = *reinterpret_cast<const float4 *>(rec + ik * 4);
                s[0] = t.x; s[1] = t.y; s[2] = t.z;
            } else {
                s[0] = s_dst[ik]; s[1] = lse[ik]; s[2] = D[ik];
            }
            if constexpr (EDGE) s[3] = edge_term(eg..., k, pos);
        };
        entry_chunks<3 + EDGE> ch;
        ch.start(indices, beg, end, lane, fetch);
        for (uint32_t base = beg; base < end; base += 64) {
            if constexpr (EDGE) pos = (size_t)base + 64 + lane;
            ch.next(indices, base, end, lane, fetch);
            const uint32_t cnt = ch.cnt;
            const float my_x = ch.my_s[0], my_l = ch.my_s[1], my_D = ch.my_s[2];
            float my_a = 0.f, my_w = 0.f;
            [[maybe_unused]] float my_q = 0.f;
            if (lane < cnt) {
                float x = my_x + ss;                // s_dst[i] + s_src[j]: the forward's sum, then the edge term
                if constexpr (EDGE) x += ch.my_s[3];
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

// the mask's operands of a _drop entry point; both index ranges of the call must fit the 32-bit counter words
gat_drop make_gat_drop(uint32_t threshold, float scale, uint64_t seed, uint32_t dropout_stream, uint32_t dst0, uint32_t n_dst,
                       uint32_t src0, uint32_t n_src) {
    MGGCN_REQUIRE((uint64_t)dst0 + n_dst <= 0x100000000ull && (uint64_t)src0 + n_src <= 0x100000000ull,
                  "gat dropout: dst0 + destinations and src0 + sources must not exceed 2^32");
    return {threshold, scale, (uint32_t)seed, (uint32_t)(seed >> 32), dropout_stream, dst0, src0};
}

// The bodies of the plain entry points and of their _drop twins: dp == nullptr launches the DROP = false kernels.  The
// float4 path needs every dense operand's rows aligned for four columns -- 16 bytes of fp32, 8 bytes of a bf16 image
// (rows16) --, so a call on an image runs the (VEC, NT, U) the fp32 call runs on the widened operand, equally aligned in elements.
// eg: nothing, or the call's gat_edge (gat_efeat.hip's make_gat_edge), which launches the kernels with the edge term.
template <class T>
const T &only(const T &v) { return v; }         // the element of a pack of one

template <class ZT, class... EG>
void gat_forward(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr, const uint32_t *indices,
                 const ZT *Z, size_t ldz, const float *s_dst, const float *s_src, uint32_t K, uint32_t dh, float slope,
                 float *out, size_t ldo, float *lse, const gat_drop *dp, const EG &...eg) {
    require_heads(K, dh);
    MGGCN_REQUIRE(ldz >= (size_t)K * dh && ldo >= (size_t)K * dh, "gat forward: leading dimension < heads * width per head");
    if (!n_rows) return;
    MGGCN_REQUIRE(indptr != nullptr && s_dst != nullptr && out != nullptr && lse != nullptr, "gat forward: null operand");
    MGGCN_REQUIRE(n_cols == 0 || (indices != nullptr && Z != nullptr && s_src != nullptr), "gat forward: null operand");
    MGGCN_REQUIRE((const void *)out != (const void *)Z, "gat forward: out must not alias Z");
    const bool vec = dh % 4 == 0 && rows16(Z, ldz) && rows16(out, ldo);
    const head_geometry hg = head_geometry_for(dh, vec);
    const gat_drop d = dp ? *dp : gat_drop{};
    gat_dispatch(vec, hg.nt, [&](auto v) {
        with_flag(dp != nullptr, [&](auto drop) {
            launch_rows(gat_forward_kernel<v.VEC, v.NT, v.U, drop, ZT, EG...>, n_rows, stream, n_rows, indptr, indices, Z, ldz,
                        s_dst, s_src, K, dh, slope, hg.lg, out, ldo, lse, d, eg...);
        });
    });
}

// P_e [n_rows x ldp]: with eg only
template <class ZT, class... EG>
void gat_backward_dst(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr, const uint32_t *indices,
                      const ZT *Z, size_t ldz, const float *s_dst, const float *s_src, const float *lse, const float *G,
                      size_t ldg, const float *out, size_t ldo, uint32_t K, uint32_t dh, float slope, float *D, float *ds_dst,
                      const gat_drop *dp, float *P_e = nullptr, size_t ldp = 0, const EG &...eg) {
    constexpr bool EDGE = sizeof...(EG) != 0;
    require_heads(K, dh);
    const size_t width = (size_t)K * dh;
    MGGCN_REQUIRE(ldz >= width && ldg >= width && ldo >= width, "gat backward: leading dimension < heads * width per head");
    if constexpr (EDGE) MGGCN_REQUIRE(ldp >= (size_t)K * only(eg...).de, "gat efeat backward: ldp < heads * edge dimension");
    if (!n_rows) return;
    MGGCN_REQUIRE(indptr != nullptr && s_dst != nullptr && lse != nullptr && G != nullptr && out != nullptr && D != nullptr &&
                      ds_dst != nullptr && (!EDGE || P_e != nullptr),
                  "gat backward: null operand");
    MGGCN_REQUIRE(n_cols == 0 || (indices != nullptr && Z != nullptr && s_src != nullptr), "gat backward: null operand");
    if constexpr (EDGE)
        MGGCN_REQUIRE(P_e != only(eg...).E && P_e != only(eg...).U && P_e != Z && P_e != G && P_e != out,
                      "gat efeat backward: P_e must not alias an input");
    const bool vec = dh % 4 == 0 && rows16(Z, ldz) && rows16(G, ldg) && rows16(out, ldo);
    const head_geometry hg = head_geometry_for(dh, vec);
    const gat_drop d = dp ? *dp : gat_drop{};
    gat_dispatch(vec, hg.nt, [&](auto v) {
        with_flag(dp != nullptr, [&](auto drop) {
            const auto launch = [&](auto... edge) {
                launch_rows(gat_backward_dst_kernel<v.VEC, v.NT, v.U, drop, ZT, EG...>, n_rows, stream, n_rows, indptr, indices,
                            Z, ldz, s_dst, s_src, lse, G, ldg, out, ldo, K, dh, slope, hg.lg, D, ds_dst, d, edge...);
            };
            if constexpr (EDGE) launch(eg..., P_e, ldp);
            else launch();
        });
    });
}

// rec != nullptr launches the REC = true kernels, which read it in place of s_dst, lse and D (all three nullptr then); the
// record form exists on an fp32 G only, and without an edge term
template <class GT, class... EG>
void gat_backward_src(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                      const uint32_t *t_indices, const float *Z, size_t ldz, const float *s_dst, const float *s_src,
                      const float *lse, const float *D, const float *rec, const GT *G, size_t ldg, const float *att,
                      const float *ds_dst, uint32_t K, uint32_t dh, float slope, float *ds_src, float *G_Z, size_t ldgz,
                      const gat_drop *dp, const EG &...eg) {
    constexpr bool has_rec = std::is_same_v<GT, float> && sizeof...(EG) == 0;
    require_heads(K, dh);
    const size_t width = (size_t)K * dh;
    MGGCN_REQUIRE(ldz >= width && ldg >= width && ldgz >= width, "gat backward: leading dimension < heads * width per head");
    if (!n_rows) return;
    MGGCN_REQUIRE(has_rec || rec == nullptr, "gat backward: the record form takes an fp32 G");
    MGGCN_REQUIRE(t_indptr != nullptr && Z != nullptr && s_src != nullptr && att != nullptr && ds_src != nullptr &&
                      G_Z != nullptr,
                  "gat backward: null operand");
    MGGCN_REQUIRE(n_cols == 0 || (t_indices != nullptr && G != nullptr &&
                                  (rec != nullptr || (s_dst != nullptr && lse != nullptr && D != nullptr))),
                  "gat backward: null operand");
    MGGCN_REQUIRE((const void *)G_Z != (const void *)G && G_Z != Z, "gat backward: G_Z must not alias G or Z");
    const bool vec = dh % 4 == 0 && rows16(Z, ldz) && rows16(G, ldg) && rows16(G_Z, ldgz) && aligned16(att);
    const head_geometry hg = head_geometry_for(dh, vec);
    const gat_drop d = dp ? *dp : gat_drop{};
    gat_dispatch(vec, hg.nt, [&](auto v) {
        with_flag(dp != nullptr, [&](auto drop) {
            const auto launch = [&](auto packed) {
                launch_rows(gat_backward_src_kernel<v.VEC, v.NT, v.U, drop, packed, GT, EG...>, n_rows, stream, n_rows, t_indptr,
                            t_indices, Z, ldz, s_dst, s_src, lse, D, rec, G, ldg, att, ds_dst, K, dh, slope, hg.lg, ds_src, G_Z,
                            ldgz, d, eg...);
            };
            if constexpr (has_rec) with_flag(rec != nullptr, launch);
            else launch(std::false_type{});
        });
    });
}

}  // namespace
