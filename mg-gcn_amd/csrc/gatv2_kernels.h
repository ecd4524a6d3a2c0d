// gatv2_kernels.h -- the three sparse kernels of GATv2 and the bodies of their entry points, as templates on the element
// type of the GATHERED operands: float (gatv2.hip, mggcn_gatv2_*_f32) or uint16_t, a bf16 image of the fp32 tensor
// (gatv2_b16.hip, mggcn_gatv2_*_bf16).  gatv2.hip describes the layout.  Gathered -- indexed by an entry's column -- are Zs
// in forward and backward_dst, Zd and G in backward_src; the row's own operands, att, lse, D, all arithmetic and every
// output are fp32 in both forms.  Only load_head_row (gat_internal.h) knows the element type.  Internal linkage in each
// translation unit that includes it.  Not part of the ABI.
#pragma once

#include <algorithm>
#include <cmath>
#include <type_traits>

#include "common.h"
#include "gat_internal.h"
#include "reduce.h"

namespace {

// this lane's part of e = sum_c a[c] lrelu(zd[c] + z[c]) (columns beyond dh hold zeros in all three)
template <int VEC, int NT>
__device__ __forceinline__ float score_head_row(const float (&a)[NT][VEC], const float (&zd)[NT][VEC],
                                                const float (&z)[NT][VEC], float slope) {
    float p = 0.f;
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int v = 0; v < VEC; v++) p = fmaf(a[t][v], gat_lrelu(zd[t][v] + z[t][v], slope), p);
    return p;
}

// ---------------------------------------------------------------------------
// forward: lse[i, k] and out[i, head k] = sum_j alpha_ijk Zs[j, head k] over the entries j of row i
// ---------------------------------------------------------------------------
// ZT: the element type of Zs, the gathered operand; Zd is the row's own
template <int VEC, int NT, int U, class ZT>
__global__ __launch_bounds__(256) void gatv2_forward_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                            const uint32_t *__restrict__ indices,
                                                            const ZT *__restrict__ Zs, size_t ldzs,
                                                            const float *__restrict__ Zd, size_t ldzd,
                                                            const float *__restrict__ att, uint32_t K, uint32_t dh,
                                                            float slope, uint32_t lg, float *__restrict__ out, size_t ldo,
                                                            float *__restrict__ lse) {
    MGGCN_GAT_WAVE_ROW(n_rows);
    const uint32_t beg = indptr[row], end = indptr[row + 1];
    for (uint32_t k = 0; k < K; k++) {
        float zd[NT][VEC], a[NT][VEC];
        load_head_row<VEC, NT>(zd, Zd + row * ldzd + (size_t)k * dh, lpr, sub, dh);
        load_head_row<VEC, NT>(a, att + (size_t)k * dh, lpr, sub, dh);
        const ZT *__restrict__ Zk = Zs + (size_t)k * dh;
        using sm = group_softmax<VEC, NT, U>;
        float m, sum, acc[NT][VEC];
        sm::start(m, sum, acc);
        entry_chunks<0> ch;                         // the indices alone
        ch.start(indices, beg, end, lane, no_scalars);
        for (uint32_t base = beg; base < end; base += 64) {
            ch.next(indices, base, end, lane, no_scalars);
            const uint32_t cnt = ch.cnt;
            for (uint32_t j = 0; j < cnt; j += n_grp * U) {
                float z[U][NT][VEC], e[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const chunk_entry en = ch.pick(j, u, n_grp, grp);
                    load_head_row<VEC, NT>(z[u], Zk + (size_t)en.c * ldzs, lpr, sub, dh, en.ok);
                    e[u] = score_head_row<VEC, NT>(a, zd, z[u], slope);
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
                    e[u] = group_sum(e[u], lpr);
                    if (!ch.pick(j, u, n_grp, grp).ok) e[u] = -INFINITY;
                }
                sm::add(m, sum, acc, e, z);
            }
        }
        sm::finish(m, sum, acc, out + row * ldo + (size_t)k * dh, lse + row * K + k, beg < end, lane, lpr, sub, grp, dh);
    }
}

// ---------------------------------------------------------------------------
// backward over the rows of F:  D[i, k] = G[i, head k] . out[i, head k],  ds_ijk = alpha_ijk (G[i, head k] . Zs[j, head k] - D[i, k])
//   G_Zd[i, k dh + c] = att[k dh + c] sum_j ds_ijk lrelu'(t_ijk[c]),  P[i, k dh + c] = sum_j ds_ijk lrelu(t_ijk[c])
// ---------------------------------------------------------------------------
// ZT: the element type of Zs, the gathered operand; Zd, G and out are the row's own
template <int VEC, int NT, int U, class ZT>
__global__ __launch_bounds__(256) void gatv2_backward_dst_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                                 const uint32_t *__restrict__ indices,
                                                                 const ZT *__restrict__ Zs, size_t ldzs,
                                                                 const float *__restrict__ Zd, size_t ldzd,
                                                                 const float *__restrict__ att, const float *__restrict__ lse,
                                                                 const float *__restrict__ G, size_t ldg,
                                                                 const float *__restrict__ out, size_t ldo, uint32_t K,
                                                                 uint32_t dh, float slope, uint32_t lg, float *__restrict__ D,
                                                                 float *__restrict__ G_Zd, size_t ldgzd, float *__restrict__ P,
                                                                 size_t ldp) {
    MGGCN_GAT_WAVE_ROW(n_rows);
    const uint32_t beg = indptr[row], end = indptr[row + 1];
    for (uint32_t k = 0; k < K; k++) {
        float g[NT][VEC], zd[NT][VEC], a[NT][VEC], accv[NT][VEC], accp[NT][VEC];
        load_head_row<VEC, NT>(g, G + row * ldg + (size_t)k * dh, lpr, sub, dh);
        const float Dk = head_row_D<VEC, NT>(g, out + row * ldo + (size_t)k * dh, lpr, sub, grp, dh);
        load_head_row<VEC, NT>(zd, Zd + row * ldzd + (size_t)k * dh, lpr, sub, dh);
        load_head_row<VEC, NT>(a, att + (size_t)k * dh, lpr, sub, dh);
        zero_head_row<VEC, NT>(accv);
        zero_head_row<VEC, NT>(accp);
        const float ls = lse[row * K + k];
        const ZT *__restrict__ Zk = Zs + (size_t)k * dh;
        entry_chunks<0> ch;                         // the indices alone
        ch.start(indices, beg, end, lane, no_scalars);
        for (uint32_t base = beg; base < end; base += 64) {
            ch.next(indices, base, end, lane, no_scalars);
            const uint32_t cnt = ch.cnt;
            for (uint32_t j = 0; j < cnt; j += n_grp * U) {
                float z[U][NT][VEC], pe[U], pd[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const chunk_entry en = ch.pick(j, u, n_grp, grp);
                    load_head_row<VEC, NT>(z[u], Zk + (size_t)en.c * ldzs, lpr, sub, dh, en.ok);
                    pe[u] = score_head_row<VEC, NT>(a, zd, z[u], slope);
                    pd[u] = dot_head_row<VEC, NT>(g, z[u]);
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const float e = group_sum(pe[u], lpr), da = group_sum(pd[u], lpr);
                    const float ds = ch.pick(j, u, n_grp, grp).ok ? expf(e - ls) * (da - Dk) : 0.f;
                    const float dss = ds * slope;
#pragma unroll
                    for (int t = 0; t < NT; t++)
#pragma unroll
                        for (int v = 0; v < VEC; v++) {
                            const float tt = zd[t][v] + z[u][t][v];
                            accv[t][v] += tt > 0.f ? ds : dss;
                            accp[t][v] = fmaf(ds, gat_lrelu(tt, slope), accp[t][v]);
                        }
                }
            }
        }
        if (lane == 0) D[row * K + k] = Dk;
        // the product rounded once, as x * att is, but + 0.0 on top: a row without entries (x = +0.0) gets +0.0 under a
        // negative att too, where the bare product is -0.0
        fold_store_head_row<VEC, NT>(G_Zd + row * ldgzd + (size_t)k * dh, accv, lpr, sub, grp, dh,
                                     [&](int t, int v, float x) { return fmaf(x, a[t][v], 0.f); });
        fold_store_head_row<VEC, NT>(P + row * ldp + (size_t)k * dh, accp, lpr, sub, grp, dh);
    }
}

// ---------------------------------------------------------------------------
// backward over the rows of F^T (row j lists the destinations i that gather j):
//   G_Zs[j, k dh + c] = sum_i (alpha_ijk G[i, k dh + c] + ds_ijk att[k dh + c] lrelu'(t_ijk[c]))
// ---------------------------------------------------------------------------
// REC: lse and D are not read; the two scalars of destination i and head k come from rec + (i K + k) 2
// GT: the element type of Zd and G, the gathered operands; Zs is the row's own
template <int VEC, int NT, int U, bool REC, class GT>
__global__ __launch_bounds__(256) void gatv2_backward_src_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                                 const uint32_t *__restrict__ indices,
                                                                 const float *__restrict__ Zs, size_t ldzs,
                                                                 const GT *__restrict__ Zd, size_t ldzd,
                                                                 const float *__restrict__ att, const float *__restrict__ lse,
                                                                 const float *__restrict__ D, const float *__restrict__ rec,
                                                                 const GT *__restrict__ G, size_t ldg, uint32_t K,
                                                                 uint32_t dh, float slope, uint32_t lg,
                                                                 float *__restrict__ G_Zs, size_t ldgzs) {
    MGGCN_GAT_WAVE_ROW(n_rows);
    const uint32_t beg = indptr[row], end = indptr[row + 1];
    for (uint32_t k = 0; k < K; k++) {
        float zs[NT][VEC], a[NT][VEC], acc[NT][VEC];
        load_head_row<VEC, NT>(zs, Zs + row * ldzs + (size_t)k * dh, lpr, sub, dh);
        load_head_row<VEC, NT>(a, att + (size_t)k * dh, lpr, sub, dh);
        zero_head_row<VEC, NT>(acc);
        const GT *__restrict__ Zdk = Zd + (size_t)k * dh;
        const GT *__restrict__ Gk = G + (size_t)k * dh;
        const fetch_lse_D<REC> fetch{lse, D, rec, K, k};        // lse and D of the entry's destination
        entry_chunks<2> ch;
        ch.start(indices, beg, end, lane, fetch);
        for (uint32_t base = beg; base < end; base += 64) {
            ch.next(indices, base, end, lane, fetch);
            const uint32_t cnt = ch.cnt;
            const float my_l = ch.my_s[0], my_D = ch.my_s[1];
            for (uint32_t j = 0; j < cnt; j += n_grp * U) {
                float zv[U][NT][VEC], gv[U][NT][VEC], pe[U], pd[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const chunk_entry en = ch.pick(j, u, n_grp, grp);
                    load_head_row<VEC, NT>(zv[u], Zdk + (size_t)en.c * ldzd, lpr, sub, dh, en.ok);
                    load_head_row<VEC, NT>(gv[u], Gk + (size_t)en.c * ldg, lpr, sub, dh, en.ok);
                    pe[u] = score_head_row<VEC, NT>(a, zv[u], zs, slope);
                    pd[u] = dot_head_row<VEC, NT>(zs, gv[u]);
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const chunk_entry en = ch.pick(j, u, n_grp, grp);
                    const float l = en.of(my_l), Dv = en.of(my_D);
                    const float e = group_sum(pe[u], lpr), da = group_sum(pd[u], lpr);
                    const float al = en.ok ? expf(e - l) : 0.f;
                    const float ds = al * (da - Dv), dss = ds * slope;
#pragma unroll
                    for (int t = 0; t < NT; t++)
#pragma unroll
                        for (int v = 0; v < VEC; v++) {
                            const float tt = zv[u][t][v] + zs[t][v];
                            acc[t][v] = fmaf(al, gv[u][t][v], acc[t][v]);
                            acc[t][v] = fmaf(tt > 0.f ? ds : dss, a[t][v], acc[t][v]);
                        }
                }
            }
        }
        fold_store_head_row<VEC, NT>(G_Zs + row * ldgzs + (size_t)k * dh, acc, lpr, sub, grp, dh);
    }
}

// The bodies of the entry points.  The float4 path needs every dense operand's rows aligned for four columns -- 16 bytes
// of fp32, 8 bytes of a bf16 image (rows16) --, so a call on an image runs the (VEC, NT, U) the fp32 call runs on the
// widened operand, equally aligned in elements.
template <class ZT>
void gatv2_forward(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr, const uint32_t *indices,
                   const ZT *Zs, size_t ldzs, const float *Zd, size_t ldzd, const float *att, uint32_t K, uint32_t dh,
                   float slope, float *out, size_t ldo, float *lse) {
    require_heads(K, dh);
    const size_t width = (size_t)K * dh;
    MGGCN_REQUIRE(ldzs >= width && ldzd >= width && ldo >= width, "gatv2 forward: leading dimension < heads * width per head");
    if (!n_rows) return;
    MGGCN_REQUIRE(indptr != nullptr && Zd != nullptr && att != nullptr && out != nullptr && lse != nullptr,
                  "gatv2 forward: null operand");
    MGGCN_REQUIRE(n_cols == 0 || (indices != nullptr && Zs != nullptr), "gatv2 forward: null operand");
    MGGCN_REQUIRE((const void *)out != (const void *)Zs && out != Zd, "gatv2 forward: out must not alias Zs or Zd");
    const bool vec = dh % 4 == 0 && rows16(Zs, ldzs) && rows16(Zd, ldzd) && rows16(out, ldo) && aligned16(att);
    const head_geometry hg = head_geometry_for(dh, vec);
    gat_dispatch(vec, hg.nt, [&](auto v) {
        launch_rows(gatv2_forward_kernel<v.VEC, v.NT, v.U, ZT>, n_rows, stream, n_rows, indptr, indices, Zs, ldzs, Zd, ldzd, att, K,
                    dh, slope, hg.lg, out, ldo, lse);
    });
}

template <class ZT>
void gatv2_backward_dst(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                        const uint32_t *indices, const ZT *Zs, size_t ldzs, const float *Zd, size_t ldzd, const float *att,
                        const float *lse, const float *G, size_t ldg, const float *out, size_t ldo, uint32_t K, uint32_t dh,
                        float slope, float *D, float *G_Zd, size_t ldgzd, float *P, size_t ldp) {
    require_heads(K, dh);
    const size_t width = (size_t)K * dh;
    MGGCN_REQUIRE(ldzs >= width && ldzd >= width && ldg >= width && ldo >= width && ldgzd >= width && ldp >= width,
                  "gatv2 backward: leading dimension < heads * width per head");
    if (!n_rows) return;
    MGGCN_REQUIRE(indptr != nullptr && Zd != nullptr && att != nullptr && lse != nullptr && G != nullptr && out != nullptr &&
                      D != nullptr && G_Zd != nullptr && P != nullptr,
                  "gatv2 backward: null operand");
    MGGCN_REQUIRE(n_cols == 0 || (indices != nullptr && Zs != nullptr), "gatv2 backward: null operand");
    const void *zs = Zs;
    MGGCN_REQUIRE(G_Zd != G && G_Zd != zs && G_Zd != Zd && G_Zd != out && P != G && P != zs && P != Zd && P != out && P != G_Zd,
                  "gatv2 backward: G_Zd and P must not alias an input or each other");
    const bool vec = dh % 4 == 0 && rows16(Zs, ldzs) && rows16(Zd, ldzd) && rows16(G, ldg) && rows16(out, ldo) &&
                     rows16(G_Zd, ldgzd) && rows16(P, ldp) && aligned16(att);
    const head_geometry hg = head_geometry_for(dh, vec);
    gat_dispatch(vec, hg.nt, [&](auto v) {
        launch_rows(gatv2_backward_dst_kernel<v.VEC, v.NT, v.U, ZT>, n_rows, stream, n_rows, indptr, indices, Zs, ldzs, Zd, ldzd,
                    att, lse, G, ldg, out, ldo, K, dh, slope, hg.lg, D, G_Zd, ldgzd, P, ldp);
    });
}

// The body of backward_src and of its record form: rec != nullptr launches the REC = true kernels, which read it in place of
// lse and D (both nullptr then); the record form exists on fp32 gathered operands only
template <class GT>
void gatv2_backward_src(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                        const uint32_t *t_indices, const float *Zs, size_t ldzs, const GT *Zd, size_t ldzd, const float *att,
                        const float *lse, const float *D, const float *rec, const GT *G, size_t ldg, uint32_t K, uint32_t dh,
                        float slope, float *G_Zs, size_t ldgzs) {
    constexpr bool has_rec = std::is_same_v<GT, float>;
    require_heads(K, dh);
    const size_t width = (size_t)K * dh;
    MGGCN_REQUIRE(ldzs >= width && ldzd >= width && ldg >= width && ldgzs >= width,
                  "gatv2 backward: leading dimension < heads * width per head");
    if (!n_rows) return;
    MGGCN_REQUIRE(has_rec || rec == nullptr, "gatv2 backward: the record form takes fp32 operands");
    MGGCN_REQUIRE(t_indptr != nullptr && Zs != nullptr && att != nullptr && G_Zs != nullptr, "gatv2 backward: null operand");
    MGGCN_REQUIRE(n_cols == 0 || (t_indices != nullptr && Zd != nullptr && G != nullptr &&
                                  (rec != nullptr || (lse != nullptr && D != nullptr))),
                  "gatv2 backward: null operand");
    MGGCN_REQUIRE((const void *)G_Zs != (const void *)G && G_Zs != Zs && (const void *)G_Zs != (const void *)Zd,
                  "gatv2 backward: G_Zs must not alias G, Zs or Zd");
    const bool vec = dh % 4 == 0 && rows16(Zs, ldzs) && rows16(Zd, ldzd) && rows16(G, ldg) && rows16(G_Zs, ldgzs) && aligned16(att);
    const head_geometry hg = head_geometry_for(dh, vec);
    gat_dispatch(vec, hg.nt, [&](auto v) {
        const auto launch = [&](auto packed) {
            launch_rows(gatv2_backward_src_kernel<v.VEC, v.NT, v.U, packed, GT>, n_rows, stream, n_rows, t_indptr, t_indices, Zs,
                        ldzs, Zd, ldzd, att, lse, D, rec, G, ldg, K, dh, slope, hg.lg, G_Zs, ldgzs);
        };
        if constexpr (has_rec) with_flag(rec != nullptr, launch);
        else launch(std::false_type{});
    });
}

}  // namespace
