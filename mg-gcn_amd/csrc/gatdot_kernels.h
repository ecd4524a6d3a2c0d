// gatdot_kernels.h -- the three sparse kernels of dot-product attention and the bodies of their entry points, as templates
// on the element type of the GATHERED operands: float (gatdot.hip, mggcn_gatdot_*_f32) or uint16_t, a bf16 image of the fp32
// tensor (gatdot_b16.hip, mggcn_gatdot_*_bf16).  gatdot.hip describes the layout.  Gathered -- indexed by an entry's column --
// are Zk and Zv in forward and backward_dst, Zq and G in backward_src; the row's own operands, lse, D, all arithmetic and
// every output are fp32 in both forms.  Only load_head_row (gat_internal.h) knows the element type.  Internal linkage in
// each translation unit that includes it.  Not part of the ABI.
#pragma once

#include <algorithm>
#include <cmath>
#include <type_traits>

#include "common.h"
#include "gat_internal.h"
#include "reduce.h"

namespace {

// ---------------------------------------------------------------------------
// forward: lse[i, k] and out[i, head k] = sum_j alpha_ijk Zv[j, head k] over the entries j of row i
// ---------------------------------------------------------------------------
// GT: the element type of Zk and Zv, the gathered operands; Zq is the row's own
template <int VEC, int NT, int U, class GT>
__global__ __launch_bounds__(256) void gatdot_forward_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                             const uint32_t *__restrict__ indices,
                                                             const float *__restrict__ Zq, size_t ldq,
                                                             const GT *__restrict__ Zk, size_t ldk,
                                                             const GT *__restrict__ Zv, size_t ldv, uint32_t K, uint32_t dh,
                                                             float c, uint32_t lg, float *__restrict__ out, size_t ldo,
                                                             float *__restrict__ lse) {
    MGGCN_GAT_WAVE_ROW(n_rows);
    const uint32_t beg = indptr[row], end = indptr[row + 1];
    for (uint32_t k = 0; k < K; k++) {
        float q[NT][VEC];
        load_head_row<VEC, NT>(q, Zq + row * ldq + (size_t)k * dh, lpr, sub, dh);
        const GT *__restrict__ Kk = Zk + (size_t)k * dh;
        const GT *__restrict__ Vk = Zv + (size_t)k * dh;
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
                for (int u = 0; u < U; u++) {       // both gathers of every unrolled entry, then the scores
                    const chunk_entry en = ch.pick(j, u, n_grp, grp);
                    float kk[NT][VEC];
                    load_head_row<VEC, NT>(kk, Kk + (size_t)en.c * ldk, lpr, sub, dh, en.ok);
                    load_head_row<VEC, NT>(z[u], Vk + (size_t)en.c * ldv, lpr, sub, dh, en.ok);
                    e[u] = dot_head_row<VEC, NT>(q, kk);
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
                    e[u] = c * group_sum(e[u], lpr);
                    if (!ch.pick(j, u, n_grp, grp).ok) e[u] = -INFINITY;
                }
                sm::add(m, sum, acc, e, z);
            }
        }
        sm::finish(m, sum, acc, out + row * ldo + (size_t)k * dh, lse + row * K + k, beg < end, lane, lpr, sub, grp, dh);
    }
}

// ---------------------------------------------------------------------------
// backward over the rows of F:  D[i, k] = G[i, head k] . out[i, head k],  ds_ijk = alpha_ijk (G[i, head k] . Zv[j, head k] - D[i, k]),
//   G_Zq[i, head k] = c sum_j ds_ijk Zk[j, head k]
// ---------------------------------------------------------------------------
// GT: the element type of Zk and Zv, the gathered operands; Zq, G and out are the row's own
template <int VEC, int NT, int U, class GT>
__global__ __launch_bounds__(256) void gatdot_backward_dst_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                                  const uint32_t *__restrict__ indices,
                                                                  const float *__restrict__ Zq, size_t ldq,
                                                                  const GT *__restrict__ Zk, size_t ldk,
                                                                  const GT *__restrict__ Zv, size_t ldv,
                                                                  const float *__restrict__ lse, const float *__restrict__ G,
                                                                  size_t ldg, const float *__restrict__ out, size_t ldo,
                                                                  uint32_t K, uint32_t dh, float c, uint32_t lg,
                                                                  float *__restrict__ D, float *__restrict__ G_Zq, size_t ldgzq) {
    MGGCN_GAT_WAVE_ROW(n_rows);
    const uint32_t beg = indptr[row], end = indptr[row + 1];
    for (uint32_t k = 0; k < K; k++) {
        float g[NT][VEC], q[NT][VEC], accq[NT][VEC];
        load_head_row<VEC, NT>(g, G + row * ldg + (size_t)k * dh, lpr, sub, dh);
        const float Dk = head_row_D<VEC, NT>(g, out + row * ldo + (size_t)k * dh, lpr, sub, grp, dh);
        load_head_row<VEC, NT>(q, Zq + row * ldq + (size_t)k * dh, lpr, sub, dh);
        zero_head_row<VEC, NT>(accq);
        const float ls = lse[row * K + k];
        const GT *__restrict__ Kk = Zk + (size_t)k * dh;
        const GT *__restrict__ Vk = Zv + (size_t)k * dh;
        entry_chunks<0> ch;                         // the indices alone
        ch.start(indices, beg, end, lane, no_scalars);
        for (uint32_t base = beg; base < end; base += 64) {
            ch.next(indices, base, end, lane, no_scalars);
            const uint32_t cnt = ch.cnt;
            for (uint32_t j = 0; j < cnt; j += n_grp * U) {
                float kk[U][NT][VEC], pe[U], pd[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const chunk_entry en = ch.pick(j, u, n_grp, grp);
                    float z[NT][VEC];
                    load_head_row<VEC, NT>(kk[u], Kk + (size_t)en.c * ldk, lpr, sub, dh, en.ok);
                    load_head_row<VEC, NT>(z, Vk + (size_t)en.c * ldv, lpr, sub, dh, en.ok);
                    pe[u] = dot_head_row<VEC, NT>(q, kk[u]);
                    pd[u] = dot_head_row<VEC, NT>(g, z);
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const float e = c * group_sum(pe[u], lpr), da = group_sum(pd[u], lpr);
                    const float ds = ch.pick(j, u, n_grp, grp).ok ? expf(e - ls) * (da - Dk) : 0.f;
                    axpy_head_row<VEC, NT>(accq, ds, kk[u]);
                }
            }
        }
        if (lane == 0) D[row * K + k] = Dk;
        // the product rounded once, + 0.0 on top: a row without entries (x = +0.0) gets +0.0 whatever the sign of c
        fold_store_head_row<VEC, NT>(G_Zq + row * ldgzq + (size_t)k * dh, accq, lpr, sub, grp, dh,
                                     [&](int, int, float x) { return fmaf(x, c, 0.f); });
    }
}

// ---------------------------------------------------------------------------
// backward over the rows of F^T (row j lists the destinations i that gather j):
//   G_Zk[j, head k] = c sum_i ds_ijk Zq[i, head k],   G_Zv[j, head k] = sum_i alpha_ijk G[i, head k]
// ---------------------------------------------------------------------------
// GT: the element type of Zq and G, the gathered operands; Zk and Zv are the row's own
template <int VEC, int NT, int U, class GT>
__global__ __launch_bounds__(256) void gatdot_backward_src_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                                  const uint32_t *__restrict__ indices,
                                                                  const GT *__restrict__ Zq, size_t ldq,
                                                                  const float *__restrict__ Zk, size_t ldk,
                                                                  const float *__restrict__ Zv, size_t ldv,
                                                                  const float *__restrict__ lse, const float *__restrict__ D,
                                                                  const GT *__restrict__ G, size_t ldg, uint32_t K,
                                                                  uint32_t dh, float c, uint32_t lg, float *__restrict__ G_Zk,
                                                                  size_t ldgzk, float *__restrict__ G_Zv, size_t ldgzv) {
    MGGCN_GAT_WAVE_ROW(n_rows);
    const uint32_t beg = indptr[row], end = indptr[row + 1];
    for (uint32_t k = 0; k < K; k++) {
        float zk[NT][VEC], zv[NT][VEC], acck[NT][VEC], accv[NT][VEC];
        load_head_row<VEC, NT>(zk, Zk + row * ldk + (size_t)k * dh, lpr, sub, dh);
        load_head_row<VEC, NT>(zv, Zv + row * ldv + (size_t)k * dh, lpr, sub, dh);
        zero_head_row<VEC, NT>(acck);
        zero_head_row<VEC, NT>(accv);
        const GT *__restrict__ Qk = Zq + (size_t)k * dh;
        const GT *__restrict__ Gk = G + (size_t)k * dh;
        const fetch_lse_D<false> fetch{lse, D, nullptr, K, k};  // lse and D of the entry's destination: no record form
        entry_chunks<2> ch;
        ch.start(indices, beg, end, lane, fetch);
        for (uint32_t base = beg; base < end; base += 64) {
            ch.next(indices, base, end, lane, fetch);
            const uint32_t cnt = ch.cnt;
            const float my_l = ch.my_s[0], my_D = ch.my_s[1];
            for (uint32_t j = 0; j < cnt; j += n_grp * U) {
                float qv[U][NT][VEC], gv[U][NT][VEC], pe[U], pd[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const chunk_entry en = ch.pick(j, u, n_grp, grp);
                    load_head_row<VEC, NT>(qv[u], Qk + (size_t)en.c * ldq, lpr, sub, dh, en.ok);
                    load_head_row<VEC, NT>(gv[u], Gk + (size_t)en.c * ldg, lpr, sub, dh, en.ok);
                    pe[u] = dot_head_row<VEC, NT>(qv[u], zk);
                    pd[u] = dot_head_row<VEC, NT>(gv[u], zv);
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const chunk_entry en = ch.pick(j, u, n_grp, grp);
                    const float l = en.of(my_l), Dv = en.of(my_D);
                    const float e = c * group_sum(pe[u], lpr), da = group_sum(pd[u], lpr);
                    const float al = en.ok ? expf(e - l) : 0.f;
                    const float ds = al * (da - Dv);
                    axpy_head_row<VEC, NT>(acck, ds, qv[u]);
                    axpy_head_row<VEC, NT>(accv, al, gv[u]);
                }
            }
        }
        fold_store_head_row<VEC, NT>(G_Zk + row * ldgzk + (size_t)k * dh, acck, lpr, sub, grp, dh,
                                     [&](int, int, float x) { return fmaf(x, c, 0.f); });
        fold_store_head_row<VEC, NT>(G_Zv + row * ldgzv + (size_t)k * dh, accv, lpr, sub, grp, dh);
    }
}

// The bodies of the entry points.  The float4 path needs every dense operand's rows aligned for four columns -- 16 bytes
// of fp32, 8 bytes of a bf16 image (rows16) --, so a call on images runs the (VEC, NT, U) the fp32 call runs on the
// widened operands, equally aligned in elements.
template <class GT>
void gatdot_forward(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr, const uint32_t *indices,
                    const float *Zq, size_t ldq, const GT *Zk, size_t ldk, const GT *Zv, size_t ldv, uint32_t K, uint32_t dh,
                    float scale, float *out, size_t ldo, float *lse) {
    require_heads(K, dh);
    const size_t width = (size_t)K * dh;
    MGGCN_REQUIRE(ldq >= width && ldk >= width && ldv >= width && ldo >= width,
                  "gatdot forward: leading dimension < heads * width per head");
    if (!n_rows) return;
    MGGCN_REQUIRE(indptr != nullptr && Zq != nullptr && out != nullptr && lse != nullptr, "gatdot forward: null operand");
    MGGCN_REQUIRE(n_cols == 0 || (indices != nullptr && Zk != nullptr && Zv != nullptr), "gatdot forward: null operand");
    const void *zk = Zk, *zv = Zv;
    MGGCN_REQUIRE(out != Zq && out != zk && out != zv, "gatdot forward: out must not alias Zq, Zk or Zv");
    const bool vec = dh % 4 == 0 && rows16(Zq, ldq) && rows16(Zk, ldk) && rows16(Zv, ldv) && rows16(out, ldo);
    const head_geometry hg = head_geometry_for(dh, vec);
    gat_dispatch(vec, hg.nt, [&](auto v) {
        launch_rows(gatdot_forward_kernel<v.VEC, v.NT, v.U, GT>, n_rows, stream, n_rows, indptr, indices, Zq, ldq, Zk, ldk, Zv, ldv,
                    K, dh, scale, hg.lg, out, ldo, lse);
    });
}

template <class GT>
void gatdot_backward_dst(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                         const uint32_t *indices, const float *Zq, size_t ldq, const GT *Zk, size_t ldk, const GT *Zv,
                         size_t ldv, const float *lse, const float *G, size_t ldg, const float *out, size_t ldo, uint32_t K,
                         uint32_t dh, float scale, float *D, float *G_Zq, size_t ldgzq) {
    require_heads(K, dh);
    const size_t width = (size_t)K * dh;
    MGGCN_REQUIRE(ldq >= width && ldk >= width && ldv >= width && ldg >= width && ldo >= width && ldgzq >= width,
                  "gatdot backward: leading dimension < heads * width per head");
    if (!n_rows) return;
    MGGCN_REQUIRE(indptr != nullptr && Zq != nullptr && lse != nullptr && G != nullptr && out != nullptr && D != nullptr &&
                      G_Zq != nullptr,
                  "gatdot backward: null operand");
    MGGCN_REQUIRE(n_cols == 0 || (indices != nullptr && Zk != nullptr && Zv != nullptr), "gatdot backward: null operand");
    const void *zk = Zk, *zv = Zv;
    MGGCN_REQUIRE(G_Zq != G && G_Zq != Zq && G_Zq != zk && G_Zq != zv && G_Zq != out,
                  "gatdot backward: G_Zq must not alias an input");
    const bool vec = dh % 4 == 0 && rows16(Zq, ldq) && rows16(Zk, ldk) && rows16(Zv, ldv) && rows16(G, ldg) && rows16(out, ldo) &&
                     rows16(G_Zq, ldgzq);
    const head_geometry hg = head_geometry_for(dh, vec);
    gat_dispatch(vec, hg.nt, [&](auto v) {
        launch_rows(gatdot_backward_dst_kernel<v.VEC, v.NT, v.U, GT>, n_rows, stream, n_rows, indptr, indices, Zq, ldq, Zk, ldk, Zv,
                    ldv, lse, G, ldg, out, ldo, K, dh, scale, hg.lg, D, G_Zq, ldgzq);
    });
}

template <class GT>
void gatdot_backward_src(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                         const uint32_t *t_indices, const GT *Zq, size_t ldq, const float *Zk, size_t ldk, const float *Zv,
                         size_t ldv, const float *lse, const float *D, const GT *G, size_t ldg, uint32_t K, uint32_t dh,
                         float scale, float *G_Zk, size_t ldgzk, float *G_Zv, size_t ldgzv) {
    require_heads(K, dh);
    const size_t width = (size_t)K * dh;
    MGGCN_REQUIRE(ldq >= width && ldk >= width && ldv >= width && ldg >= width && ldgzk >= width && ldgzv >= width,
                  "gatdot backward: leading dimension < heads * width per head");
    if (!n_rows) return;
    MGGCN_REQUIRE(t_indptr != nullptr && Zk != nullptr && Zv != nullptr && G_Zk != nullptr && G_Zv != nullptr,
                  "gatdot backward: null operand");
    MGGCN_REQUIRE(n_cols == 0 || (t_indices != nullptr && Zq != nullptr && G != nullptr && lse != nullptr && D != nullptr),
                  "gatdot backward: null operand");
    const void *g = G, *zq = Zq;
    MGGCN_REQUIRE(G_Zk != g && G_Zk != zq && G_Zk != Zk && G_Zk != Zv && G_Zv != g && G_Zv != zq && G_Zv != Zk && G_Zv != Zv &&
                      G_Zk != G_Zv,
                  "gatdot backward: G_Zk and G_Zv must not alias an input or each other");
    const bool vec = dh % 4 == 0 && rows16(Zq, ldq) && rows16(Zk, ldk) && rows16(Zv, ldv) && rows16(G, ldg) &&
                     rows16(G_Zk, ldgzk) && rows16(G_Zv, ldgzv);
    const head_geometry hg = head_geometry_for(dh, vec);
    gat_dispatch(vec, hg.nt, [&](auto v) {
        launch_rows(gatdot_backward_src_kernel<v.VEC, v.NT, v.U, GT>, n_rows, stream, n_rows, t_indptr, t_indices, Zq, ldq, Zk, ldk,
                    Zv, ldv, lse, D, G, ldg, K, dh, scale, hg.lg, G_Zk, ldgzk, G_Zv, ldgzv);
    });
}

}  // namespace
