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
template <int VEC, int NT, int U>
__global__ __launch_bounds__(256) void gatv2_forward_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                            const uint32_t *__restrict__ indices,
                                                            const float *__restrict__ Zs, size_t ldzs,
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
        const float *__restrict__ Zk = Zs + (size_t)k * dh;
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
template <int VEC, int NT, int U>
__global__ __launch_bounds__(256) void gatv2_backward_dst_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                                 const uint32_t *__restrict__ indices,
                                                                 const float *__restrict__ Zs, size_t ldzs,
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
        const float *__restrict__ Zk = Zs + (size_t)k * dh;
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
template <int VEC, int NT, int U, bool REC>
__global__ __launch_bounds__(256) void gatv2_backward_src_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                                 const uint32_t *__restrict__ indices,
                                                                 const float *__restrict__ Zs, size_t ldzs,
                                                                 const float *__restrict__ Zd, size_t ldzd,
                                                                 const float *__restrict__ att, const float *__restrict__ lse,
                                                                 const float *__restrict__ D, const float *__restrict__ rec,
                                                                 const float *__restrict__ G, size_t ldg, uint32_t K,
                                                                 uint32_t dh, float slope, uint32_t lg,
                                                                 float *__restrict__ G_Zs, size_t ldgzs) {
    MGGCN_GAT_WAVE_ROW(n_rows);
    const uint32_t beg = indptr[row], end = indptr[row + 1];
    for (uint32_t k = 0; k < K; k++) {
        float zs[NT][VEC], a[NT][VEC], acc[NT][VEC];
        load_head_row<VEC, NT>(zs, Zs + row * ldzs + (size_t)k * dh, lpr, sub, dh);
        load_head_row<VEC, NT>(a, att + (size_t)k * dh, lpr, sub, dh);
        zero_head_row<VEC, NT>(acc);
        const float *__restrict__ Zdk = Zd + (size_t)k * dh;
        const float *__restrict__ Gk = G + (size_t)k * dh;
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
    require_heads(K, dh);
    const size_t width = (size_t)K * dh;
    MGGCN_REQUIRE(ldzs >= width && ldzd >= width && ldo >= width, "gatv2 forward: leading dimension < heads * width per head");
    if (!n_rows) return;
    MGGCN_REQUIRE(indptr != nullptr && Zd != nullptr && att != nullptr && out != nullptr && lse != nullptr,
                  "gatv2 forward: null operand");
    MGGCN_REQUIRE(n_cols == 0 || (indices != nullptr && Zs != nullptr), "gatv2 forward: null operand");
    MGGCN_REQUIRE(out != Zs && out != Zd, "gatv2 forward: out must not alias Zs or Zd");
    const bool vec = dh % 4 == 0 && rows16(Zs, ldzs) && rows16(Zd, ldzd) && rows16(out, ldo) && aligned16(att);
    const head_geometry hg = head_geometry_for(dh, vec);
    gat_dispatch(vec, hg.nt, [&](auto v) {
        launch_rows(gatv2_forward_kernel<v.VEC, v.NT, v.U>, n_rows, stream, n_rows, indptr, indices, Zs, ldzs, Zd, ldzd, att, K, dh,
                    slope, hg.lg, out, ldo, lse);
    });
}

MGGCN_API void mggcn_gatv2_backward_dst_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                            const uint32_t *indices, const float *Zs, size_t ldzs, const float *Zd,
                                            size_t ldzd, const float *att, const float *lse, const float *G, size_t ldg,
                                            const float *out, size_t ldo, uint32_t K, uint32_t dh, float slope, float *D,
                                            float *G_Zd, size_t ldgzd, float *P, size_t ldp) {
    require_heads(K, dh);
    const size_t width = (size_t)K * dh;
    MGGCN_REQUIRE(ldzs >= width && ldzd >= width && ldg >= width && ldo >= width && ldgzd >= width && ldp >= width,
                  "gatv2 backward: leading dimension < heads * width per head");
    if (!n_rows) return;
    MGGCN_REQUIRE(indptr != nullptr && Zd != nullptr && att != nullptr && lse != nullptr && G != nullptr && out != nullptr &&
                      D != nullptr && G_Zd != nullptr && P != nullptr,
                  "gatv2 backward: null operand");
    MGGCN_REQUIRE(n_cols == 0 || (indices != nullptr && Zs != nullptr), "gatv2 backward: null operand");
    MGGCN_REQUIRE(G_Zd != G && G_Zd != Zs && G_Zd != Zd && G_Zd != out && P != G && P != Zs && P != Zd && P != out && P != G_Zd,
                  "gatv2 backward: G_Zd and P must not alias an input or each other");
    const bool vec = dh % 4 == 0 && rows16(Zs, ldzs) && rows16(Zd, ldzd) && rows16(G, ldg) && rows16(out, ldo) &&
                     rows16(G_Zd, ldgzd) && rows16(P, ldp) && aligned16(att);
    const head_geometry hg = head_geometry_for(dh, vec);
    gat_dispatch(vec, hg.nt, [&](auto v) {
        launch_rows(gatv2_backward_dst_kernel<v.VEC, v.NT, v.U>, n_rows, stream, n_rows, indptr, indices, Zs, ldzs, Zd, ldzd, att,
                    lse, G, ldg, out, ldo, K, dh, slope, hg.lg, D, G_Zd, ldgzd, P, ldp);
    });
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

// The body of backward_src and of its record form: rec != nullptr launches the REC = true kernels, which read it in place of
// lse and D (both nullptr then).  Internal linkage.
namespace {
void gatv2_backward_src(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                        const uint32_t *t_indices, const float *Zs, size_t ldzs, const float *Zd, size_t ldzd, const float *att,
                        const float *lse, const float *D, const float *rec, const float *G, size_t ldg, uint32_t K, uint32_t dh,
                        float slope, float *G_Zs, size_t ldgzs) {
    require_heads(K, dh);
    const size_t width = (size_t)K * dh;
    MGGCN_REQUIRE(ldzs >= width && ldzd >= width && ldg >= width && ldgzs >= width,
                  "gatv2 backward: leading dimension < heads * width per head");
    if (!n_rows) return;
    MGGCN_REQUIRE(t_indptr != nullptr && Zs != nullptr && att != nullptr && G_Zs != nullptr, "gatv2 backward: null operand");
    MGGCN_REQUIRE(n_cols == 0 || (t_indices != nullptr && Zd != nullptr && G != nullptr &&
                                  (rec != nullptr || (lse != nullptr && D != nullptr))),
                  "gatv2 backward: null operand");
    MGGCN_REQUIRE(G_Zs != G && G_Zs != Zs && G_Zs != Zd, "gatv2 backward: G_Zs must not alias G, Zs or Zd");
    const bool vec = dh % 4 == 0 && rows16(Zs, ldzs) && rows16(Zd, ldzd) && rows16(G, ldg) && rows16(G_Zs, ldgzs) && aligned16(att);
    const head_geometry hg = head_geometry_for(dh, vec);
    gat_dispatch(vec, hg.nt, [&](auto v) {
        with_flag(rec != nullptr, [&](auto packed) {
            launch_rows(gatv2_backward_src_kernel<v.VEC, v.NT, v.U, packed>, n_rows, stream, n_rows, t_indptr, t_indices, Zs, ldzs,
                        Zd, ldzd, att, lse, D, rec, G, ldg, K, dh, slope, hg.lg, G_Zs, ldgzs);
        });
    });
}
}  // namespace

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
