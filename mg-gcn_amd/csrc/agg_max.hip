// agg_max.hip -- the element-wise maximum over a vertex's neighbours (GraphSAGE's max aggregator) on gfx950, forward and
// backward.  Both kernels are built on gat_internal.h as the attention kernels are (gat.hip describes the layout): one wave
// per CSR row, the row's entries in 64-entry chunks (entry_chunks), the wave cut into 64 / LPR groups of LPR lanes that hold
// one dense row each -- one head of width d in the terms of head_geometry_for --, VEC columns per lane and NT column tiles, U
// entries per group and step, and the five (VEC, NT, U) variants of gat_dispatch.  No LDS, no atomics, no per-edge array.
//   forward   out[i, c] = max over the entries j of row i of B[j, c] and arg[i, c] = src0 + j of the winner.  A SELECTION under
//             a total order on (value, j): the larger value wins, equal values (==: -0.0 ties with +0.0) go to the smaller j,
//             a NaN is never selected.  Every group keeps its best (value, j) per column, the groups meet in a butterfly over
//             the pairs under the same order, and the winner's bits are stored as they were loaded.  The result is therefore
//             a function of the SET of (j, B[j, c]) of the row: not of the lane geometry, the chunking, the order of the
//             entries or duplicates, and the float4 and the element path give the same bits.
//   backward  over the rows j of F^T, whose entries are the destinations i: G_B[j, c] = the sum of G[i, c] over the entries
//             with arg[i, c] == src0 + j.  An entry gathers one row of arg and one row of G and adds G[i, c] or +0.0 by a
//             select; a group adds its entries in row order, the groups are folded by fold_groups.  An entry whose index
//             equals its predecessor's in the row is skipped, so a pair (i, j) that the pattern holds twice delivers once:
//             equal indices of a row must be adjacent, which holds for a row in ascending order.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "gat_internal.h"

namespace {

constexpr uint32_t kAggNone = MGGCN_AGG_NONE;

template <int VEC>
__device__ __forceinline__ void loadv_u32(uint32_t (&r)[VEC], const uint32_t *p) {
    if constexpr (VEC == 4) {
        const uint4 t = *reinterpret_cast<const uint4 *>(p);
        r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w;
    } else {
        r[0] = *p;
    }
}
template <int VEC>
__device__ __forceinline__ void storev_u32(uint32_t *p, const uint32_t (&r)[VEC]) {
    if constexpr (VEC == 4) *reinterpret_cast<uint4 *>(p) = make_uint4(r[0], r[1], r[2], r[3]);
    else *p = r[0];
}

// the total order of the forward: does (x, j) beat (b, bj)?  A NaN x fails both comparisons; (-inf, NONE), the start, loses
// to every entry that is not a NaN, a row of -inf included (NONE is larger than any index)
__device__ __forceinline__ bool agg_beats(float x, uint32_t j, float b, uint32_t bj) { return x > b || (x == b && j < bj); }

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <int VEC, int NT, int U>
__global__ __launch_bounds__(256) void agg_max_forward_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                              const uint32_t *__restrict__ indices,
                                                              const float *__restrict__ B, size_t ldb, uint32_t d, uint32_t src0,
                                                              uint32_t lg, float *__restrict__ out, size_t ldo,
                                                              uint32_t *__restrict__ arg, size_t lda) {
    MGGCN_GAT_WAVE_ROW(n_rows);
    const uint32_t beg = indptr[row], end = indptr[row + 1];
    float best[NT][VEC];
    uint32_t bj[NT][VEC];
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int v = 0; v < VEC; v++) {
            best[t][v] = -INFINITY;
            bj[t][v] = kAggNone;
        }
    entry_chunks<0> ch;
    ch.start(indices, beg, end, lane, no_scalars);
    for (uint32_t base = beg; base < end; base += 64) {
        ch.next(indices, base, end, lane, no_scalars);
        const uint32_t cnt = ch.cnt;
        for (uint32_t j = 0; j < cnt; j += n_grp * U) {
            float z[U][NT][VEC];
            chunk_entry en[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                en[u] = ch.pick(j, u, n_grp, grp);
                load_head_row<VEC, NT>(z[u], B + (size_t)en[u].c * ldb, lpr, sub, d, en[u].ok);
            }
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int t = 0; t < NT; t++)
#pragma unroll
                    for (int v = 0; v < VEC; v++) {
                        const bool take = en[u].ok && agg_beats(z[u][t][v], en[u].c, best[t][v], bj[t][v]);
                        best[t][v] = take ? z[u][t][v] : best[t][v];
                        bj[t][v] = take ? en[u].c : bj[t][v];
                    }
        }
    }
    // the groups meet: a butterfly over (value, j) pairs under the same order, so every group ends with the row's winner
#pragma unroll
    for (int t = 0; t < NT; t++) {
        uint32_t a[VEC];
#pragma unroll
        for (int v = 0; v < VEC; v++) {
            float b = best[t][v];
            uint32_t j = bj[t][v];
            for (uint32_t off = lpr; off < 64; off <<= 1) {
                const float ob = __shfl_xor(b, off);
                const uint32_t oj = __shfl_xor(j, off);
                const bool take = agg_beats(ob, oj, b, j);
                b = take ? ob : b;
                j = take ? oj : j;
            }
            const bool sel = j != kAggNone;             // nothing selected (no entry, or NaNs only): +0.0 and NONE
            best[t][v] = sel ? b : 0.f;
            a[v] = sel ? src0 + j : kAggNone;
        }
        const uint32_t col = (t * lpr + sub) * VEC;
        if (grp == 0 && col < d) {
            storev<VEC>(out + row * ldo + col, best[t]);
            if (arg) storev_u32<VEC>(arg + row * lda + col, a);
        }
    }
}

// ---------------------------------------------------------------------------
// backward over the rows of F^T
// ---------------------------------------------------------------------------
template <int VEC, int NT, int U, bool ACC>
__global__ __launch_bounds__(256) void agg_max_backward_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                               const uint32_t *__restrict__ indices,
                                                               const uint32_t *__restrict__ arg, size_t lda,
                                                               const float *__restrict__ G, size_t ldg, uint32_t d,
                                                               uint32_t src0, uint32_t lg, float *__restrict__ G_B,
                                                               size_t ldgb) {
    MGGCN_GAT_WAVE_ROW(n_rows);
    const uint32_t beg = indptr[row], end = indptr[row + 1];
    const uint32_t me = src0 + (uint32_t)row;
    float acc[NT][VEC];
    zero_head_row<VEC, NT>(acc);
    uint32_t carry = 0;                                   // the index of the entry before this chunk's first
    entry_chunks<0> ch;
    ch.start(indices, beg, end, lane, no_scalars);
    for (uint32_t base = beg; base < end; base += 64) {
        ch.next(indices, base, end, lane, no_scalars);
        const uint32_t cnt = ch.cnt;
        // an entry equal to its predecessor in the row is a duplicate pair: it delivers nothing
        uint32_t prev = __shfl_up(ch.my_c, 1);
        if (lane == 0) prev = carry;
        const bool first = base == beg && lane == 0;
        const uint32_t my_live = lane < cnt && (first || prev != ch.my_c) ? 1u : 0u;
        carry = __shfl(ch.my_c, 63);                      // read by the next chunk only, and then this one was full
        for (uint32_t j = 0; j < cnt; j += n_grp * U) {
            float g[U][NT][VEC];
            uint32_t a[U][NT][VEC];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const chunk_entry en = ch.pick(j, u, n_grp, grp);
                const uint32_t live = en.of(my_live);       // by every lane: a ds_bpermute reads active lanes only
                const bool on = en.ok && live != 0;
                const uint32_t *__restrict__ ar = arg + (size_t)en.c * lda;
                const float *__restrict__ gr = G + (size_t)en.c * ldg;
#pragma unroll
                for (int t = 0; t < NT; t++) {              // the entry's rows of arg and G under one predicate
                    const uint32_t col = (t * lpr + sub) * VEC;
                    if (on && col < d) {
                        loadv_u32<VEC>(a[u][t], ar + col);
                        loadv<VEC>(g[u][t], gr + col);
                    } else {
                        zerov<VEC>(g[u][t]);
#pragma unroll
                        for (int v = 0; v < VEC; v++) a[u][t][v] = kAggNone;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int t = 0; t < NT; t++)
#pragma unroll
                    for (int v = 0; v < VEC; v++) acc[t][v] += a[u][t][v] == me ? g[u][t][v] : 0.f;
        }
    }
#pragma unroll
    for (int t = 0; t < NT; t++) {
#pragma unroll
        for (int v = 0; v < VEC; v++) acc[t][v] = fold_groups(acc[t][v], lpr);
        const uint32_t col = (t * lpr + sub) * VEC;
        if (grp == 0 && col < d) {
            float *p = G_B + row * ldgb + col;
            if constexpr (ACC) {
                float old[VEC];
                loadv<VEC>(old, p);
#pragma unroll
                for (int v = 0; v < VEC; v++) acc[t][v] = old[v] + acc[t][v];
            }
            storev<VEC>(p, acc[t]);
        }
    }
}

bool rows16_u32(const uint32_t *p, size_t ld) { return aligned16(p) && ld % 4 == 0; }

}  // namespace

// ============================ C ABI =========================================
MGGCN_API void mggcn_agg_max_forward_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                         const uint32_t *indices, const float *B, size_t ldb, uint32_t d, uint32_t src0,
                                         float *out, size_t ldo, uint32_t *arg, size_t lda) {
    require_heads(1, d);
    MGGCN_REQUIRE(ldb >= d && ldo >= d && (arg == nullptr || lda >= d), "agg max forward: leading dimension < width");
    MGGCN_REQUIRE((uint64_t)src0 + n_cols <= 0xFFFFFFFFull, "agg max forward: src0 + sources must stay below 2^32 - 1 (MGGCN_AGG_NONE)");
    if (!n_rows) return;
    MGGCN_REQUIRE(indptr != nullptr && out != nullptr, "agg max forward: null operand");
    MGGCN_REQUIRE(n_cols == 0 || (indices != nullptr && B != nullptr), "agg max forward: null operand");
    MGGCN_REQUIRE((const void *)out != (const void *)B, "agg max forward: out must not alias B");
    const bool vec = d % 4 == 0 && rows16(B, ldb) && rows16(out, ldo) && (arg == nullptr || rows16_u32(arg, lda));
    const head_geometry hg = head_geometry_for(d, vec);
    gat_dispatch(vec, hg.nt, [&](auto v) {
        launch_rows(agg_max_forward_kernel<v.VEC, v.NT, v.U>, n_rows, stream, n_rows, indptr, indices, B, ldb, d, src0, hg.lg,
                    out, ldo, arg, lda);
    });
}

MGGCN_API void mggcn_agg_max_backward_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                                          const uint32_t *t_indices, const uint32_t *arg, size_t lda, const float *G,
                                          size_t ldg, uint32_t d, uint32_t src0, uint32_t flags, float *G_B, size_t ldgb) {
    require_heads(1, d);
    MGGCN_REQUIRE((flags & ~MGGCN_AGG_ACCUMULATE) == 0, "agg max backward: unknown flags");
    MGGCN_REQUIRE(lda >= d && ldg >= d && ldgb >= d, "agg max backward: leading dimension < width");
    MGGCN_REQUIRE((uint64_t)src0 + n_rows <= 0xFFFFFFFFull, "agg max backward: src0 + sources must stay below 2^32 - 1 (MGGCN_AGG_NONE)");
    if (!n_rows) return;
    MGGCN_REQUIRE(t_indptr != nullptr && G_B != nullptr, "agg max backward: null operand");
    MGGCN_REQUIRE(n_cols == 0 || (t_indices != nullptr && arg != nullptr && G != nullptr), "agg max backward: null operand");
    MGGCN_REQUIRE((const void *)G_B != (const void *)G, "agg max backward: G_B must not alias G");
    const bool vec = d % 4 == 0 && rows16_u32(arg, lda) && rows16(G, ldg) && rows16(G_B, ldgb);
    const head_geometry hg = head_geometry_for(d, vec);
    gat_dispatch(vec, hg.nt, [&](auto v) {
        with_flag((flags & MGGCN_AGG_ACCUMULATE) != 0, [&](auto acc) {
            launch_rows(agg_max_backward_kernel<v.VEC, v.NT, v.U, acc>, n_rows, stream, n_rows, t_indptr, t_indices, arg, lda, G,
                        ldg, d, src0, hg.lg, G_B, ldgb);
        });
    });
}
