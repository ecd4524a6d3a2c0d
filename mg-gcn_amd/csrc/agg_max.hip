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
//   record    (REC = true, mggcn_agg_max_backward_rec_f32): the two gathered rows come from ONE matrix of 8-byte records that
//             agg_max_pack_kernel interleaves -- words 2c and 2c + 1 of row i are the bits of arg[i, c] and of G[i, c].  A
//             lane's four columns are 32 contiguous bytes (two adjacent 16-byte loads) where the plain kernel reads 16 bytes
//             of each of two rows; the element path reads one 8-byte record per column.  Only the loads differ: the walk,
//             the skip rule, the select and the order of the sums, and so every bit of G_B, are the plain kernel's.
//             REC = false compiles to the kernel as it was.  What the row partition exchanges in one collective
//             (DESIGN.md 3.13.1).
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

// (arg, G) of VEC columns from `col` on of one destination: two rows (ar, gr), or -- REC -- the row `ar` of interleaved records
template <int VEC, bool REC>
__device__ __forceinline__ void load_sel_grad(uint32_t (&a)[VEC], float (&g)[VEC], const uint32_t *__restrict__ ar,
                                              const float *__restrict__ gr, uint32_t col) {
    if constexpr (!REC) {
        loadv_u32<VEC>(a, ar + col);
        loadv<VEC>(g, gr + col);
    } else if constexpr (VEC == 4) {
        const uint4 lo = *reinterpret_cast<const uint4 *>(ar + 2 * (size_t)col);
        const uint4 hi = *reinterpret_cast<const uint4 *>(ar + 2 * (size_t)col + 4);
        a[0] = lo.x; g[0] = __uint_as_float(lo.y); a[1] = lo.z; g[1] = __uint_as_float(lo.w);
        a[2] = hi.x; g[2] = __uint_as_float(hi.y); a[3] = hi.z; g[3] = __uint_as_float(hi.w);
    } else {
        const uint2 t = *reinterpret_cast<const uint2 *>(ar + 2 * (size_t)col);
        a[0] = t.x; g[0] = __uint_as_float(t.y);
    }
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
// REC: G is not read; `arg` is the record matrix and `lda` its leading dimension in 32-bit words
template <int VEC, int NT, int U, bool ACC, bool REC>
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
                const float *__restrict__ gr = REC ? nullptr : G + (size_t)en.c * ldg;
#pragma unroll
                for (int t = 0; t < NT; t++) {              // the entry's rows of arg and G under one predicate
                    const uint32_t col = (t * lpr + sub) * VEC;
                    if (on && col < d) {
                        load_sel_grad<VEC, REC>(a[u][t], g[u][t], ar, gr, col);
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

// ---------------------------------------------------------------------------
// the record: rec[i, 2c] = arg[i, c], rec[i, 2c + 1] = the bits of G[i, c].  One thread per (row, VEC columns), grid-stride
// ---------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(256) void agg_max_pack_kernel(const uint32_t *__restrict__ arg, size_t lda,
                                                           const float *__restrict__ G, size_t ldg, size_t n_rows, uint32_t d,
                                                           uint32_t *__restrict__ rec, size_t ldr) {
    const uint32_t units = d / VEC;
    const size_t total = n_rows * units;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const size_t row = idx / units;
        const uint32_t col = (uint32_t)(idx - row * units) * VEC;
        uint32_t a[VEC], g[VEC];
        loadv_u32<VEC>(a, arg + row * lda + col);
        loadv_u32<VEC>(g, reinterpret_cast<const uint32_t *>(G) + row * ldg + col);
        uint32_t *p = rec + row * ldr + 2 * (size_t)col;
        if constexpr (VEC == 4) {
            *reinterpret_cast<uint4 *>(p) = make_uint4(a[0], g[0], a[1], g[1]);
            *reinterpret_cast<uint4 *>(p + 4) = make_uint4(a[2], g[2], a[3], g[3]);
        } else {
            *reinterpret_cast<uint2 *>(p) = make_uint2(a[0], g[0]);
        }
    }
}

bool rows16_u32(const uint32_t *p, size_t ld) { return aligned16(p) && ld % 4 == 0; }

// the launch both backward entry points share: `vec` is the caller's float4 condition on its own operands
template <bool REC>
void agg_max_backward_launch(mggcn_stream_t stream, bool vec, uint32_t n_rows, const uint32_t *t_indptr,
                             const uint32_t *t_indices, const uint32_t *arg, size_t lda, const float *G, size_t ldg, uint32_t d,
                             uint32_t src0, uint32_t flags, float *G_B, size_t ldgb) {
    const head_geometry hg = head_geometry_for(d, vec);
    gat_dispatch(vec, hg.nt, [&](auto v) {
        with_flag((flags & MGGCN_AGG_ACCUMULATE) != 0, [&](auto acc) {
            launch_rows(agg_max_backward_kernel<v.VEC, v.NT, v.U, acc, REC>, n_rows, stream, n_rows, t_indptr, t_indices, arg,
                        lda, G, ldg, d, src0, hg.lg, G_B, ldgb);
        });
    });
}

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
    agg_max_backward_launch<false>(stream, vec, n_rows, t_indptr, t_indices, arg, lda, G, ldg, d, src0, flags, G_B, ldgb);
}

MGGCN_API void mggcn_agg_max_pack_f32(mggcn_stream_t stream, const uint32_t *arg, size_t lda, const float *G, size_t ldg,
                                      size_t n_rows, uint32_t d, uint32_t *rec, size_t ldr) {
    require_heads(1, d);
    MGGCN_REQUIRE(lda >= d && ldg >= d && ldr >= 2 * (size_t)d, "agg max pack: leading dimension < width");
    MGGCN_REQUIRE((reinterpret_cast<uintptr_t>(rec) & 7u) == 0 && ldr % 2 == 0,
                  "agg max pack: rec must be 8-byte aligned with an even leading dimension");
    if (!n_rows) return;
    MGGCN_REQUIRE(arg != nullptr && G != nullptr && rec != nullptr, "agg max pack: null operand");
    MGGCN_REQUIRE((const void *)rec != (const void *)arg && (const void *)rec != (const void *)G,
                  "agg max pack: rec must not alias an input");
    const bool vec = d % 4 == 0 && rows16_u32(arg, lda) && rows16(G, ldg) && rows16_u32(rec, ldr);
    const size_t total = n_rows * (vec ? d / 4 : d);
    const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, 1u << 20);
    const auto kernel = vec ? agg_max_pack_kernel<4> : agg_max_pack_kernel<1>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, as_stream(stream), arg, lda, G, ldg, n_rows, d, rec, ldr);
    MGGCN_CHECK_LAUNCH();
}

MGGCN_API void mggcn_agg_max_backward_rec_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                                              const uint32_t *t_indices, const uint32_t *rec, size_t ldr, uint32_t d,
                                              uint32_t src0, uint32_t flags, float *G_B, size_t ldgb) {
    require_heads(1, d);
    MGGCN_REQUIRE((flags & ~MGGCN_AGG_ACCUMULATE) == 0, "agg max backward rec: unknown flags");
    MGGCN_REQUIRE(ldr >= 2 * (size_t)d && ldgb >= d, "agg max backward rec: leading dimension < width");
    MGGCN_REQUIRE((reinterpret_cast<uintptr_t>(rec) & 7u) == 0 && ldr % 2 == 0,
                  "agg max backward rec: rec must be 8-byte aligned with an even leading dimension");
    MGGCN_REQUIRE((uint64_t)src0 + n_rows <= 0xFFFFFFFFull, "agg max backward rec: src0 + sources must stay below 2^32 - 1 (MGGCN_AGG_NONE)");
    if (!n_rows) return;
    MGGCN_REQUIRE(t_indptr != nullptr && G_B != nullptr, "agg max backward rec: null operand");
    MGGCN_REQUIRE(n_cols == 0 || (t_indices != nullptr && rec != nullptr), "agg max backward rec: null operand");
    MGGCN_REQUIRE((const void *)G_B != (const void *)rec, "agg max backward rec: G_B must not alias rec");
    // the plain call's condition on equally aligned operands: a 16-byte record row is a 16-byte arg row and a 16-byte G row
    const bool vec = d % 4 == 0 && rows16_u32(rec, ldr) && rows16(G_B, ldgb);
    agg_max_backward_launch<true>(stream, vec, n_rows, t_indptr, t_indices, rec, ldr, nullptr, 0, d, src0, flags, G_B, ldgb);
}
