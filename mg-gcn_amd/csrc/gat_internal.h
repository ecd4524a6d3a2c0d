// gat_internal.h -- what the graph attention kernels of gat.hip (GAT), gatv2.hip (GATv2) and gatdot.hip share: the one-wave-per-row
// layout with LPR-lane groups (gat.hip describes it), the walk over a row's entries (entry_chunks), the group butterfly,
// the head-row loads (of fp32 rows and, for the _b16 translation units, of bf16 images), zero, dot product, axpy and the epilogue, D = G . out of a row (head_row_D), the (lse, D) fetch of an
// entry's destination (fetch_lse_D), the per-group online softmax of the GATv2 and dot-product forwards (group_softmax), the
// head geometry, the (VEC, NT, U) dispatch with the row launch, and the column-sum pass behind G_att.  Internal linkage in
// each translation unit that includes it.  Not part of the ABI.
#pragma once

#include <algorithm>
#include <type_traits>

#include "common.h"
#include "reduce.h"
#include "scratch_internal.h"

namespace {

constexpr unsigned kGatColsumBlocks = kNumCU * 2;      // grid cap of the G_att partial pass = rows of partials in the scratch

// sum over the lanes of a group (offsets below lpr) / over the groups (offsets from lpr up)
__device__ __forceinline__ float group_sum(float v, uint32_t lpr) {
    for (uint32_t off = 1; off < lpr; off <<= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ float fold_groups(float v, uint32_t lpr) {
    for (uint32_t off = lpr; off < 64; off <<= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ float gat_lrelu(float x, float slope) { return x > 0.f ? x : slope * x; }

template <int VEC>
__device__ __forceinline__ void loadv(float (&r)[VEC], const float *p) {
    if constexpr (VEC == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w;
    } else {
        r[0] = *p;
    }
}
// The same columns of a bf16 image (bit patterns, uint16_t): one 8-byte load for four columns, one 2-byte load for one, and
// every value widened exactly -- its bits shifted left by 16, so -0.0 and the denormals survive.  What follows a load is
// the fp32 instruction stream in the fp32 order: a kernel on an image gives the bits it gives on the widened fp32 operand.
template <int VEC>
__device__ __forceinline__ void loadv(float (&r)[VEC], const uint16_t *p) {
    if constexpr (VEC == 4) {
        const uint2 t = *reinterpret_cast<const uint2 *>(p);
        r[0] = __uint_as_float(t.x << 16); r[1] = __uint_as_float(t.x & 0xFFFF0000u);
        r[2] = __uint_as_float(t.y << 16); r[3] = __uint_as_float(t.y & 0xFFFF0000u);
    } else {
        r[0] = __uint_as_float((uint32_t)*p << 16);
    }
}
template <int VEC>
__device__ __forceinline__ void storev(float *p, const float (&r)[VEC]) {
    if constexpr (VEC == 4) *reinterpret_cast<float4 *>(p) = make_float4(r[0], r[1], r[2], r[3]);
    else *p = r[0];
}
template <int VEC>
__device__ __forceinline__ void zerov(float (&r)[VEC]) {
#pragma unroll
    for (int v = 0; v < VEC; v++) r[v] = 0.f;
}

// the head-row of `row` (NT tiles of VEC columns per lane), zeros beyond dh; T: float, or uint16_t for a bf16 image
template <int VEC, int NT, class T>
__device__ __forceinline__ void load_head_row(float (&r)[NT][VEC], const T *p, uint32_t lpr, uint32_t sub, uint32_t dh,
                                              bool on = true) {
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const uint32_t col = (t * lpr + sub) * VEC;
        if (on && col < dh) loadv<VEC>(r[t], p + col);
        else zerov<VEC>(r[t]);
    }
}
template <int VEC, int NT>
__device__ __forceinline__ void zero_head_row(float (&r)[NT][VEC]) {
#pragma unroll
    for (int t = 0; t < NT; t++) zerov<VEC>(r[t]);
}
template <int VEC, int NT>
__device__ __forceinline__ float dot_head_row(const float (&a)[NT][VEC], const float (&b)[NT][VEC]) {
    float p = 0.f;
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int v = 0; v < VEC; v++) p = fmaf(a[t][v], b[t][v], p);
    return p;
}
// acc += w z, element by element
template <int VEC, int NT>
__device__ __forceinline__ void axpy_head_row(float (&acc)[NT][VEC], float w, const float (&z)[NT][VEC]) {
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int v = 0; v < VEC; v++) acc[t][v] = fmaf(w, z[t][v], acc[t][v]);
}
// D[i, k] = G[i, head k] . out[i, head k] of the three backward_dst kernels: g is the row's head-row of G in every group,
// out_row = out + i ldo + k dh
template <int VEC, int NT>
__device__ __forceinline__ float head_row_D(const float (&g)[NT][VEC], const float *out_row, uint32_t lpr, uint32_t sub,
                                            uint32_t grp, uint32_t dh) {
    float o[NT][VEC];
    load_head_row<VEC, NT>(o, out_row, lpr, sub, dh, grp == 0);   // one group's worth
    return wave_sum(dot_head_row<VEC, NT>(g, o));
}

// the sums over a row's entries: fold the G groups in fixed order, post(t, v, sum) gives the element its final value (the
// forwards' 1 / sum, GATv2 backward_dst's att), and group 0 stores the columns below dh
template <int VEC, int NT, class Post>
__device__ __forceinline__ void fold_store_head_row(float *p, float (&acc)[NT][VEC], uint32_t lpr, uint32_t sub, uint32_t grp,
                                                    uint32_t dh, Post post) {
#pragma unroll
    for (int t = 0; t < NT; t++) {
#pragma unroll
        for (int v = 0; v < VEC; v++) acc[t][v] = post(t, v, fold_groups(acc[t][v], lpr));
        const uint32_t col = (t * lpr + sub) * VEC;
        if (grp == 0 && col < dh) storev<VEC>(p + col, acc[t]);
    }
}
template <int VEC, int NT>
__device__ __forceinline__ void fold_store_head_row(float *p, float (&acc)[NT][VEC], uint32_t lpr, uint32_t sub, uint32_t grp,
                                                    uint32_t dh) {
    fold_store_head_row<VEC, NT>(p, acc, lpr, sub, grp, dh, [](int, int, float x) { return x; });
}

// The entry group `grp` handles at step (j, u) of a chunk: its number in the chunk, its index, whether it exists; of(x) is
// the owner lane's x (ds_bpermute)
struct chunk_entry {
    uint32_t src, c;
    bool ok;
    template <class T>
    __device__ __forceinline__ T of(T x) const { return __shfl(x, src & 63); }
};

// The walk of one wave over the CSR row [beg, end) in 64-entry chunks, software-pipelined: lane l owns entry l of the chunk,
// its index is fetched two chunks ahead and its NS scalars -- fetch(c, s) loads those of index c into s[0 .. NS) -- one chunk
// ahead; whatever lies beyond the row's end is not fetched and reads as zero.  start() before the loop over base = beg,
// beg + 64, ...; next() at the top of every turn leaves the chunk's my_c, my_s and cnt = min(64, end - base).  The bounds are
// tested in 64 bits: a row may end within 128 entries of 2^32.
template <int NS>
struct entry_chunks {
    uint32_t my_c, cnt;
    float my_s[NS ? NS : 1];

    template <class Fetch>
    __device__ __forceinline__ void start(const uint32_t *__restrict__ indices, uint32_t beg, uint32_t end, uint32_t lane,
                                          Fetch fetch) {
        c1 = c2 = 0;
        zerov(s1);
        if ((size_t)beg + lane < end) { c1 = indices[beg + lane]; fetch(c1, s1); }
        if ((size_t)beg + 64 + lane < end) c2 = indices[beg + 64 + lane];
    }
    template <class Fetch>
    __device__ __forceinline__ void next(const uint32_t *__restrict__ indices, uint32_t base, uint32_t end, uint32_t lane,
                                         Fetch fetch) {
        my_c = c1;
#pragma unroll
        for (int s = 0; s < NS; s++) my_s[s] = s1[s];
        c1 = c2;
        zerov(s1); c2 = 0;
        if ((size_t)base + 64 + lane < end) fetch(c1, s1);
        if ((size_t)base + 128 + lane < end) c2 = indices[base + 128 + lane];
        cnt = min(64u, end - base);
    }
    __device__ __forceinline__ chunk_entry pick(uint32_t j, int u, uint32_t n_grp, uint32_t grp) const {
        const uint32_t src = j + u * n_grp + grp;
        return {src, (uint32_t)__shfl(my_c, src & 63), src < cnt};
    }

private:
    uint32_t c1, c2;
    float s1[NS ? NS : 1];
};
__device__ __forceinline__ void no_scalars(uint32_t, float *) {}

// The fetch of entry_chunks<2> in the GATv2 and dot-product backward_src kernels: lse and D of the entry's destination i at
// head k -- two 4-byte gathers, or (REC: lse and D are not read) one 8-byte load of the packed record rec[(i K + k) 2 + {0, 1}]
template <bool REC>
struct fetch_lse_D {
    const float *__restrict__ lse, *__restrict__ D, *__restrict__ rec;
    uint32_t K, k;
    __device__ __forceinline__ void operator()(uint32_t i, float *s) const {
        const size_t ik = (size_t)i * K + k;
        if constexpr (REC) {
            const float2 t = *reinterpret_cast<const float2 *>(rec + ik * 2);
            s[0] = t.x; s[1] = t.y;
        } else {
            s[0] = lse[ik]; s[1] = D[ik];
        }
    }
};

// The softmax of one row and head in ONE pass where the score of an entry exists only in the group that gathered it (the
// GATv2 and dot-product forwards; v1's forward has its scores per lane and a wave-wide maximum per chunk, a different
// algorithm).  The running maximum is kept PER GROUP: m, sum and the accumulators of a group are rescaled when its maximum
// moves.  start(); then add(e, z) per step of U entries -- e[u] the group-summed score of my group's u-th entry, -inf for
// one that does not exist, z[u] the head-row it contributes; finish() lets the groups meet at the wave's maximum M: group
// g enters with the factor exp(m_g - M), the sums and accumulators are folded in the fixed order of fold_groups,
// out = acc / sum and lse = M + log(sum).  The state (m, sum, acc: of my group, every lane of a group holds the same bits)
// is the kernel's own and every operation takes it by reference: as members of this struct, by value or by reference, the
// compiler splits packed adds and multiplies of the float4 variants and gatdot_forward<4, 1, 4> loses a wave per SIMD.
template <int VEC, int NT, int U>
struct group_softmax {
    __device__ static __forceinline__ void start(float &m, float &sum, float (&acc)[NT][VEC]) {
        m = -INFINITY;
        sum = 0.f;
        zero_head_row<VEC, NT>(acc);
    }
    __device__ static __forceinline__ void add(float &m, float &sum, float (&acc)[NT][VEC], const float (&e)[U],
                                               const float (&z)[U][NT][VEC]) {
        float m_new = m;
#pragma unroll
        for (int u = 0; u < U; u++) m_new = fmaxf(m_new, e[u]);
        // m_new = -inf: my group has not met an entry yet, nothing to rescale and every weight below is 0
        const float scale = m_new == -INFINITY ? 1.f : expf(m - m_new);     // 0 at the group's first entry
        float w[U], ws = 0.f;
#pragma unroll
        for (int u = 0; u < U; u++) {
            w[u] = e[u] == -INFINITY ? 0.f : expf(e[u] - m_new);
            ws += w[u];
        }
        sum = fmaf(sum, scale, ws);
        m = m_new;
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int v = 0; v < VEC; v++) {
                float s = acc[t][v] * scale;
#pragma unroll
                for (int u = 0; u < U; u++) s = fmaf(w[u], z[u][t][v], s);
                acc[t][v] = s;
            }
    }
    // out_row = out + i ldo + k dh, lse_ik = lse + i K + k; any: the row has an entry
    __device__ static __forceinline__ void finish(float &m, float &sum, float (&acc)[NT][VEC], float *out_row, float *lse_ik,
                                                  bool any, uint32_t lane, uint32_t lpr, uint32_t sub, uint32_t grp,
                                                  uint32_t dh) {
        // the groups meet at the wave's maximum; a group that never met an entry (m = -inf) enters with 0
        float M = m;
        for (uint32_t off = lpr; off < 64; off <<= 1) M = fmaxf(M, __shfl_xor(M, off));
        const float f = m == -INFINITY ? 0.f : expf(m - M);
        sum = fold_groups(sum * f, lpr);
        const float inv = any ? 1.f / sum : 0.f;
        if (lane == 0) *lse_ik = any ? M + logf(sum) : 0.f;
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int v = 0; v < VEC; v++) acc[t][v] *= f;
        fold_store_head_row<VEC, NT>(out_row, acc, lpr, sub, grp, dh,
                                     [&](int, int, float x) { return x * inv; });      // an empty row: +0.0
    }
};

#define MGGCN_GAT_WAVE_ROW(n_rows)                                                                            \
    const uint32_t lane = threadIdx.x & 63;                                                                   \
    const uint32_t lpr = 1u << lg, n_grp = 64u >> lg, sub = lane & (lpr - 1), grp = lane >> lg;               \
    const size_t row = (size_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);             \
    if (row >= (n_rows)) return

uint32_t ceil_log2(uint32_t x) {
    uint32_t l = 0;
    while ((1u << l) < x) l++;
    return l;
}

// group geometry of one head: log2(LPR) and the number of column tiles
struct head_geometry { uint32_t lg, nt; };
head_geometry head_geometry_for(uint32_t dh, bool vec) {
    const uint32_t units = vec ? dh / 4 : dh;                   // lane slots one head-row needs
    const uint32_t lg = std::min(ceil_log2(units), 6u);
    return {lg, (units + (1u << lg) - 1) >> lg};
}

void require_heads(uint32_t K, uint32_t dh) {
    MGGCN_REQUIRE(K >= 1 && K <= MGGCN_GAT_MAX_HEADS, "gat supports 1 <= heads <= 16");
    MGGCN_REQUIRE(dh >= 1 && (size_t)K * dh <= MGGCN_GAT_MAX_WIDTH, "gat supports 1 <= heads * width per head <= 1024");
}

bool rows16(const float *p, size_t ld) { return aligned16(p) && ld % 4 == 0; }
// the same rule counted in elements for a bf16 image: four columns are 8 bytes there
[[maybe_unused]] bool rows16(const uint16_t *p, size_t ld) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0 && ld % 4 == 0; }

// (VEC, NT, U) from the path and the tile count: vec needs <= 4 tiles (dh <= 1024), the element path <= 16.  f gets the
// variant as a tag; with_flag hands a run-time flag (DROP, REC) on as a std::bool_constant.
template <int VEC_, int NT_, int U_>
struct gat_variant { static constexpr int VEC = VEC_, NT = NT_, U = U_; };
template <class F>
void gat_dispatch(bool vec, uint32_t nt, F f) {
    if (vec) {
        if (nt == 1) f(gat_variant<4, 1, 4>{});
        else f(gat_variant<4, 4, 1>{});
    } else {
        if (nt == 1) f(gat_variant<1, 1, 4>{});
        else if (nt <= 4) f(gat_variant<1, 4, 2>{});
        else f(gat_variant<1, 16, 1>{});
    }
}
template <class F>
void with_flag(bool flag, F f) {
    if (flag) f(std::true_type{});
    else f(std::false_type{});
}

// one wave per row, four rows per workgroup (MGGCN_GAT_WAVE_ROW)
template <class... P, class... A>
void launch_rows(void (*kernel)(P...), size_t n_rows, mggcn_stream_t stream, A... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, as_stream(stream), args...);
    MGGCN_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------
// The column sums behind G_att: out[side][c] = sum over r < term.rows(side) of the term at (side, r, c), which `term` adds as
// acc = term(side, r, c, term.head(c), acc).  A workgroup walks rows blockIdx * R + rr, + gridDim * R, ... (R = 256 / tpr rows
// at a time, tpr threads per row), folds its R row slots in LDS in slot order and stores one [SIDES x width] partial;
// colsum_final_kernel (reduce.h) adds the partials in workgroup order.
// ---------------------------------------------------------------------------
template <int SIDES, class Term>
__global__ __launch_bounds__(256) void gat_colsum_partial_kernel(Term term, uint32_t width, uint32_t tl,
                                                                 float *__restrict__ partials) {
    __shared__ float red[256];
    const uint32_t tpr = 1u << tl, R = 256u >> tl, rr = threadIdx.x >> tl, cc = threadIdx.x & (tpr - 1);
#pragma unroll
    for (int side = 0; side < SIDES; side++) {
        const size_t n = term.rows(side);
        for (uint32_t c0 = 0; c0 < width; c0 += tpr) {      // every thread of the block takes every turn (barriers)
            const uint32_t c = c0 + cc;
            const bool on = c < width;
            const uint32_t k = on ? term.head(c) : 0;
            float acc = 0.f;
            if (on)
                for (size_t r = (size_t)blockIdx.x * R + rr; r < n; r += (size_t)gridDim.x * R) acc = term(side, r, c, k, acc);
            red[threadIdx.x] = acc;
            __syncthreads();
            if (rr == 0 && on) {
                float s = red[cc];
                for (uint32_t q = 1; q < R; q++) s += red[q * tpr + cc];
                partials[((size_t)blockIdx.x * SIDES + side) * width + c] = s;
            }
            __syncthreads();
        }
    }
}

// G_att [SIDES x width] from the partials of at most kGatColsumBlocks workgroups; n = the most rows of a side
template <int SIDES, class Term>
void gat_column_sums(mggcn_stream_t stream, const Term &term, size_t n, uint32_t width, float *G_att) {
    const hipStream_t st = as_stream(stream);
    unsigned grid = 0;
    float *partials = nullptr;
    if (n) {
        const uint32_t tl = std::min(ceil_log2(width), 8u);            // threads per row: the power of two covering the width, <= 256
        const size_t R = 256u >> tl;
        grid = (unsigned)std::min<size_t>((n + R - 1) / R, kGatColsumBlocks);
        partials = stream_scratch(st, scratch_kind::colsums, (size_t)kGatColsumBlocks * SIDES * width);
        hipLaunchKernelGGL((gat_colsum_partial_kernel<SIDES, Term>), dim3(grid), dim3(256), 0, st, term, width, tl, partials);
        MGGCN_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(colsum_final_kernel, dim3((SIDES * width + 63) / 64), dim3(256), 0, st, partials, grid, SIDES * width, G_att,
                       G_att + (SIDES - 1) * width, width);
    MGGCN_CHECK_LAUNCH();
}

}  // namespace
