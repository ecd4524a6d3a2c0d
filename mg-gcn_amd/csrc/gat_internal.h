// gat_internal.h -- what the graph attention kernels of gat.hip (GAT) and gatv2.hip (GATv2) share: the one-wave-per-row
// layout with LPR-lane groups (gat.hip describes it), the group butterfly, the head-row loads, the head geometry and the
// (VEC, NT, U) dispatch.  Internal linkage in each translation unit that includes it.  Not part of the ABI.
#pragma once

#include <algorithm>

#include "common.h"

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

// the head-row of `row` (NT tiles of VEC columns per lane), zeros beyond dh
template <int VEC, int NT>
__device__ __forceinline__ void load_head_row(float (&r)[NT][VEC], const float *p, uint32_t lpr, uint32_t sub, uint32_t dh,
                                              bool on = true) {
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const uint32_t col = (t * lpr + sub) * VEC;
        if (on && col < dh) loadv<VEC>(r[t], p + col);
        else zerov<VEC>(r[t]);
    }
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

// (VEC, NT, U) from the path and the tile count: vec needs <= 4 tiles (dh <= 1024), the element path <= 16
#define MGGCN_GAT_DISPATCH(F, vec, nt)        \
    do {                                      \
        if (vec) {                            \
            if ((nt) == 1) F(4, 1, 4);        \
            else F(4, 4, 1);                  \
        } else {                              \
            if ((nt) == 1) F(1, 1, 4);        \
            else if ((nt) <= 4) F(1, 4, 2);   \
            else F(1, 16, 1);                 \
        }                                     \
    } while (0)

}  // namespace
