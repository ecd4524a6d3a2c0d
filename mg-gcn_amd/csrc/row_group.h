// row_group.h -- one dense row per group of L lanes: the register layout, the row walk, the grid and the dispatch that the
// layer norm pair (elementwise.hip) and the gated skip pair (gated_skip.hip) share.  Device code and launch helpers with
// internal linkage in each translation unit that includes it.  Not part of the ABI.
//
// A row of m <= 1024 columns lives in the registers of L = 16 or 64 lanes: lane `sub` of the group holds the K units
// sub + L * k (k < K) of V floats each (V = 4: float4 loads, m % 4 == 0 and 16-byte aligned operands; V = 1: any width and
// alignment), i.e. columns (sub + L * k) * V + v.  The mapping depends on (V, L, K) alone, which the host picks from m and
// the alignment, never on where the row sits in the grid: a row gives the same bits alone, in a shard or in the whole
// matrix.  With L = 16 a wave works on four rows at once (the 16-lane-row form of the fused loss: every reduction is four
// DPP rotations inside the row); with L = 64, R = 2 rows are in flight where the registers allow it.  All loads of a pass
// are issued before the first reduction, so x may be y and G_in may be G or act: a row is read whole before any of it is
// written.  Both sums of a pass are butterflies: every lane of a group ends with the same bits.
#pragma once

#include <algorithm>

#include "common.h"
#include "reduce.h"

namespace {

constexpr unsigned kLayerNormBlocks = kNumCU * 4;          // grid cap of both passes: four workgroups of four waves per CU

template <int L>
__device__ __forceinline__ float ln_group_sum(float v) {
    if constexpr (L == 16) return row16_reduce(v, [](float a, float b) { return a + b; });
    else return wave_sum_dpp(v);
}

template <int V>
__device__ __forceinline__ void ln_load(float *dst, const float *p, bool ok, float fill) {
    if constexpr (V == 4) {
        const float4 t = ok ? *reinterpret_cast<const float4 *>(p) : make_float4(fill, fill, fill, fill);
        dst[0] = t.x; dst[1] = t.y; dst[2] = t.z; dst[3] = t.w;
    } else {
        dst[0] = ok ? *p : fill;
    }
}

template <int V>
__device__ __forceinline__ void ln_store(float *p, const float *src) {
    if constexpr (V == 4) *reinterpret_cast<float4 *>(p) = make_float4(src[0], src[1], src[2], src[3]);
    else *p = src[0];
}

// where group `sub`-lane of this thread starts and how the grid walks the rows (wave-uniform trip count: the DPP steps
// want every lane of a row group in step)
template <int L>
struct ln_walk {
    uint32_t sub;
    size_t g0, w0, gstride;
    __device__ ln_walk() {
        sub = threadIdx.x & (L - 1);
        gstride = ((size_t)gridDim.x * blockDim.x) / L;
        g0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / L;
        w0 = ((size_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u)) / L;       // first group of this wave
    }
};

template <int L, int R>
unsigned layer_norm_grid(size_t n_rows) {
    const size_t per_block = (size_t)(256 / L) * R;
    return (unsigned)std::min<size_t>((n_rows + per_block - 1) / per_block, kLayerNormBlocks);
}

// (V, L, K, R) from the width and the alignment; F(V, L, K, R) launches
#define MGGCN_LN_DISPATCH(F, vec, m)                                          \
    do {                                                                      \
        if (vec) {                                                            \
            const size_t q_ = (m) / 4;                                        \
            if (q_ <= 16) F(4, 16, 1, 1);                                     \
            else if (q_ <= 32) F(4, 16, 2, 1);                                \
            else if (q_ <= 64) F(4, 16, 4, 1);                                \
            else if (q_ <= 128) F(4, 64, 2, 2);                               \
            else F(4, 64, 4, 1);                                              \
        } else {                                                              \
            if ((m) <= 16) F(1, 16, 1, 1);                                    \
            else if ((m) <= 32) F(1, 16, 2, 1);                               \
            else if ((m) <= 48) F(1, 16, 3, 1);                               \
            else if ((m) <= 64) F(1, 16, 4, 1);                               \
            else if ((m) <= 128) F(1, 64, 2, 2);                              \
            else if ((m) <= 256) F(1, 64, 4, 2);                              \
            else if ((m) <= 512) F(1, 64, 8, 1);                              \
            else F(1, 64, 16, 1);                                             \
        }                                                                     \
    } while (0)

}  // namespace
