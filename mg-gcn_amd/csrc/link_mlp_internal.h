// link_mlp_internal.h -- what the two MLP decoders of the link head share (link_mlp.hip on the fp32 matrix instruction,
// link_mlp_b16.hip on the bf16 one): the C layout of a 32 x 32 accumulator tile, the half-wave folds, the grid caps that fix
// the order of the sums, the shape checks and the (DB, HB) dispatch.  Internal linkage in each translation unit that includes
// it.  Not part of the ABI.
#pragma once

#include <type_traits>

#include "gat_internal.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr float kLinkMlpSlope = 0.01f;                  // the leaky ReLU of every gcn layer (elementwise.hip)
constexpr unsigned kLinkMlpWalkGrid = kNumCU * 2;       // workgroups of the walk: two fit a CU's LDS at 128 x 128
constexpr unsigned kLinkMlpPairsGrid = kNumCU;          // workgroups of the pairs kernel = rows of its partials

// Nothing is scheduled across it.  Left to itself the scheduler hoists the LDS reads of a whole unrolled product (up to 256
// A operands) in front of its first MFMA and spills the accumulators to make room for them.
#define MLP_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)

// the row of the C layout that register r of lane half h holds
__device__ __forceinline__ constexpr int c_row(int r, int h) { return 8 * (r >> 2) + 4 * h + (r & 3); }

// sum over the 32 lanes of a half wave, the same bits on all of them: a butterfly inside each row of 16, then the rows
__device__ __forceinline__ float half_sum(float v) {
    v = row16_reduce(v, [](float a, float b) { return a + b; });
    return v + __shfl_xor(v, 16);
}
__device__ __forceinline__ uint32_t half_sum_u32(uint32_t v) {
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) v += (uint32_t)__shfl_xor((int)v, off);
    return v;
}

__device__ __forceinline__ void load4(float (&r)[4], const float *p, bool vec) {
    if (vec) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w;
    } else {
        r[0] = p[0]; r[1] = p[1]; r[2] = p[2]; r[3] = p[3];
    }
}

[[maybe_unused]] bool overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a_bytes && b_bytes && x < y + b_bytes && y < x + a_bytes;
}
// of an fp32 matrix; an image of 2-byte elements passes elem = 2
[[maybe_unused]] size_t matrix_bytes(size_t rows, size_t ld, size_t d, size_t elem = sizeof(float)) {
    return rows ? ((rows - 1) * ld + d) * elem : 0;
}

[[maybe_unused]] void require_mlp_shape(uint32_t d, uint32_t hd) {
    MGGCN_REQUIRE(d >= 32 && d <= MGGCN_LINK_MLP_MAX_WIDTH && d % 32 == 0, "link mlp: d must be a multiple of 32 in [32, 128]");
    MGGCN_REQUIRE(hd >= 32 && hd <= MGGCN_LINK_MLP_MAX_WIDTH && hd % 32 == 0, "link mlp: hd must be a multiple of 32 in [32, 128]");
}

// f(std::integral_constant DB, HB)
template <class F>
void mlp_dispatch(uint32_t d, uint32_t hd, F f) {
    const auto by_hb = [&](auto db) {
        switch (hd / 32) {
        case 1: f(db, std::integral_constant<int, 1>{}); break;
        case 2: f(db, std::integral_constant<int, 2>{}); break;
        case 3: f(db, std::integral_constant<int, 3>{}); break;
        default: f(db, std::integral_constant<int, 4>{}); break;
        }
    };
    switch (d / 32) {
    case 1: by_hb(std::integral_constant<int, 1>{}); break;
    case 2: by_hb(std::integral_constant<int, 2>{}); break;
    case 3: by_hb(std::integral_constant<int, 3>{}); break;
    default: by_hb(std::integral_constant<int, 4>{}); break;
    }
}

}  // namespace
