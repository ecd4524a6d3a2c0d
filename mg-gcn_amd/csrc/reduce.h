// reduce.h -- the fixed-order reduction tree of every reproducible sum ("the reduction tree"): device code only,
// internal linkage in each translation unit that includes it (elementwise.hip, gat.hip).  Not part of the ABI.
//
//   wave      wave_sum / wave_max (xor butterfly) or the DPP family -- a kernel keeps the flavour it has: the two add in
//             different orders
//   workgroup block_fold: four waves through LDS, (w0 + w1) + (w2 + w3), one partial per workgroup
//   grid      sums_final_kernel / colsum_final_kernel: the partials in workgroup order; segsum_final_kernel: one such sum
//             per segment of a list, the partials in chunk order
//
// A kernel that needs such a sum calls these and never writes the tree out.
#pragma once

#include <type_traits>

#include "common.h"

namespace {

// ---- wave level: xor butterfly (every lane ends with the same bits) -------
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// ---- wave level: DPP -------------------------------------------------------
// Wave-wide reductions on the DPP path (no LDS): four in-row steps (quad swaps, half-row and row mirrors) leave every
// lane of a 16-lane row with its row's result, four v_readlane bring the row results together.  hipcc lowers
// __shfl_xor to ds_bpermute_b32, an LDS-crossbar instruction: the fused loss kernel spent its time there (~30 per row).
template <typename Op>
__device__ __forceinline__ float wave_reduce_dpp(float v, Op op) {
    auto dpp = [](float x, auto ctrl) {
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), decltype(ctrl)::value, 0xF, 0xF, true));
    };
    v = op(v, dpp(v, std::integral_constant<int, 0xB1>{}));     // quad_perm [1,0,3,2]
    v = op(v, dpp(v, std::integral_constant<int, 0x4E>{}));     // quad_perm [2,3,0,1]
    v = op(v, dpp(v, std::integral_constant<int, 0x141>{}));    // row_half_mirror
    v = op(v, dpp(v, std::integral_constant<int, 0x140>{}));    // row_mirror
    // (the builtin is typed int: a float argument would be CONVERTED, not re-interpreted)
    auto lane_f = [](float x, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), l)); };
    const float r0 = lane_f(v, 0), r1 = lane_f(v, 16), r2 = lane_f(v, 32), r3 = lane_f(v, 48);
    return op(op(r0, r1), op(r2, r3));
}
__device__ __forceinline__ float wave_sum_dpp(float v) { return wave_reduce_dpp(v, [](float a, float b) { return a + b; }); }
__device__ __forceinline__ float wave_max_dpp(float v) { return wave_reduce_dpp(v, [](float a, float b) { return fmaxf(a, b); }); }

// One row per 16-LANE GROUP: every reduction is four DPP rotations inside the 16-lane row (row_ror 8, 4, 2, 1: a butterfly
// -- both lanes of a pair add the same two numbers, so all 16 lanes end with the same bits), no v_readlane, no cross-row
// step.
template <typename T, typename Op>
__device__ __forceinline__ T row16_reduce(T v, Op op) {
    auto ror = [](T x, auto ctrl) {
        return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), decltype(ctrl)::value, 0xF, 0xF, true));
    };
    v = op(v, ror(v, std::integral_constant<int, 0x128>{}));    // row_ror:8
    v = op(v, ror(v, std::integral_constant<int, 0x124>{}));    // row_ror:4
    v = op(v, ror(v, std::integral_constant<int, 0x122>{}));    // row_ror:2
    v = op(v, ror(v, std::integral_constant<int, 0x121>{}));    // row_ror:1
    return v;
}

// ---- workgroup level -------------------------------------------------------
// The end of a kernel of four waves: v[j] is wave-reduced (lane 0 of each wave holds the wave's value), lds is [NV][4]
// shared floats of the caller, and thread j < NV leaves out[j] = (w0 + w1) + (w2 + w3) of value j (Add: added to what
// out[j] holds).  Which thread does the last addition does not touch the bits; the expression does.  Holds one
// __syncthreads(): every thread of the workgroup calls it.
template <int NV, bool Add = false>
__device__ __forceinline__ void block_fold(const float (&v)[NV], float (*lds)[4], float *out) {
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < NV; j++) lds[j][threadIdx.x >> 6] = v[j];
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        const float t = (lds[threadIdx.x][0] + lds[threadIdx.x][1]) + (lds[threadIdx.x][2] + lds[threadIdx.x][3]);
        out[threadIdx.x] = Add ? out[threadIdx.x] + t : t;
    }
}

// ---- grid level: scalars ----------------------------------------------------
// sums[j] (+)= the workgroups' partials [n_blocks][NV], each of the NV values summed on its own in a fixed order: thread t
// adds workgroups t, t + 256, ..., then the tree above.  One workgroup.  (First version of the loss: two float atomics per
// workgroup on the same two addresses -- 4096 device-scope read-modify-writes in a row were most of the pass, and the two
// scalars depended on arrival order in their last bits.)
// NV = 1 store: |x| sum; 2 add: the fused loss's (loss, correct); 4 store: |x| sums by set; 8 add: the split-aware loss's
// pair per slot; 16 add: the sigmoid-BCE loss's (loss, TP, FP, FN) per slot.
template <int NV, bool Add>
__global__ __launch_bounds__(256) void sums_final_kernel(const float *__restrict__ partials, unsigned n_blocks,
                                                         float *__restrict__ sums) {
    __shared__ float w[NV][4];
    float v[NV];
#pragma unroll
    for (int j = 0; j < NV; j++) v[j] = 0.f;
    for (unsigned i = threadIdx.x; i < n_blocks; i += 256) {
#pragma unroll
        for (int j = 0; j < NV; j++) v[j] += partials[NV * i + j];
    }
#pragma unroll
    for (int j = 0; j < NV; j++) v[j] = wave_sum(v[j]);
    block_fold<NV, Add>(v, w, sums);
}

// ---- grid level: columns ----------------------------------------------------
// out[idx] = the workgroups' partials [n_blocks][width] added in a fixed order: 64 of the `width` sums per workgroup, each
// from four slices (workgroups b, b + 4, ... in order) that meet in LDS.  idx < split lands in out_lo[idx], the rest in
// out_hi[idx - split] (the two need not be adjacent).  n_blocks == 0 stores zeros.
[[maybe_unused]]        // label_input.hip sums by segment instead
__global__ __launch_bounds__(256) void colsum_final_kernel(const float *__restrict__ partials, unsigned n_blocks,
                                                           uint32_t width, float *__restrict__ out_lo,
                                                           float *__restrict__ out_hi, uint32_t split) {
    __shared__ float w[4][64];
    const uint32_t lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const uint32_t idx = blockIdx.x * 64 + lane;
    float s = 0.f;
    if (idx < width) {
#pragma unroll 8
        for (unsigned b = slice; b < n_blocks; b += 4) s += partials[(size_t)b * width + idx];
    }
    w[slice][lane] = s;
    __syncthreads();
    if (slice == 0 && idx < width) {
        const float t = (w[0][lane] + w[1][lane]) + (w[2][lane] + w[3][lane]);
        if (idx < split) out_lo[idx] = t;
        else out_hi[idx - split] = t;
    }
}

// ---- grid level: columns, by segment -----------------------------------------
// out[s][idx] = the partials of segment s added in a fixed order, for a sum whose rows are a list cut into segments
// (seg_ptr[s] .. seg_ptr[s + 1], the list n_list long) and whose producer stored one [width] partial per chunk of Chunk
// list entries of a segment: chunk q of segment s at row seg_ptr[s] / Chunk + s + q of `partials` (the rows of a segment
// end before the next segment's begin).  The tree is colsum_final_kernel's: four slices (chunks q, q + 4, ... in order)
// that meet in LDS.  Grid (width / 64 rounded up, segments); a segment without an entry, and every segment when
// n_list == 0 (seg_ptr is not read then), stores +0.0.  A template, so that only its user carries it.
template <unsigned Chunk>
__global__ __launch_bounds__(256) void segsum_final_kernel(const float *__restrict__ partials,
                                                           const uint32_t *__restrict__ seg_ptr, uint32_t n_list,
                                                           uint32_t width, float *__restrict__ out, size_t ldo) {
    __shared__ float w[4][64];
    const uint32_t lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const uint32_t idx = blockIdx.x * 64 + lane, seg = blockIdx.y;
    uint32_t first = 0, chunks = 0;
    if (n_list) {
        const uint32_t lo = seg_ptr[seg], hi = seg_ptr[seg + 1] < n_list ? seg_ptr[seg + 1] : n_list;
        first = lo / Chunk + seg;
        chunks = hi > lo ? (hi - lo + Chunk - 1) / Chunk : 0;
    }
    float s = 0.f;
    if (idx < width) {
#pragma unroll 8
        for (uint32_t q = slice; q < chunks; q += 4) s += partials[(size_t)(first + q) * width + idx];
    }
    w[slice][lane] = s;
    __syncthreads();
    if (slice == 0 && idx < width) out[(size_t)seg * ldo + idx] = (w[0][lane] + w[1][lane]) + (w[2][lane] + w[3][lane]);
}

}  // namespace
