// edge_sample.hip -- the per-epoch edge sample of gat / sage(aggr="max"), drawn on the device (gfx950): count, scan, compact.
// An entry (destination i, source j; global vertex numbers) of a CSR pattern is kept iff
//     i == j   or   t_i == 0xFFFFFFFF   or   word 0 of Philox4x32-10((j, i, 0xC0000000, epoch), seed) < t_i,
// t the destination's threshold.  The bit is a pure function of (seed, epoch, i, j): it is never stored, count and compact
// draw it twice, and a matrix and its transpose (transposed = 1: the rows are sources, the entry's column is the destination
// and t is gathered) keep the same set of pairs -- each in its own entry order, so the two results are transposes of each
// other entry for entry.  Duplicate entries share one bit.
//   count     one wave per row: lane l tests entries l, l + 64, ... of the row, the lanes' integer counts meet in a butterfly.
//   scan      exclusive scan of the counts into n_rows + 1 words in three launches, none of which waits on another workgroup:
//             (1) every workgroup scans its 256 counts and stores the inclusive sums at out[1 + i]; (2) ONE workgroup walks
//             the last word of every 256-block in order and makes it the global sum; (3) every workgroup but the first adds
//             the word in front of its block to its other 255.  Integer sums: any order gives the same bits.
//   compact   one wave per row over 64-entry chunks: the keep bits of a chunk are a ballot, a lane's rank is the population
//             count of the lanes below it, and a running base per row carries from chunk to chunk.  Kept columns land in
//             their original order at out_indices + out_indptr[row]; a store at or beyond out_indptr[row + 1] is never issued.
// No atomics, no LDS outside the scan, no scratch; the output does not depend on the grid.
//
// The sample WITH VALUES (gcn / sage(aggr="mean") with edge_rescale=): the same keep bit, and beside the kept columns the kept
// values times a factor per DESTINATION -- one array that both sides read (scale[row] on F, gathered scale[column] on F^T), so
// the two samples hold the same pairs with the same value bits.
//   rowscale     the count kernel's walk over F with two fp32 sums riding along: S over the row's values, S' over the kept ones,
//                both lane by lane over entries l, l + 64, ... and then through one fixed butterfly; scale = S / S' (0 where
//                S' == 0, exactly 1 where every entry is kept: the two sums are then the same additions).
//   compact_val  compact, storing value * scale[destination] (one fp32 multiply; skipped for i == j when scale_self == 0).
#include <algorithm>

#include "common.h"
#include "philox.h"

namespace {

constexpr uint32_t kSampleDomain = 0xC0000000u;      // counter word 2: apart from feature dropout (row >> 32), attention
                                                     // dropout (0x80000000 | k >> 2) and the label mask (word 0 = 0xFFFFFFFF)
constexpr uint32_t kScanBlock = 256;

struct sample_draw {
    const uint32_t *__restrict__ thr;
    uint32_t row0, col0, k0, k1, epoch;
    bool transposed;

    // the row's own threshold where the rows are destinations (read once per row)
    __device__ __forceinline__ uint32_t row_threshold(size_t row) const { return transposed ? 0u : thr[row]; }

    __device__ __forceinline__ bool keep(size_t row, uint32_t c, uint32_t t_row) const {
        const uint32_t r = row0 + (uint32_t)row, g = col0 + c;
        const uint32_t i = transposed ? g : r, j = transposed ? r : g;
        const uint32_t t = transposed ? thr[c] : t_row;
        if (i == j || t == 0xFFFFFFFFu) return true;
        return philox4x32_10(j, i, kSampleDomain, epoch, k0, k1).w[0] < t;
    }
};

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off);
    return v;
}

// one wave per row, four rows per workgroup
__global__ __launch_bounds__(256) void edge_sample_count_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                                const uint32_t *__restrict__ indices, sample_draw draw,
                                                                uint32_t *__restrict__ counts) {
    const uint32_t lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (row >= n_rows) return;
    const uint32_t beg = indptr[row], end = indptr[row + 1];
    const uint32_t t_row = draw.row_threshold(row);
    uint32_t kept = 0;
    for (size_t e = (size_t)beg + lane; e < end; e += 64) kept += draw.keep(row, indices[e], t_row) ? 1u : 0u;
    kept = wave_sum_u32(kept);
    if (lane == 0) counts[row] = kept;
}

__global__ __launch_bounds__(256) void edge_sample_compact_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                                  const uint32_t *__restrict__ indices, sample_draw draw,
                                                                  const uint32_t *__restrict__ out_indptr,
                                                                  uint32_t *__restrict__ out_indices) {
    const uint32_t lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (row >= n_rows) return;
    const uint32_t beg = indptr[row], end = indptr[row + 1];
    const uint32_t t_row = draw.row_threshold(row);
    const uint64_t below = ((uint64_t)1 << lane) - 1;               // the lanes in front of mine
    size_t base = out_indptr[row];                                  // where the chunk's first kept entry goes
    const size_t out_end = out_indptr[row + 1];
    for (size_t chunk = beg; chunk < end; chunk += 64) {            // wave-uniform trip count: the ballot wants every lane
        const size_t e = chunk + lane;
        uint32_t c = 0;
        bool keep = false;
        if (e < end) {
            c = indices[e];
            keep = draw.keep(row, c, t_row);
        }
        const uint64_t bits = __ballot(keep);
        const size_t at = base + (size_t)__popcll(bits & below);
        if (keep && at < out_end) out_indices[at] = c;              // the bound holds by construction: count drew the same bits
        base += (size_t)__popcll(bits);
    }
}

__device__ __forceinline__ float wave_sum_f32(float v) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off);   // a + b == b + a: every lane ends with the same bits
    return v;
}

// the count kernel's walk over F (rows are destinations) with the row's value sums: one wave per row, four rows per workgroup
__global__ __launch_bounds__(256) void edge_sample_rowscale_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                                   const uint32_t *__restrict__ indices,
                                                                   const float *__restrict__ values, sample_draw draw,
                                                                   uint32_t *__restrict__ counts, float *__restrict__ scale) {
    const uint32_t lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (row >= n_rows) return;
    const uint32_t beg = indptr[row], end = indptr[row + 1];
    const uint32_t t_row = draw.row_threshold(row);
    uint32_t kept = 0;
    float all = 0.f, sub = 0.f;
    for (size_t e = (size_t)beg + lane; e < end; e += 64) {
        const bool keep = draw.keep(row, indices[e], t_row);
        const float v = values[e];
        kept += keep ? 1u : 0u;
        all += v;
        sub += keep ? v : 0.f;
    }
    kept = wave_sum_u32(kept);
    all = wave_sum_f32(all);
    sub = wave_sum_f32(sub);
    if (lane == 0) {
        counts[row] = kept;
        scale[row] = sub == 0.f ? 0.f : (kept == end - beg ? 1.f : all / sub);
    }
}

__global__ __launch_bounds__(256) void edge_sample_compact_val_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                                      const uint32_t *__restrict__ indices,
                                                                      const float *__restrict__ values, sample_draw draw,
                                                                      const float *__restrict__ scale, bool scale_self,
                                                                      const uint32_t *__restrict__ out_indptr,
                                                                      uint32_t *__restrict__ out_indices,
                                                                      float *__restrict__ out_values) {
    const uint32_t lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (row >= n_rows) return;
    const uint32_t beg = indptr[row], end = indptr[row + 1];
    const uint32_t t_row = draw.row_threshold(row);
    const float f_row = (scale != nullptr && !draw.transposed) ? scale[row] : 1.f;
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    size_t base = out_indptr[row];
    const size_t out_end = out_indptr[row + 1];
    for (size_t chunk = beg; chunk < end; chunk += 64) {            // wave-uniform trip count: the ballot wants every lane
        const size_t e = chunk + lane;
        uint32_t c = 0;
        float v = 0.f;
        bool keep = false;
        if (e < end) {
            c = indices[e];
            keep = draw.keep(row, c, t_row);
        }
        if (keep) {
            v = values[e];
            const bool self = draw.row0 + (uint32_t)row == draw.col0 + c;
            if (scale != nullptr && (scale_self || !self)) v *= draw.transposed ? scale[c] : f_row;
        }
        const uint64_t bits = __ballot(keep);
        const size_t at = base + (size_t)__popcll(bits & below);
        if (keep && at < out_end) {                                 // the bound holds by construction: count drew the same bits
            out_indices[at] = c;
            out_values[at] = v;
        }
        base += (size_t)__popcll(bits);
    }
}

// inclusive scan of one value per thread over the workgroup's 256 threads (four waves)
__device__ __forceinline__ uint32_t block_inclusive_scan(uint32_t v, uint32_t *wave_totals) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = __shfl_up(v, off);
        if (lane >= (uint32_t)off) v += up;
    }
    if (lane == 63) wave_totals[wave] = v;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t w = 0; w < wave; w++) before += wave_totals[w];
    __syncthreads();                                                // wave_totals may be written again by the caller's next turn
    return v + before;
}

// (1) out[1 + i] = the sum of counts[block start .. i]; out[0] = 0
__global__ __launch_bounds__(256) void edge_sample_scan_blocks_kernel(const uint32_t *__restrict__ counts, size_t n,
                                                                      uint32_t *__restrict__ out) {
    __shared__ uint32_t wave_totals[4];
    const size_t i = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    const uint32_t s = block_inclusive_scan(i < n ? counts[i] : 0u, wave_totals);
    if (i < n) out[1 + i] = s;
    if (i == 0) out[0] = 0;
}

// (2) one workgroup: the last word of every full block becomes the sum of everything up to it
__global__ __launch_bounds__(256) void edge_sample_scan_totals_kernel(size_t n, uint32_t *__restrict__ out) {
    __shared__ uint32_t wave_totals[4];
    __shared__ uint32_t carry_s;
    const size_t n_blocks = n / kScanBlock;                         // full blocks: a partial last block has no successor
    uint32_t carry = 0;
    for (size_t b0 = 0; b0 < n_blocks; b0 += kScanBlock) {
        const size_t b = b0 + threadIdx.x;
        uint32_t *p = out + (b + 1) * kScanBlock;                   // = out[1 + (last element of block b)]
        const uint32_t s = carry + block_inclusive_scan(b < n_blocks ? *p : 0u, wave_totals);
        if (b < n_blocks) *p = s;
        if (threadIdx.x == kScanBlock - 1) carry_s = s;
        __syncthreads();
        carry = carry_s;
        __syncthreads();
    }
}

// (3) every word of block b >= 1 but its last (final since (2)) takes the word in front of the block
__global__ __launch_bounds__(256) void edge_sample_scan_add_kernel(size_t n, uint32_t *__restrict__ out) {
    const size_t b = (size_t)blockIdx.x + 1;
    const size_t i = b * kScanBlock + threadIdx.x;
    if (i < n && threadIdx.x != kScanBlock - 1) out[1 + i] += out[b * kScanBlock];
}

sample_draw make_draw(const uint32_t *thr, int transposed, uint32_t row0, uint32_t col0, uint64_t seed, uint32_t epoch) {
    return {thr, row0, col0, (uint32_t)(seed & 0xFFFFFFFFull), (uint32_t)(seed >> 32), epoch, transposed != 0};
}

}  // namespace

// ============================ C ABI =========================================
MGGCN_API void mggcn_edge_sample_count_u32(mggcn_stream_t stream, uint32_t n_rows, const uint32_t *indptr,
                                           const uint32_t *indices, const uint32_t *thr, int transposed, uint32_t row0,
                                           uint32_t col0, uint64_t seed, uint32_t epoch, uint32_t *counts) {
    MGGCN_REQUIRE(transposed == 0 || transposed == 1, "edge sample count: transposed must be 0 or 1");
    if (!n_rows) return;
    MGGCN_REQUIRE(indptr != nullptr && thr != nullptr && counts != nullptr, "edge sample count: null operand");
    hipLaunchKernelGGL(edge_sample_count_kernel, dim3((unsigned)(((size_t)n_rows + 3) / 4)), dim3(256), 0, as_stream(stream), n_rows, indptr,
                       indices, make_draw(thr, transposed, row0, col0, seed, epoch), counts);
    MGGCN_CHECK_LAUNCH();
}

MGGCN_API void mggcn_edge_sample_scan_u32(mggcn_stream_t stream, const uint32_t *counts, size_t n_rows, uint32_t *out_indptr) {
    MGGCN_REQUIRE(out_indptr != nullptr, "edge sample scan: null operand");
    MGGCN_REQUIRE(n_rows == 0 || counts != nullptr, "edge sample scan: null operand");
    MGGCN_REQUIRE(n_rows < ((size_t)1 << 32), "edge sample scan: at most 2^32 - 1 rows");
    const hipStream_t st = as_stream(stream);
    const size_t blocks = (n_rows + kScanBlock - 1) / kScanBlock;
    hipLaunchKernelGGL(edge_sample_scan_blocks_kernel, dim3((unsigned)std::max<size_t>(blocks, 1)), dim3(kScanBlock), 0, st,
                       counts, n_rows, out_indptr);
    MGGCN_CHECK_LAUNCH();
    if (blocks < 2) return;
    hipLaunchKernelGGL(edge_sample_scan_totals_kernel, dim3(1), dim3(kScanBlock), 0, st, n_rows, out_indptr);
    MGGCN_CHECK_LAUNCH();
    hipLaunchKernelGGL(edge_sample_scan_add_kernel, dim3((unsigned)(blocks - 1)), dim3(kScanBlock), 0, st, n_rows, out_indptr);
    MGGCN_CHECK_LAUNCH();
}

MGGCN_API void mggcn_edge_sample_compact_u32(mggcn_stream_t stream, uint32_t n_rows, const uint32_t *indptr,
                                             const uint32_t *indices, const uint32_t *thr, int transposed, uint32_t row0,
                                             uint32_t col0, uint64_t seed, uint32_t epoch, const uint32_t *out_indptr,
                                             uint32_t *out_indices) {
    MGGCN_REQUIRE(transposed == 0 || transposed == 1, "edge sample compact: transposed must be 0 or 1");
    if (!n_rows) return;
    MGGCN_REQUIRE(indptr != nullptr && thr != nullptr && out_indptr != nullptr, "edge sample compact: null operand");
    MGGCN_REQUIRE((const void *)out_indices != (const void *)indices || indices == nullptr,
                  "edge sample compact: out_indices must not alias indices");
    hipLaunchKernelGGL(edge_sample_compact_kernel, dim3((unsigned)(((size_t)n_rows + 3) / 4)), dim3(256), 0, as_stream(stream), n_rows, indptr,
                       indices, make_draw(thr, transposed, row0, col0, seed, epoch), out_indptr, out_indices);
    MGGCN_CHECK_LAUNCH();
}

MGGCN_API void mggcn_edge_sample_rowscale_f32(mggcn_stream_t stream, uint32_t n_rows, const uint32_t *indptr,
                                              const uint32_t *indices, const float *values, const uint32_t *thr, uint32_t row0,
                                              uint32_t col0, uint64_t seed, uint32_t epoch, uint32_t *counts, float *scale) {
    if (!n_rows) return;
    MGGCN_REQUIRE(indptr != nullptr && thr != nullptr && counts != nullptr && scale != nullptr, "edge sample rowscale: null operand");
    hipLaunchKernelGGL(edge_sample_rowscale_kernel, dim3((unsigned)(((size_t)n_rows + 3) / 4)), dim3(256), 0, as_stream(stream), n_rows,
                       indptr, indices, values, make_draw(thr, 0, row0, col0, seed, epoch), counts, scale);
    MGGCN_CHECK_LAUNCH();
}

MGGCN_API void mggcn_edge_sample_compact_val_f32(mggcn_stream_t stream, uint32_t n_rows, const uint32_t *indptr,
                                                 const uint32_t *indices, const float *values, const uint32_t *thr, int transposed,
                                                 uint32_t row0, uint32_t col0, uint64_t seed, uint32_t epoch, const float *scale,
                                                 int scale_self, const uint32_t *out_indptr, uint32_t *out_indices,
                                                 float *out_values) {
    MGGCN_REQUIRE(transposed == 0 || transposed == 1, "edge sample compact: transposed must be 0 or 1");
    if (!n_rows) return;
    MGGCN_REQUIRE(indptr != nullptr && thr != nullptr && out_indptr != nullptr, "edge sample compact: null operand");
    MGGCN_REQUIRE((const void *)out_indices != (const void *)indices || indices == nullptr,
                  "edge sample compact: out_indices must not alias indices");
    MGGCN_REQUIRE((const void *)out_values != (const void *)values || values == nullptr,
                  "edge sample compact: out_values must not alias values");
    hipLaunchKernelGGL(edge_sample_compact_val_kernel, dim3((unsigned)(((size_t)n_rows + 3) / 4)), dim3(256), 0, as_stream(stream),
                       n_rows, indptr, indices, values, make_draw(thr, transposed, row0, col0, seed, epoch), scale, scale_self != 0,
                       out_indptr, out_indices, out_values);
    MGGCN_CHECK_LAUNCH();
}
