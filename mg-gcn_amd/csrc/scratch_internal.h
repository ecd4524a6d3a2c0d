// scratch_internal.h -- the per-(device, stream) scratch for per-workgroup partials of the reduction tree (reduce.h), owned
// by runtime.hip and used by elementwise.hip, gat.hip and gated_skip.hip.  Not part of the ABI.
#pragma once

#include "common.h"

// sums: the scalar partials ([workgroup][value]) of a kernel that ends in block_fold, always asked for at one size;
// colsums: the column partials ([workgroup][width]) of the layer norm's, the GAT's and the gated skip's backward, which grow
// with the width.
// Two buffers, so that a wider column sum never moves the scalars' buffer.
enum class scratch_kind { sums, colsums };

// At least `floats` floats of device memory that belong to (the current device, st, kind): grown on first use (never on a
// captured launch path; growing synchronises st), freed by mggcn_stream_release_scratch.  Per STREAM, not per device:
// several contexts may drive one GPU at once (a dist_context whose ranks share a device, two models on two streams) and
// two sums in flight on different streams must not share their partials.  Kernels enqueued on st use it one after the
// other.
float *stream_scratch(hipStream_t st, scratch_kind kind, size_t floats);

// The sums kind holds kSumsPerBlockMax values for each workgroup of a grid of kSumsGridMax at the most; a launcher states
// what it writes (values per workgroup, grid cap) and gets the buffer.
constexpr unsigned kSumsPerBlockMax = 16;
constexpr unsigned kSumsGridMax = kNumCU * 8;          // the cap of stream_grid
template <unsigned PerBlock, unsigned GridCap>
float *sums_scratch(hipStream_t st) {
    static_assert(PerBlock <= kSumsPerBlockMax && GridCap <= kSumsGridMax, "more partials than the sums scratch holds");
    return stream_scratch(st, scratch_kind::sums, (size_t)kSumsPerBlockMax * kSumsGridMax);
}
