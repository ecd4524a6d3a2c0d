// scratch_internal.h -- the per-(device, stream) scratch for per-workgroup column-sum partials, shared between
// elementwise.hip (which owns it: mggcn_layer_norm_backward_f32) and gat.hip.  Not part of the ABI.
#pragma once

#include "common.h"

// At least `floats` floats of device memory that belong to (the current device, st): grown on first use (never on a captured
// launch path; growing synchronises st), freed by mggcn_stream_release_scratch.  Kernels enqueued on st use it one after
// the other.
float *colsum_scratch(hipStream_t st, size_t floats);
