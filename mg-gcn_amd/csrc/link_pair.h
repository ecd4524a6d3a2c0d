// link_pair.h -- what one pair of the link head adds to the loss, shared by the dot decoder (link.hip) and the MLP decoder
// (link_mlp.hip): both score a pair their own way and hand the score to the same binary cross-entropy.  Device code only,
// internal linkage in each translation unit that includes it.  Not part of the ABI.
#pragma once

#include "common.h"

namespace {

// what one pair adds: g = dL/ds times the pair's weight, its loss term, whether s falls on the label's side of 0.
// e = exp(-|s|) serves log1p and both sigmoids; sigma(s) - 1 is formed as -sigma(-s), which does not cancel.
struct pair_terms { float g, loss; uint32_t hit; };
__device__ __forceinline__ pair_terms link_pair(float s, bool positive, float weight) {
    const float e = expf(-fabsf(s)), l1p = log1pf(e), inv = 1.f / (1.f + e);
    const float sig_abs = inv, sig_neg = e * inv;               // sigma(|s|), sigma(-|s|)
    if (positive) return {-(s >= 0.f ? sig_neg : sig_abs) * weight, fmaxf(-s, 0.f) + l1p, s > 0.f ? 1u : 0u};
    return {(s >= 0.f ? sig_abs : sig_neg) * weight, fmaxf(s, 0.f) + l1p, s > 0.f ? 0u : 1u};
}

}  // namespace
