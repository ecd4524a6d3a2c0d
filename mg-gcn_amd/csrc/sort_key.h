// sort_key.h -- the order-preserving map from an fp32 score to a u32 radix-sort key, shared by the ROC-AUC keys (roc_auc.hip)
// and the ranking metrics of the link head (link_rank.hip).  Device code only, internal linkage in each translation unit that
// includes it.  Not part of the ABI.
#pragma once

#include "common.h"

namespace {

// x = v + 0.0f (-0.0 becomes +0.0), u = bits(x), (u >> 31) ? ~u : (u | 0x80000000): monotone over every finite value and the
// infinities, equal keys exactly where a float compare says ==; a NaN lands where this map puts its bit pattern.
__device__ __forceinline__ uint32_t sortable_key(float v) {
    const uint32_t u = __float_as_uint(v + 0.0f);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}

}  // namespace
