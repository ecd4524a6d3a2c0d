// philox.h -- the counter-based generator behind every mask that is never stored: mggcn_dropout_f32 (elementwise.hip) and
// the attention dropout of the mggcn_gat_*_drop_f32 kernels (gat.hip) share this one definition.
// Philox4x32-10 (Salmon et al., SC'11): multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten
// rounds.  The 32 x 32 -> 64 products are written as one 64-bit multiply each (v_mad_u64_u32: both halves from one instruction).
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

struct philox4 { uint32_t w[4]; };

__device__ __forceinline__ philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; round++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return {{c0, c1, c2, c3}};
}
