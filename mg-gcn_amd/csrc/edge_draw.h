// edge_draw.h -- the one draw of the per-epoch edge sample, shared by edge_sample.hip (the keep bit of count / compact /
// rowscale / compact_val) and edge_select.hip (the per-row threshold of the exact fan-out): entry (destination i, source j),
// global vertex numbers, draws word 0 of Philox4x32-10((j, i, 0xC0000000, epoch), seed) and is kept iff
//     i == j   or   t_i == 0xFFFFFFFF   or   that word < t_i.
#pragma once

#include "philox.h"

constexpr uint32_t kSampleDomain = 0xC0000000u;      // counter word 2: apart from feature dropout (row >> 32), attention
                                                     // dropout (0x80000000 | k >> 2) and the label mask (word 0 = 0xFFFFFFFF)

constexpr uint32_t kLinkDomain = 0xE0000000u;        // counter word 2 of the link head's negatives (link.hip): apart from all
                                                     // of the above and from kSampleDomain; word 0 is an entry position
                                                     // p < 2^31, which the label mask's 0xFFFFFFFF never is

// Negative (p, r) of the link head: the tail of the entry at position p, r < R.  Word r & 3 of
// Philox4x32-10((p, r >> 2, kLinkDomain, epoch), seed) mapped onto [0, n) by the high half of a 32 x 32 product.
// link_negative is one of them on its own; link_negatives keeps the four words of one call: next(r) for r = 0, 1, ... in
// order draws again at every fourth.  Both pick their word where the four live: a shared function that took the four, by
// reference or by value, moved the register allocation of every MLP walk kernel (link_mlp*.hip), which has none to spare.
__device__ __forceinline__ uint32_t link_tail(uint32_t word, uint32_t n) { return (uint32_t)(((uint64_t)word * n) >> 32); }
__device__ __forceinline__ uint32_t link_negative(uint32_t p, uint32_t r, uint32_t n, uint32_t epoch, uint32_t k0, uint32_t k1) {
    const philox4 wd = philox4x32_10(p, r >> 2, kLinkDomain, epoch, k0, k1);
    const uint32_t q = r & 3;
    return link_tail(q == 0 ? wd.w[0] : q == 1 ? wd.w[1] : q == 2 ? wd.w[2] : wd.w[3], n);
}
struct link_negatives {
    uint32_t p, n, k0, k1, epoch;
    philox4 w;
    __device__ __forceinline__ uint32_t next(uint32_t r) {
        if ((r & 3) == 0) w = philox4x32_10(p, r >> 2, kLinkDomain, epoch, k0, k1);
        const uint32_t q = r & 3;
        return link_tail(q == 0 ? w.w[0] : q == 1 ? w.w[1] : q == 2 ? w.w[2] : w.w[3], n);
    }
};

__device__ __forceinline__ uint32_t sample_word(uint32_t i, uint32_t j, uint32_t epoch, uint32_t k0, uint32_t k1) {
    return philox4x32_10(j, i, kSampleDomain, epoch, k0, k1).w[0];
}

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
        return sample_word(i, j, epoch, k0, k1) < t;
    }
};
