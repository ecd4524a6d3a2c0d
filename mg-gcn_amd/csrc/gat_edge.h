// gat_edge.h -- the edge term of the GAT score (PyG's GATConv(edge_dim = de) with lin_edge and att_edge folded into one
// [K x de] matrix U = att_edge):
//   t_pk = fmaf(E[p, de - 1], U[k, de - 1], ... fmaf(E[p, 0], U[k, 0], 0.f)),   x_ijk = (s_dst[i, k] + s_src[j, k]) + t_pk
// for entry p = (i, j) of the CSR a kernel walks.  The three kernels of gat_kernels.h take it as a compile-time option: an
// instantiation with a gat_edge parameter (gat_efeat.hip) adds t to x, one without (gat.hip, gat_b16.hip) has no trace of it.
//   * The edge term belongs to a POSITION, not to an index: the lane that owns entry l of a chunk owns row base + l of E.  The
//     walk (entry_chunks of gat_internal.h) calls its fetch for exactly one position per call -- beg + lane from start(),
//     base + 64 + lane from next() -- so the fetch reads that position from a variable the kernel sets before the call
//     (`pos`) and t rides as one more scalar of the walk, loaded and folded one chunk ahead like s_src.
//   * U[k, :] is wave-uniform per head and read through a uniform pointer; a row of E is read with 16-byte loads when
//     de % 4 == 0 and base and lde are aligned for them (a run-time, wave-uniform choice), element by element otherwise.
//     Both paths run the one fmaf chain, c ascending, so forward over F, backward_dst over F and backward_src over F^T give
//     an edge the same x, and so the same alpha, whichever copy of E they read.
//   * P_e[i, k de + c] = sum_j ds_ijk E[p, c], the row's share of G_att_edge (backward_dst): ds of an entry is formed by the
//     group that gathered it and handed BACK to the lane that owns the entry (one __shfl per step of a turn), and the owner
//     adds ds E[p, :] to its de accumulators once per chunk -- 64 lanes read 64 consecutive rows of E, the access of the
//     edge term itself.  A lane's entries in row order, then the lanes through wave_sum.  (Letting lane `sub` of the
//     gathering group add column sub of the entry's row, the obvious geometry, costs one scattered 4 de-byte read per
//     entry and group: 1.7 x the plain kernel at 128 columns / 4 heads and 3 x at 41 / 1, profiles/experiments/gat_efeat.log.)
//     The accumulators are a register array indexed by constants: no scratch.  The column sums of P_e are
//     mggcn_gatv2_att_grad_f32's.
// Internal linkage in each translation unit that includes it.  Not part of the ABI.
#pragma once

#include "common.h"
#include "reduce.h"

namespace {

constexpr int kEdgeSlots = MGGCN_GAT_MAX_EDGE_DIM;      // columns of E one lane can own: de <= 16 at LPR = 1

// the edge operands of a call; vec: a row of E may be read four columns at a time
struct gat_edge {
    const float *E, *U;
    size_t lde;
    uint32_t de;
    bool vec;
};

// t of position `pos` at head k: the one chain of the contract, c ascending
__device__ __forceinline__ float edge_term(const gat_edge &eg, uint32_t k, size_t pos) {
    const float *__restrict__ Uk = eg.U + (size_t)k * eg.de;
    const float *__restrict__ Ep = eg.E + pos * eg.lde;
    float t = 0.f;
    if (eg.vec) {
        for (uint32_t c = 0; c < eg.de; c += 4) {
            const float4 e = *reinterpret_cast<const float4 *>(Ep + c);
            t = fmaf(e.x, Uk[c], t);
            t = fmaf(e.y, Uk[c + 1], t);
            t = fmaf(e.z, Uk[c + 2], t);
            t = fmaf(e.w, Uk[c + 3], t);
        }
    } else {
        for (uint32_t c = 0; c < eg.de; c++) t = fmaf(Ep[c], Uk[c], t);
    }
    return t;
}

// pe[c] += ds E[pos, c] for c < de: the share of one entry in its row's P_e, on the lane that owns the entry.  The loops are
// unrolled over all sixteen slots with a wave-uniform test each, so pe is indexed by constants and stays in registers.
__device__ __forceinline__ void edge_axpy(const gat_edge &eg, size_t pos, float ds, float (&pe)[kEdgeSlots]) {
    const float *__restrict__ Ep = eg.E + pos * eg.lde;
    if (eg.vec) {
#pragma unroll
        for (int c = 0; c < kEdgeSlots; c += 4) {
            if ((uint32_t)c < eg.de) {
                const float4 e = *reinterpret_cast<const float4 *>(Ep + c);
                pe[c] = fmaf(ds, e.x, pe[c]);
                pe[c + 1] = fmaf(ds, e.y, pe[c + 1]);
                pe[c + 2] = fmaf(ds, e.z, pe[c + 2]);
                pe[c + 3] = fmaf(ds, e.w, pe[c + 3]);
            }
        }
    } else {
#pragma unroll
        for (int c = 0; c < kEdgeSlots; c++)
            if ((uint32_t)c < eg.de) pe[c] = fmaf(ds, Ep[c], pe[c]);
    }
}

// P_e[k de + c] of the row at P_e_row = the wave's sum of pe[c], slot by slot
__device__ __forceinline__ void edge_store(const gat_edge &eg, uint32_t k, uint32_t lane, const float (&pe)[kEdgeSlots],
                                           float *__restrict__ P_e_row) {
#pragma unroll
    for (int c = 0; c < kEdgeSlots; c++) {
        if ((uint32_t)c < eg.de) {              // wave-uniform
            const float s = wave_sum(pe[c]);
            if (lane == 0) P_e_row[(size_t)k * eg.de + c] = s;
        }
    }
}

}  // namespace
