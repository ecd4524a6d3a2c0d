// edge_select.hip -- the exact fan-out of the per-epoch edge sample (gfx950): one threshold per destination, written on the
// device every epoch, so that "the k smallest Philox words of the row win".  Over the forward matrix F only (rows are
// destinations).  Row i's candidates are its entries with i != j, each as it lies (a duplicated pair counts twice and carries
// the same word), m_i their number:
//     m_i <= k:   thr[i] = t_keep
//     otherwise:  thr[i] = min(s_i, t_keep, 0xFFFFFFFE),  s_i the (k+1)-th smallest candidate word (multiset order).
// The word is edge_draw.h's -- the one count and compact draw -- so under their keep rule (w < thr) row i keeps its self
// entries and at most k others, on F and, thr gathered, on F^T alike.  thr is a pure function of (seed, epoch, the row's
// multiset of pairs): a selection has no order to depend on.
//
// One wave per row, four rows per workgroup (the row walk of count and compact).  Three paths, chosen per row:
//   short      len <= k: no index is read.  m <= k after the self entries are counted: no word is drawn.
//   register   len <= 64 R: lane l holds entries l, l + 64, ... of the row in R registers, first the columns, then -- m > k --
//              their words, drawn ONCE; a self entry or a slot past the row's end holds 0xFFFFFFFF, which is never below a
//              candidate, so the (k+1)-th smallest of the 64 R slots is the (k+1)-th smallest candidate.  The select is a
//              descent over the VALUE, one bit per step: s is the largest v with #{w < v} <= k, and that predicate is
//              monotone in v, so bit b of s is set iff #{w < prefix | 1 << b} <= k.  A step is R compares whose lane masks
//              the scalar unit counts (v_cmp, s_bcnt1, s_add): no shuffle, no LDS, no per-digit rank to carry; prefix and
//              count live in SGPRs.  32 R compares in all -- less than the draw itself (DESIGN.md 3.14.2 on the digit width).
//   streaming  longer rows, and every row under force_stream: words are not stored, every pass draws again.  A pass
//              histograms the next 8-bit digit of the candidates that match the prefix so far into the wave's own 256 LDS bins
//              (integer LDS adds: a sum of ones has no order), a wave scan of the bins (four per lane, shfl_up over the lane
//              sums) finds the bin that holds the rank, and prefix and rank move on.  When that bin holds at most 64 R
//              words, one more pass collects them into the wave's LDS pool (ballot ranks, bounded stores) and the register
//              descent finishes on the remaining bits; otherwise the next digit is histogrammed.  After four digits the
//              prefix IS the answer: at most four histogram passes plus one collect for any row length up to 2^32 - 1.
// No global atomics, no scratch, nothing of size nnz, no workgroup waits on another (no __syncthreads at all: the LDS
// slices are per wave and ordered by the wave's own program order), nothing written but thr[row].
#include "common.h"
#include "edge_draw.h"

namespace {

struct select_args {
    uint32_t k, t_keep, row0, col0, k0, k1, epoch;
    bool force_stream;
};

// the (rank + 1)-th smallest of the wave's 64 R words, all of which agree with ``prefix`` above bit ``top``: the largest v
// with #{w < v} <= rank, built from bit ``top`` down.  Wave-uniform: the counts are scalar population counts of ballots.
template <int R>
__device__ __forceinline__ uint32_t select_descent(const uint32_t (&w)[R], uint32_t rank, uint32_t prefix, int top) {
    for (int b = top; b >= 0; b--) {
        const uint32_t v = prefix | (1u << b);
        uint32_t below = 0;
#pragma unroll
        for (int r = 0; r < R; r++) below += (uint32_t)__popcll(__ballot(w[r] < v));
        if (below <= rank) prefix = v;
    }
    return prefix;
}

template <int R>
__global__ __launch_bounds__(256) void edge_select_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                          const uint32_t *__restrict__ indices, select_args a,
                                                          uint32_t *__restrict__ thr) {
    constexpr uint32_t kReg = 64u * R;                              // the entries the registers (and the pool) hold
    __shared__ uint32_t hist[4][256];
    __shared__ uint32_t pool[4][kReg];
    const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t row = (size_t)blockIdx.x * 4 + wave;
    if (row >= n_rows) return;
    const uint32_t beg = indptr[row], len = indptr[row + 1] - beg;
    const uint32_t i = a.row0 + (uint32_t)row;
    uint32_t s;                                                     // the (k+1)-th smallest candidate word
    if (len <= a.k) {                                               // m <= len <= k
        if (lane == 0) thr[row] = a.t_keep;
        return;
    }
    if (!a.force_stream && len <= kReg) {
        uint32_t w[R], m = 0;
#pragma unroll
        for (int r = 0; r < R; r++) {                               // the columns; a slot that holds no candidate gets i
            const uint32_t at = (uint32_t)r * 64 + lane;
            w[r] = at < len ? a.col0 + indices[(size_t)beg + at] : i;
            m += (uint32_t)__popcll(__ballot(w[r] != i));
        }
        if (m <= a.k) {
            if (lane == 0) thr[row] = a.t_keep;
            return;
        }
#pragma unroll
        for (int r = 0; r < R; r++) w[r] = w[r] != i ? sample_word(i, w[r], a.epoch, a.k0, a.k1) : 0xFFFFFFFFu;
        s = select_descent<R>(w, a.k, 0u, 31);
    } else {
        const uint64_t lanes_below = ((uint64_t)1 << lane) - 1;
        uint32_t prefix = 0, rank = a.k, fixed = 0;                 // fixed: the mask of the bits of prefix that are decided
        int shift = 24;
        for (;; shift -= 8) {
#pragma unroll
            for (int q = 0; q < 4; q++) hist[wave][q * 64 + lane] = 0;
            __builtin_amdgcn_wave_barrier();
            for (uint64_t e = lane; e < len; e += 64) {
                const uint32_t j = a.col0 + indices[(size_t)beg + e];
                if (j == i) continue;
                const uint32_t word = sample_word(i, j, a.epoch, a.k0, a.k1);
                if (((word ^ prefix) & fixed) == 0) atomicAdd(&hist[wave][(word >> shift) & 255u], 1u);
            }
            __builtin_amdgcn_wave_barrier();
            uint32_t h[4], mine = 0;                                // lane l: bins 4 l .. 4 l + 3
#pragma unroll
            for (int q = 0; q < 4; q++) {
                h[q] = hist[wave][lane * 4 + q];
                mine += h[q];
            }
            __builtin_amdgcn_wave_barrier();                        // the bins are cleared again by the next pass
            uint32_t upto = mine;                                   // inclusive over the lanes; at most len: no overflow
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t up = __shfl_up(upto, off);
                if (lane >= (uint32_t)off) upto += up;
            }
            if (shift == 24 && (uint32_t)__shfl(upto, 63) <= a.k) {          // the first pass counted the candidates: m <= k
                if (lane == 0) thr[row] = a.t_keep;
                return;
            }
            // rank < the pass's total (m > k at first, the chosen bin's count afterwards): exactly one bin holds it
            uint32_t before = upto - mine, digit = 0, under = 0, inside = 0;
            bool found = false;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if (!found && rank < before + h[q]) {
                    found = true;
                    digit = lane * 4 + q, under = before, inside = h[q];
                }
                before += h[q];
            }
            const int src = __ffsll((unsigned long long)__ballot(found)) - 1;
            digit = __shfl(digit, src), under = __shfl(under, src), inside = __shfl(inside, src);
            prefix |= digit << shift;
            fixed |= 255u << shift;
            rank -= under;
            if (shift == 0) {                                       // all 32 bits are decided
                s = prefix;
                break;
            }
            if (inside <= kReg) {                                   // the bin fits the pool: collect it, finish in registers
                uint32_t base = 0;
                for (uint64_t chunk = 0; chunk < len; chunk += 64) {        // wave-uniform trip count: the ballot wants every lane
                    const uint64_t e = chunk + lane;
                    uint32_t word = 0;
                    bool in = false;
                    if (e < len) {
                        const uint32_t j = a.col0 + indices[(size_t)beg + e];
                        if (j != i) {
                            word = sample_word(i, j, a.epoch, a.k0, a.k1);
                            in = ((word ^ prefix) & fixed) == 0;
                        }
                    }
                    const uint64_t bits = __ballot(in);
                    const uint32_t at = base + (uint32_t)__popcll(bits & lanes_below);
                    if (in && at < kReg) pool[wave][at] = word;     // the bound holds by construction: the histogram drew the same words
                    base += (uint32_t)__popcll(bits);
                }
                __builtin_amdgcn_wave_barrier();
                uint32_t w[R];
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const uint32_t at = (uint32_t)r * 64 + lane;
                    w[r] = at < inside ? pool[wave][at] : 0xFFFFFFFFu;
                }
                s = select_descent<R>(w, rank, prefix, shift - 1);
                break;
            }
        }
    }
    if (lane == 0) thr[row] = min(min(s, a.t_keep), 0xFFFFFFFEu);
}

template <int R>
void launch_select(hipStream_t st, uint32_t n_rows, const uint32_t *indptr, const uint32_t *indices, const select_args &a,
                   uint32_t *thr) {
    hipLaunchKernelGGL(edge_select_kernel<R>, dim3((unsigned)(((size_t)n_rows + 3) / 4)), dim3(256), 0, st, n_rows, indptr, indices,
                       a, thr);
}

}  // namespace

// ============================ C ABI =========================================
MGGCN_API uint32_t mggcn_edge_sample_select_reg_entries(void) { return 64u * MGGCN_EDGE_SELECT_R; }

MGGCN_API void mggcn_edge_sample_select_r_u32(mggcn_stream_t stream, uint32_t n_rows, const uint32_t *indptr,
                                              const uint32_t *indices, uint32_t k, uint32_t t_keep, uint32_t row0, uint32_t col0,
                                              uint64_t seed, uint32_t epoch, int force_stream, uint32_t R, uint32_t *thr) {
    MGGCN_REQUIRE(k >= 1, "edge sample select: k must be at least 1");
    MGGCN_REQUIRE(R == 4 || R == 8 || R == 12 || R == 16, "edge sample select: R must be 4, 8, 12 or 16");
    if (!n_rows) return;
    MGGCN_REQUIRE(indptr != nullptr && thr != nullptr, "edge sample select: null operand");
    const select_args a = {k, t_keep, row0, col0, (uint32_t)(seed & 0xFFFFFFFFull), (uint32_t)(seed >> 32), epoch, force_stream != 0};
    const hipStream_t st = as_stream(stream);
    switch (R) {
        case 4: launch_select<4>(st, n_rows, indptr, indices, a, thr); break;
        case 8: launch_select<8>(st, n_rows, indptr, indices, a, thr); break;
        case 12: launch_select<12>(st, n_rows, indptr, indices, a, thr); break;
        default: launch_select<16>(st, n_rows, indptr, indices, a, thr); break;
    }
    MGGCN_CHECK_LAUNCH();
}

MGGCN_API void mggcn_edge_sample_select_u32(mggcn_stream_t stream, uint32_t n_rows, const uint32_t *indptr,
                                            const uint32_t *indices, uint32_t k, uint32_t t_keep, uint32_t row0, uint32_t col0,
                                            uint64_t seed, uint32_t epoch, int force_stream, uint32_t *thr) {
    mggcn_edge_sample_select_r_u32(stream, n_rows, indptr, indices, k, t_keep, row0, col0, seed, epoch, force_stream,
                                   MGGCN_EDGE_SELECT_R, thr);
}
