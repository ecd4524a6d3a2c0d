// link_mlp.hip -- the MLP decoder of the link head (include/mggcn.h, "link prediction, MLP decoder"): a pair (u, v) scores
//     x = H[u] (.) H[v],   z = W1^T x + b1,   a = leaky_relu(z),   s = w2 . a + b2
// with W1 [d x hd], b1, w2 [hd] and b2 [1], d = 32 DB and hd = 32 HB, DB, HB in 1 .. 4.  The loss of a score is the dot
// decoder's (link_pair.h).  No reference counterpart.  Two kernels, both on v_mfma_f32_32x32x2_f32 (bitwise a k-ordered
// fmaf chain), neither with an atomic:
//
// link_mlp_loss_kernel -- the walk of link.hip with the same contract (three launches over P, P^T and the negatives'
// transpose, G[x] = beta G[x] + sum): s is symmetric in its endpoints and ds/dH[x] = dX (.) H[y] with dX = W1 dZ, so the row
// x of a pattern gets its whole gradient from its own pairs.  A persistent grid of 4-wave workgroups, W1 (rows padded to
// hd + 1 words: both products read it without a bank conflict), b1 and w2 in LDS once per workgroup, one wave per row, the
// row's own H[x] in a per-wave LDS strip.  The row's entries go in tiles of 32 pairs, lane = (pair t, half h):
//     forward   Z^T [hd x 32] = W1^T X^T: A = W1 from LDS, B = h_x[c] H[y_t][c] formed in registers.  Lane (t, h) owns the
//               columns c = 32 b + 8 q + 4 h + i (b < DB, q < 4, i < 4) of H[y_t] -- DB x 4 loads of 16 bytes, the two halves
//               of a pair together 32 contiguous bytes -- and k-step (b, q, i) pairs the low half's column with the high
//               half's.  The accumulators start at b1.
//     score     the C layout has lane = pair: s_t is an in-lane sum over the lane's z registers and one exchange with
//               lane ^ 32.
//     backward  dZ^T = g_t w2_j lrelu'(z) in place in the accumulators.  The C layout hands lane (t, h) the rows
//               j = 32 jb + 8 q + 4 h + i: the very pairing of the forward's k-steps, so the accumulator registers ARE the B
//               operand of dX^T [d x 32] = W1 dZ^T, 32 rows of d at a time.  No transpose goes through LDS.
//     gradient  dX^T comes out with lane (t, h) holding the columns it loaded of H[y_t]: acc[c] += dX^T[c][t] H[y_t][c] in
//               registers over all tiles of the row; the 32 pair-lanes are folded once at the end of the row (four DPP
//               rotations and one exchange per register) and lanes 0 and 32 store.
// A tile slot without a pair loads nothing and contributes exact zeros (g = 0).
//
// link_mlp_pairs_kernel -- a flat list of pairs (explicit, or the training list of P: position q -> entry q / (1 + R), slot
// 0 the positive, slot r + 1 negative r drawn again): the scores and / or the gradient of the four parameters from one pass
// over each pair.  A persistent grid of at most kLinkMlpPairsGrid workgroups; workgroup b takes tiles b, b + grid, ... of
// 32 pairs in order, its 4 waves share a tile: X [32 x d] is gathered coalesced (lane = column) and multiplied into LDS,
// wave w < HB owns the hidden columns [32 w, 32 w + 32) (the matrix instruction is 32 wide: at hd < 128 the waves
// beyond HB only gather), computes Z = X W1 with lane = hidden unit and rows = pairs, the partial scores of the blocks meet
// through LDS in block order, thread t < 32 forms g_t, and the wave's dZ -- again in place in the C layout, its registers
// the B operand -- goes into G_W1[:, block] += X^T dZ with X read transposed from the LDS tile; the DB x 16 accumulators
// live for the whole kernel.  G_b1 and G_w2 are column sums of the same registers, G_b2 the sum of g.  Every workgroup
// stores one partial [d hd + 2 hd + 1] and colsum_final_kernel (reduce.h) adds them in workgroup order.  The grid cap and
// the tile rule fix the bits of the sums.
#include "edge_draw.h"
#include "gat_internal.h"
#include "link_mlp_internal.h"
#include "link_pair.h"

namespace {

#define MLP_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

// W1 [D x HD] into LDS rows of LD words, b1 and w2 behind it: every thread of the workgroup, before a barrier
template <int D, int HD, int LD>
__device__ __forceinline__ void stage_params(float *W1s, float *b1s, float *w2s, const float *__restrict__ W1,
                                             const float *__restrict__ b1, const float *__restrict__ w2) {
    for (int i = threadIdx.x; i < D * HD; i += 256) W1s[(i / HD) * LD + (i % HD)] = W1[i];
    if (threadIdx.x < HD) {
        b1s[threadIdx.x] = b1[threadIdx.x];
        w2s[threadIdx.x] = w2[threadIdx.x];
    }
}

// R == 0: no negatives are drawn (launches (b) and (c) of link.hip); row_loss == nullptr: no row sums are written
template <int DB, int HB>
__global__ __launch_bounds__(256) void link_mlp_loss_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                            const uint32_t *__restrict__ indices,
                                                            const float *__restrict__ H, size_t ldh, bool vec,
                                                            const float *__restrict__ W1, const float *__restrict__ b1,
                                                            const float *__restrict__ w2, const float *__restrict__ b2p,
                                                            bool positive, float weight, uint32_t R, float neg_weight,
                                                            uint32_t n_draw, uint32_t k0, uint32_t k1, uint32_t epoch,
                                                            float beta, float *__restrict__ G, size_t ldg,
                                                            float *__restrict__ row_loss, uint32_t *__restrict__ row_correct) {
    constexpr int D = 32 * DB, HD = 32 * HB, LD = HD + 1;
    __shared__ __attribute__((aligned(16))) float W1s[D * LD];
    __shared__ __attribute__((aligned(16))) float b1s[HD];
    __shared__ __attribute__((aligned(16))) float w2s[HD];
    __shared__ __attribute__((aligned(16))) float hxs[4][D];
    stage_params<D, HD, LD>(W1s, b1s, w2s, W1, b1, w2);
    __syncthreads();
    const float b2 = *b2p;
    const uint32_t lane = threadIdx.x & 63, t = lane & 31, h = lane >> 5;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float *hx = hxs[wave];

    for (size_t row = (size_t)blockIdx.x * 4 + wave; row < n_rows; row += (size_t)gridDim.x * 4) {
        __builtin_amdgcn_wave_barrier();            // the strip's readers of the row before are done (one wave, in order)
        for (uint32_t c = lane; c < D; c += 64) hx[c] = H[row * ldh + c];
        __builtin_amdgcn_wave_barrier();
        const uint32_t beg = indptr[row], end = indptr[row + 1];
        float acc[DB][16];
#pragma unroll
        for (int b = 0; b < DB; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[b][r] = 0.f;
        float loss_pos = 0.f, loss_neg = 0.f;       // of my pair slot; both halves hold the same bits
        uint32_t hits = 0;

        entry_chunks<0> ch;
        ch.start(indices, beg, end, lane, no_scalars);
        for (uint32_t base = beg; base < end; base += 64) {
            ch.next(indices, base, end, lane, no_scalars);
            const uint32_t cnt = ch.cnt;
            link_negatives neg{base + lane, n_draw, k0, k1, epoch, {}};
            for (uint32_t pass = 0; pass <= R; pass++) {        // the chunk's entries, then negative r = pass - 1 of each
                const uint32_t my_c = pass == 0 ? ch.my_c : neg.next(pass - 1);
                const bool pos = pass == 0 && positive;
                const float w = pass == 0 ? weight : neg_weight;
                for (uint32_t k = 0; k * 32 < cnt; k++) {
                    const uint32_t slot = k * 32 + t;
                    const uint32_t c_t = (uint32_t)__shfl((int)my_c, (int)slot);
                    const bool ok = slot < cnt;
                    // ---- my columns of H[y_t] ----
                    float y[DB][4][4];
                    const float *yp = H + (size_t)c_t * ldh + 4 * h;
#pragma unroll
                    for (int b = 0; b < DB; b++)
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            if (ok) load4(y[b][q], yp + 32 * b + 8 * q, vec);
                            else y[b][q][0] = y[b][q][1] = y[b][q][2] = y[b][q][3] = 0.f;
                        }
                    // ---- forward: z = b1 + W1^T x ----
                    f32x16 z[HB];
#pragma unroll
                    for (int jb = 0; jb < HB; jb++)
#pragma unroll
                        for (int r = 0; r < 16; r++) z[jb][r] = b1s[32 * jb + 8 * (r >> 2) + 4 * h + (r & 3)];
#pragma unroll
                    for (int b = 0; b < DB; b++)
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            const float4 hx4 = *reinterpret_cast<const float4 *>(hx + 32 * b + 8 * q + 4 * h);
                            const float x[4] = {hx4.x * y[b][q][0], hx4.y * y[b][q][1], hx4.z * y[b][q][2], hx4.w * y[b][q][3]};
#pragma unroll
                            for (int i = 0; i < 4; i++) {
                                const float *wrow = W1s + (32 * b + 8 * q + 4 * h + i) * LD + t;
#pragma unroll
                                for (int jb = 0; jb < HB; jb++) z[jb] = MLP_MFMA(wrow[32 * jb], x[i], z[jb]);
                            }
                            MLP_SCHED_FENCE();
                        }
                    // ---- the score, the pair's terms ----
                    float s = 0.f;
#pragma unroll
                    for (int jb = 0; jb < HB; jb++)
#pragma unroll
                        for (int r = 0; r < 16; r++)
                            s = fmaf(w2s[32 * jb + 8 * (r >> 2) + 4 * h + (r & 3)], gat_lrelu(z[jb][r], kLinkMlpSlope), s);
                    s = (s + __shfl_xor(s, 32)) + b2;
                    const pair_terms pt = link_pair(s, pos, w);
                    const float g = ok ? pt.g : 0.f;
                    if (pos) loss_pos += ok ? pt.loss : 0.f;
                    else loss_neg += ok ? pt.loss : 0.f;
                    hits += ok ? pt.hit : 0u;
                    // ---- backward: dZ in place, dX 32 rows at a time, acc += dX (.) H[y] ----
#pragma unroll
                    for (int jb = 0; jb < HB; jb++)
#pragma unroll
                        for (int r = 0; r < 16; r++)
                            z[jb][r] = (g * w2s[32 * jb + 8 * (r >> 2) + 4 * h + (r & 3)]) * (z[jb][r] > 0.f ? 1.f : kLinkMlpSlope);
#pragma unroll
                    for (int cb = 0; cb < DB; cb++) {
                        f32x16 dx;
#pragma unroll
                        for (int r = 0; r < 16; r++) dx[r] = 0.f;
                        const float *wcol = W1s + (32 * cb + t) * LD + 4 * h;
#pragma unroll
                        for (int jb = 0; jb < HB; jb++)
#pragma unroll
                            for (int r = 0; r < 16; r++) {
                                dx = MLP_MFMA(wcol[32 * jb + 8 * (r >> 2) + (r & 3)], z[jb][r], dx);
                                if ((r & 3) == 3) MLP_SCHED_FENCE();
                            }
#pragma unroll
                        for (int r = 0; r < 16; r++) acc[cb][r] = fmaf(dx[r], y[cb][r >> 2][r & 3], acc[cb][r]);
                    }
                }
            }
        }

        float *__restrict__ g_row = G + row * ldg + 4 * h;
#pragma unroll
        for (int b = 0; b < DB; b++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                float v[4];
#pragma unroll
                for (int i = 0; i < 4; i++) v[i] = half_sum(acc[b][4 * q + i]);
                if (t == 0) {
                    float *p = g_row + 32 * b + 8 * q;
                    if (beta != 0.f) {              // beta == 0 never reads G
                        float old[4];
                        load4(old, p, vec);
#pragma unroll
                        for (int i = 0; i < 4; i++) v[i] = fmaf(beta, old[i], v[i]);
                    }
                    if (vec) *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
                    else { p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3]; }
                }
            }
        if (row_loss != nullptr) {
            loss_pos = half_sum(loss_pos);
            loss_neg = half_sum(loss_neg);
            hits = half_sum_u32(hits);
            if (lane == 0) {
                row_loss[2 * row] = loss_pos;
                row_loss[2 * row + 1] = loss_neg;
                row_correct[row] = hits;
            }
        }
    }
}

// src != nullptr: the explicit list (src, dst, m), every pair of label `positive` and weight `weight`; otherwise the
// training list of m = M (1 + R) pairs.  out and / or partials (the gradients) may be null.
template <int DB, int HB>
__global__ __launch_bounds__(256) void link_mlp_pairs_kernel(const uint32_t *__restrict__ src, const uint32_t *__restrict__ dst,
                                                             size_t m, const uint32_t *__restrict__ head,
                                                             const uint32_t *__restrict__ indices, uint32_t R, uint32_t n_draw,
                                                             uint32_t k0, uint32_t k1, uint32_t epoch, bool positive,
                                                             float weight, float neg_weight, const float *__restrict__ H,
                                                             size_t ldh, const float *__restrict__ W1,
                                                             const float *__restrict__ b1, const float *__restrict__ w2,
                                                             const float *__restrict__ b2p, float *__restrict__ out,
                                                             float *__restrict__ partials) {
    constexpr int D = 32 * DB, HD = 32 * HB, LDX = D + 1;
    __shared__ __attribute__((aligned(16))) float W1s[D * HD];
    __shared__ float b1s[HD], w2s[HD];
    __shared__ float Xs[32 * LDX];
    __shared__ float sps[HB][32], gs[32];
    __shared__ uint32_t us[32], vs[32], oks[32];
    stage_params<D, HD, HD>(W1s, b1s, w2s, W1, b1, w2);
    const float b2 = *b2p;
    const bool grads = partials != nullptr;
    const uint32_t tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool owner = wave < HB;                   // of the hidden columns [32 wave, 32 wave + 32)
    const uint32_t j = owner ? 32 * wave + l31 : 0;

    f32x16 accW[DB];
#pragma unroll
    for (int cb = 0; cb < DB; cb++)
#pragma unroll
        for (int r = 0; r < 16; r++) accW[cb][r] = 0.f;
    float gb1 = 0.f, gw2 = 0.f, gb2 = 0.f;
    __syncthreads();
    const float b1j = b1s[j], w2j = w2s[j];

    const size_t n_tiles = (m + 31) / 32;
    for (size_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        // ---- 1: the tile's pairs ----
        const size_t qi = tile * 32 + tid;
        bool my_ok = false, my_pos = positive;
        float my_w = weight;
        if (tid < 32) {
            my_ok = qi < m;
            uint32_t u = 0, v = 0;
            if (my_ok) {
                if (src != nullptr) {
                    u = src[qi];
                    v = dst[qi];
                } else {
                    const uint32_t p = (uint32_t)(qi / (1 + R)), slot = (uint32_t)(qi % (1 + R));
                    u = head[p];
                    if (slot == 0) {
                        v = indices[p];
                        my_pos = true;
                    } else {
                        v = link_negative(p, slot - 1, n_draw, epoch, k0, k1);
                        my_pos = false;
                        my_w = neg_weight;
                    }
                }
            }
            us[tid] = u; vs[tid] = v; oks[tid] = my_ok ? 1u : 0u;
        }
        __syncthreads();
        // ---- 2: X = H[u] (.) H[v], eight pairs per wave, lane = column ----
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const uint32_t tt = 8 * wave + i;
            const bool ok = oks[tt] != 0;
            const float *hu = H + (size_t)us[tt] * ldh, *hv = H + (size_t)vs[tt] * ldh;
            for (uint32_t c = lane; c < D; c += 64) Xs[tt * LDX + c] = ok ? hu[c] * hv[c] : 0.f;
        }
        __syncthreads();
        // ---- 3: my block of Z = b1 + X W1, its part of the scores ----
        f32x16 z;
        float a[16];
        if (owner) {
#pragma unroll
            for (int r = 0; r < 16; r++) z[r] = b1j;
#pragma unroll 8
            for (int kk = 0; kk < D / 2; kk++) {
                const int c = 2 * kk + h;
                z = MLP_MFMA(Xs[l31 * LDX + c], W1s[c * HD + j], z);
            }
#pragma unroll
            for (int r = 0; r < 16; r++) {
                a[r] = gat_lrelu(z[r], kLinkMlpSlope);
                const float p = half_dot(w2j, a[r]);
                if (l31 == 0) sps[wave][c_row(r, h)] = p;
            }
        }
        __syncthreads();
        // ---- 4: the scores, g ----
        if (tid < 32) {
            float s = sps[0][tid];
#pragma unroll
            for (int jb = 1; jb < HB; jb++) s += sps[jb][tid];
            s += b2;
            if (my_ok && out != nullptr) out[qi] = s;
            if (grads) {
                const float g = my_ok ? link_pair(s, my_pos, my_w).g : 0.f;
                gs[tid] = g;
                gb2 += g;
            }
        }
        if (!grads) continue;                       // the barriers of steps 1 and 2 keep the next tile apart
        __syncthreads();
        // ---- 5: dZ in place, the column sums, G_W1[:, block] += X^T dZ ----
        if (owner) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const float g = gs[c_row(r, h)];
                gw2 = fmaf(g, a[r], gw2);
                const float dz = (g * w2j) * (z[r] > 0.f ? 1.f : kLinkMlpSlope);
                gb1 += dz;
                z[r] = dz;
            }
#pragma unroll
            for (int cb = 0; cb < DB; cb++)
#pragma unroll
                for (int r = 0; r < 16; r++) accW[cb] = MLP_MFMA(Xs[c_row(r, h) * LDX + 32 * cb + l31], z[r], accW[cb]);
        }
    }

    if (!grads) return;
    float *part = partials + (size_t)blockIdx.x * (D * HD + 2 * HD + 1);
    if (owner) {
#pragma unroll
        for (int cb = 0; cb < DB; cb++)
#pragma unroll
            for (int r = 0; r < 16; r++) part[(size_t)(32 * cb + c_row(r, h)) * HD + j] = accW[cb][r];
        gb1 += __shfl_xor(gb1, 32);
        gw2 += __shfl_xor(gw2, 32);
        if (h == 0) {
            part[D * HD + j] = gb1;
            part[D * HD + HD + j] = gw2;
        }
    }
    if (wave == 0) {
        gb2 = half_sum(gb2);                        // threads 32 .. 63 hold zeros of their own half
        if (tid == 0) part[D * HD + 2 * HD] = gb2;
    }
}

}  // namespace

MGGCN_API void mggcn_link_mlp_loss_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                       const uint32_t *indices, size_t nnz, const float *H, size_t ldh, uint32_t d,
                                       const float *W1, const float *b1, const float *w2, const float *b2, uint32_t hd,
                                       int positive, float weight, uint32_t R, float neg_weight, uint64_t seed, uint32_t epoch,
                                       float beta, float *G, size_t ldg, float *row_loss, uint32_t *row_correct) {
    if (!require_walk({H, ldh, 4, W1}, n_rows, n_cols, indptr, indices, nnz, d, hd, b1, w2, b2, R, G, ldg, row_loss, row_correct))
        return;
    const bool vec = rows16(H, ldh) && rows16(G, ldg);
    const unsigned grid = (unsigned)std::min<size_t>(((size_t)n_rows + 3) / 4, kLinkMlpWalkGrid);
    mlp_dispatch(d, hd, [&](auto db, auto hb) {
        hipLaunchKernelGGL((link_mlp_loss_kernel<db.value, hb.value>), dim3(grid), dim3(256), 0, as_stream(stream), n_rows,
                           indptr, indices, H, ldh, vec, W1, b1, w2, b2, positive != 0, weight, nnz ? R : 0u, neg_weight, n_cols,
                           (uint32_t)(seed & 0xFFFFFFFFull), (uint32_t)(seed >> 32), epoch, beta, G, ldg, row_loss, row_correct);
        MGGCN_CHECK_LAUNCH();
    });
}

MGGCN_API size_t mggcn_link_mlp_partial_floats(uint32_t d, uint32_t hd) {
    return (size_t)kLinkMlpPairsGrid * link_mlp_grad_floats(d, hd);
}

MGGCN_API void mggcn_link_mlp_pairs_f32(mggcn_stream_t stream, const uint32_t *src, const uint32_t *dst, size_t m,
                                        const uint32_t *head, const uint32_t *indices, size_t M, uint32_t R, uint32_t n_draw,
                                        uint64_t seed, uint32_t epoch, int positive, float weight, float neg_weight,
                                        const float *H, size_t ldh, size_t n_rows, uint32_t d, const float *W1, const float *b1,
                                        const float *w2, const float *b2, uint32_t hd, float *out, float *grads,
                                        float *partials) {
    m = require_pairs({H, ldh, 4, W1}, src, dst, m, head, indices, M, R, n_draw, n_rows, d, hd, b1, w2, b2, out, grads, partials,
                      mggcn_link_mlp_partial_floats(d, hd));
    const hipStream_t st = as_stream(stream);
    unsigned grid = 0;
    if (m) {
        grid = (unsigned)std::min<size_t>((m + 31) / 32, kLinkMlpPairsGrid);
        mlp_dispatch(d, hd, [&](auto db, auto hb) {
            hipLaunchKernelGGL((link_mlp_pairs_kernel<db.value, hb.value>), dim3(grid), dim3(256), 0, st, src, dst, m, head,
                               indices, R, n_draw, (uint32_t)(seed & 0xFFFFFFFFull), (uint32_t)(seed >> 32), epoch, positive != 0,
                               weight, neg_weight, H, ldh, W1, b1, w2, b2, out, partials);
            MGGCN_CHECK_LAUNCH();
        });
    }
    if (grads != nullptr) pairs_final(st, partials, grid, d, hd, grads);
}
