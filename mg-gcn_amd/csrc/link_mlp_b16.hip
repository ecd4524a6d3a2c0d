// link_mlp_b16.hip -- the MLP decoder of the link head on the bf16 matrix instruction v_mfma_f32_32x32x16_bf16 (include/mggcn.h,
// "link prediction, MLP decoder, bf16 operands"): link_mlp.hip's two kernels and three-launch contract with the operands of
// both products rounded to bf16 and the sums kept in fp32.  No reference counterpart.
//     Hb = bf16(H) (mggcn_convert_f32_bf16), W1b = bf16(W1) (mggcn_link_mlp_pack_bf16), both round to nearest even
//     x  = bf16(Hb[u] Hb[v])        the product of two bf16 values is exact in fp32: one rounding
//     z  = b1 + W1b^T x             fp32 accumulation; a, s, the loss, g and the hit in fp32 as link_pair.h has them
//     dz = bf16(g w2 lrelu'(z)),  dx = W1b dz,  G[x] = beta G[x] + sum dx (.) Hb[y],  G_W1 = sum x^T dz        (straight-through)
//     G_b1, G_w2, G_b2 from the unrounded fp32 dz, g a and g.
//
// The instruction: lane (t = l % 32, h = l / 32) holds 8 consecutive k-slots 8 h .. 8 h + 7 of row t of A and of column t of B;
// register r of lane (t, h) is row c_row(r, h) = 8 (r / 4) + 4 h + (r % 4) of column t of C.  The order of k inside a product is
// free as long as A and B agree, so slot e of lane half h in step s of a 32-block stands for index
//     16 s + 8 (e / 4) + 4 h + (e % 4) = c_row(8 s + e, h):
// a lane's 16 slots over the two steps of a block are the 16 rows the C layout gives it.  Eight consecutive accumulator
// registers, rounded and packed, are therefore one B operand of the next product, and that product lands on the lane that holds
// the matching columns: link_mlp.hip's trick of never transposing through LDS survives the 16-deep instruction.
// perm32(i) = i with bits 2 and 3 swapped (an involution) is the place of index i in that order: a row stored as
// row[32 b + perm32(i)] gives lane half h its 8 slots of step s as the 16 contiguous bytes at 32 b + 16 s + 8 h.
//
// The W1 image (mggcn_link_mlp_pack_bf16) holds both orientations in that order, rows padded by 8 elements so that the
// 16-byte LDS reads of 16 lanes fall into 16 different groups of 4 banks:
//     F [hd x (d + 8)]   F[j][perm(c)] = W1b[c][j]      A operand of the forward Z^T = W1^T X^T, B operand of the pairs' Z = X W1
//     B [d x (hd + 8)]   B[c][perm(j)] = W1b[c][j]      A operand of the backward dX^T = W1 dZ^T
// with perm the swap inside each 32-block.  At 128 x 128 the two are 68 KiB (the fp32 W1 padded: 64.5 KiB): two workgroups of the
// walk still fit a CU.  One copy with strided 2-byte reads for the other orientation was rejected: it turns one read per MFMA
// into eight.  Hb is plain row-major: a lane's columns of a block are 4 x 8 bytes and the halves of a pair read 16 contiguous bytes.
//
// link_mlp_loss_b16_kernel -- link_mlp_loss_kernel with 2 MFMAs per (32-block of d, 32-block of hd) in place of 16, each A
// operand one 16-byte LDS read.  The row's own Hb[x] sits widened in the per-wave strip; H[y_t] stays packed in registers and is
// widened where it is multiplied.  link_mlp_pairs_b16_kernel -- link_mlp_pairs_kernel with the tile X [32 x d] formed in bf16
// and kept in LDS in both orientations (X for Z = X W1b, X^T for G_W1 += X^T dZ, whose k is the tile's 32 pairs: two MFMAs per
// (cb, block)); the owner wave's columns of F stay in registers for the whole kernel, so W1 is never staged.  The same
// persistent grids, tile rules, partial layout and colsum_final_kernel epilogue as the fp32 kernels: the same bits on every
// call, no atomics.
#include "edge_draw.h"
#include "gat_internal.h"
#include "link_mlp_internal.h"
#include "link_pair.h"

namespace {

#define B16_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, (a)), __builtin_bit_cast(bf16x8, (b)), (c), 0, 0, 0)

// both orientations of W1 and the zero padding, one thread per element of W1
__global__ __launch_bounds__(256) void link_mlp_pack_kernel(const float *__restrict__ W1, uint32_t d, uint32_t hd,
                                                            uint16_t *__restrict__ image) {
    uint16_t *F = image, *B = image + (size_t)hd * (d + kPad);
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < d * hd) {
        const uint32_t c = i / hd, j = i % hd;
        const uint16_t v = __builtin_bit_cast(uint16_t, (__bf16)W1[i]);
        F[(size_t)j * (d + kPad) + perm32(c)] = v;
        B[(size_t)c * (hd + kPad) + perm32(j)] = v;
    }
    if (i < hd * kPad) F[(size_t)(i / kPad) * (d + kPad) + d + i % kPad] = 0;
    if (i < d * kPad) B[(size_t)(i / kPad) * (hd + kPad) + hd + i % kPad] = 0;
}

// R == 0: no negatives are drawn; row_loss == nullptr: no row sums are written
template <int DB, int HB>
__global__ __launch_bounds__(256) void link_mlp_loss_b16_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                                const uint32_t *__restrict__ indices,
                                                                const uint16_t *__restrict__ Hb, size_t ldhb,
                                                                const uint16_t *__restrict__ image, const float *__restrict__ b1,
                                                                const float *__restrict__ w2, const float *__restrict__ b2p,
                                                                bool positive, float weight, uint32_t R, float neg_weight,
                                                                uint32_t n_draw, uint32_t k0, uint32_t k1, uint32_t epoch,
                                                                float beta, float *__restrict__ G, size_t ldg, bool vec,
                                                                float *__restrict__ row_loss, uint32_t *__restrict__ row_correct) {
    constexpr int D = 32 * DB, HD = 32 * HB, LDF = D + kPad, LDB = HD + kPad;
    __shared__ __attribute__((aligned(16))) uint16_t Ws[HD * LDF + D * LDB];     // F, then B: the image as it is
    __shared__ __attribute__((aligned(16))) float b1s[HD];
    __shared__ __attribute__((aligned(16))) float w2s[HD];
    __shared__ __attribute__((aligned(16))) float hxs[4][D];
    for (int i = threadIdx.x; i < (HD * LDF + D * LDB) / 8; i += 256)
        reinterpret_cast<uint4 *>(Ws)[i] = reinterpret_cast<const uint4 *>(image)[i];
    if (threadIdx.x < HD) {
        b1s[threadIdx.x] = b1[threadIdx.x];
        w2s[threadIdx.x] = w2[threadIdx.x];
    }
    __syncthreads();
    const uint16_t *Fs = Ws, *Bs = Ws + HD * LDF;
    const float b2 = *b2p;
    const uint32_t lane = threadIdx.x & 63, t = lane & 31, h = lane >> 5;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float *hx = hxs[wave];

    for (size_t row = (size_t)blockIdx.x * 4 + wave; row < n_rows; row += (size_t)gridDim.x * 4) {
        __builtin_amdgcn_wave_barrier();            // the strip's readers of the row before are done (one wave, in order)
        for (uint32_t c = 2 * lane; c < D; c += 128) {
            const uint32_t p = *reinterpret_cast<const uint32_t *>(Hb + row * ldhb + c);
            hx[c] = widen_lo(p);
            hx[c + 1] = widen_hi(p);
        }
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
                    // ---- my columns 32 b + 8 q + 4 h + i of Hb[y_t], packed ----
                    uint2 y[DB][4];
                    const uint16_t *yp = Hb + (size_t)c_t * ldhb + 4 * h;
#pragma unroll
                    for (int b = 0; b < DB; b++)
#pragma unroll
                        for (int q = 0; q < 4; q++)
                            y[b][q] = ok ? *reinterpret_cast<const uint2 *>(yp + 32 * b + 8 * q) : make_uint2(0u, 0u);
                    // ---- forward: z = b1 + W1b^T x, x rounded as it is formed ----
                    f32x16 z[HB];
#pragma unroll
                    for (int jb = 0; jb < HB; jb++)
#pragma unroll
                        for (int r = 0; r < 16; r++) z[jb][r] = b1s[32 * jb + c_row(r, h)];
#pragma unroll
                    for (int b = 0; b < DB; b++)
#pragma unroll
                        for (int s = 0; s < 2; s++) {
                            uint4 x;
                            {
                                const float4 a = *reinterpret_cast<const float4 *>(hx + 32 * b + 16 * s + 4 * h);
                                const float4 c = *reinterpret_cast<const float4 *>(hx + 32 * b + 16 * s + 8 + 4 * h);
                                const uint2 ya = y[b][2 * s], yc = y[b][2 * s + 1];
                                x.x = bf16_pair(a.x * widen_lo(ya.x), a.y * widen_hi(ya.x));
                                x.y = bf16_pair(a.z * widen_lo(ya.y), a.w * widen_hi(ya.y));
                                x.z = bf16_pair(c.x * widen_lo(yc.x), c.y * widen_hi(yc.x));
                                x.w = bf16_pair(c.z * widen_lo(yc.y), c.w * widen_hi(yc.y));
                            }
                            const uint16_t *wrow = Fs + t * LDF + 32 * b + 16 * s + 8 * h;
#pragma unroll
                            for (int jb = 0; jb < HB; jb++)
                                z[jb] = B16_MFMA(*reinterpret_cast<const uint4 *>(wrow + 32 * jb * LDF), x, z[jb]);
                            MLP_SCHED_FENCE();
                        }
                    // ---- the score, the pair's terms ----
                    float s = 0.f;
#pragma unroll
                    for (int jb = 0; jb < HB; jb++)
#pragma unroll
                        for (int r = 0; r < 16; r++)
                            s = fmaf(w2s[32 * jb + c_row(r, h)], gat_lrelu(z[jb][r], kLinkMlpSlope), s);
                    s = (s + __shfl_xor(s, 32)) + b2;
                    const pair_terms pt = link_pair(s, pos, w);
                    const float g = ok ? pt.g : 0.f;
                    if (pos) loss_pos += ok ? pt.loss : 0.f;
                    else loss_neg += ok ? pt.loss : 0.f;
                    hits += ok ? pt.hit : 0u;
                    // ---- backward: dZ rounded and packed from the accumulators, dX 32 rows at a time, acc += dX (.) Hb[y] ----
                    uint4 dz[HB][2];
#pragma unroll
                    for (int jb = 0; jb < HB; jb++)
#pragma unroll
                        for (int s2 = 0; s2 < 2; s2++) {
                            float v[8];
#pragma unroll
                            for (int e = 0; e < 8; e++) {
                                const int r = 8 * s2 + e;
                                v[e] = (g * w2s[32 * jb + c_row(r, h)]) * (z[jb][r] > 0.f ? 1.f : kLinkMlpSlope);
                            }
                            dz[jb][s2] = make_uint4(bf16_pair(v[0], v[1]), bf16_pair(v[2], v[3]), bf16_pair(v[4], v[5]), bf16_pair(v[6], v[7]));
                        }
#pragma unroll
                    for (int cb = 0; cb < DB; cb++) {
                        f32x16 dx;
#pragma unroll
                        for (int r = 0; r < 16; r++) dx[r] = 0.f;
                        const uint16_t *wcol = Bs + (32 * cb + t) * LDB + 8 * h;
#pragma unroll
                        for (int jb = 0; jb < HB; jb++)
#pragma unroll
                            for (int s2 = 0; s2 < 2; s2++)
                                dx = B16_MFMA(*reinterpret_cast<const uint4 *>(wcol + 32 * jb + 16 * s2), dz[jb][s2], dx);
                        MLP_SCHED_FENCE();
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            const uint2 yq = y[cb][q];
                            acc[cb][4 * q + 0] = fmaf(dx[4 * q + 0], widen_lo(yq.x), acc[cb][4 * q + 0]);
                            acc[cb][4 * q + 1] = fmaf(dx[4 * q + 1], widen_hi(yq.x), acc[cb][4 * q + 1]);
                            acc[cb][4 * q + 2] = fmaf(dx[4 * q + 2], widen_lo(yq.y), acc[cb][4 * q + 2]);
                            acc[cb][4 * q + 3] = fmaf(dx[4 * q + 3], widen_hi(yq.y), acc[cb][4 * q + 3]);
                        }
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
__global__ __launch_bounds__(256) void link_mlp_pairs_b16_kernel(const uint32_t *__restrict__ src, const uint32_t *__restrict__ dst,
                                                                 size_t m, const uint32_t *__restrict__ head,
                                                                 const uint32_t *__restrict__ indices, uint32_t R, uint32_t n_draw,
                                                                 uint32_t k0, uint32_t k1, uint32_t epoch, bool positive,
                                                                 float weight, float neg_weight, const uint16_t *__restrict__ Hb,
                                                                 size_t ldhb, const uint16_t *__restrict__ image,
                                                                 const float *__restrict__ b1, const float *__restrict__ w2,
                                                                 const float *__restrict__ b2p, float *__restrict__ out,
                                                                 float *__restrict__ partials) {
    constexpr int D = 32 * DB, HD = 32 * HB, LDF = D + kPad, LDX = D + kPad, LDT = 32 + kPad;
    __shared__ __attribute__((aligned(16))) uint16_t Xs[32 * LDX];      // X[pair][perm(c)]: the A operand of Z = X W1b
    __shared__ __attribute__((aligned(16))) uint16_t XTs[D * LDT];      // X[perm(pair)] of column c: the A operand of X^T dZ
    __shared__ float sps[HB][32], gs[32];
    __shared__ uint32_t us[32], vs[32], oks[32];
    const float b2 = *b2p;
    const bool grads = partials != nullptr;
    const uint32_t tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool owner = wave < HB;                   // of the hidden columns [32 wave, 32 wave + 32)
    const uint32_t j = owner ? 32 * wave + l31 : 0;

    uint4 wj[2 * DB];                               // my slots of row j of F: the B operands of every tile
#pragma unroll
    for (int ks = 0; ks < 2 * DB; ks++) wj[ks] = *reinterpret_cast<const uint4 *>(image + (size_t)j * LDF + 16 * ks + 8 * h);
    const float b1j = b1[j], w2j = w2[j];
    f32x16 accW[DB];
#pragma unroll
    for (int cb = 0; cb < DB; cb++)
#pragma unroll
        for (int r = 0; r < 16; r++) accW[cb][r] = 0.f;
    float gb1 = 0.f, gw2 = 0.f, gb2 = 0.f;

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
        // ---- 2: X = bf16(Hb[u] (.) Hb[v]) in both orientations, eight pairs per wave, lane = two columns ----
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const uint32_t tt = 8 * wave + i;
            const bool ok = oks[tt] != 0;
            const uint16_t *hu = Hb + (size_t)us[tt] * ldhb, *hv = Hb + (size_t)vs[tt] * ldhb;
            if (2 * lane < D) {
                const uint32_t c = 2 * lane;
                uint32_t x = 0;
                if (ok) {
                    const uint32_t pu = *reinterpret_cast<const uint32_t *>(hu + c), pv = *reinterpret_cast<const uint32_t *>(hv + c);
                    x = bf16_pair(widen_lo(pu) * widen_lo(pv), widen_hi(pu) * widen_hi(pv));
                }
                *reinterpret_cast<uint32_t *>(Xs + tt * LDX + (c & ~31u) + perm32(c & 31u)) = x;
                XTs[c * LDT + perm32(tt)] = (uint16_t)(x & 0xFFFFu);
                XTs[(c + 1) * LDT + perm32(tt)] = (uint16_t)(x >> 16);
            }
        }
        __syncthreads();
        // ---- 3: my block of Z = b1 + X W1b, its part of the scores ----
        f32x16 z;
        float a[16];
        if (owner) {
#pragma unroll
            for (int r = 0; r < 16; r++) z[r] = b1j;
#pragma unroll
            for (int ks = 0; ks < 2 * DB; ks++)
                z = B16_MFMA(*reinterpret_cast<const uint4 *>(Xs + l31 * LDX + 16 * ks + 8 * h), wj[ks], z);
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
        // ---- 5: the column sums from the fp32 dZ, then dZ rounded and packed, G_W1[:, block] += X^T dZ ----
        if (owner) {
            uint4 dz[2];
#pragma unroll
            for (int s2 = 0; s2 < 2; s2++) {
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const int r = 8 * s2 + e;
                    const float g = gs[c_row(r, h)];
                    gw2 = fmaf(g, a[r], gw2);
                    v[e] = (g * w2j) * (z[r] > 0.f ? 1.f : kLinkMlpSlope);
                    gb1 += v[e];
                }
                dz[s2] = make_uint4(bf16_pair(v[0], v[1]), bf16_pair(v[2], v[3]), bf16_pair(v[4], v[5]), bf16_pair(v[6], v[7]));
            }
#pragma unroll
            for (int cb = 0; cb < DB; cb++)
#pragma unroll
                for (int s2 = 0; s2 < 2; s2++)
                    accW[cb] = B16_MFMA(*reinterpret_cast<const uint4 *>(XTs + (32 * cb + l31) * LDT + 16 * s2 + 8 * h), dz[s2], accW[cb]);
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

MGGCN_API size_t mggcn_link_mlp_image_halves(uint32_t d, uint32_t hd) {
    return link_mlp_image_halves(d, hd);
}

MGGCN_API void mggcn_link_mlp_pack_bf16(mggcn_stream_t stream, const float *W1, uint32_t d, uint32_t hd, uint16_t *image) {
    require_mlp_shape(d, hd);
    MGGCN_REQUIRE(W1 != nullptr && image != nullptr, "link mlp pack: null operand");
    MGGCN_REQUIRE((reinterpret_cast<uintptr_t>(image) & 15u) == 0, "link mlp bf16: the W1 image must be 16-byte aligned");
    MGGCN_REQUIRE(!overlap(image, link_mlp_image_halves(d, hd) * 2, W1, (size_t)d * hd * 4), "link mlp pack: the image must not overlap W1");
    hipLaunchKernelGGL(link_mlp_pack_kernel, dim3((d * hd + 255) / 256), dim3(256), 0, as_stream(stream), W1, d, hd, image);
    MGGCN_CHECK_LAUNCH();
}

MGGCN_API void mggcn_link_mlp_loss_bf16(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                        const uint32_t *indices, size_t nnz, const uint16_t *Hb, size_t ldhb, uint32_t d,
                                        const uint16_t *image, const float *b1, const float *w2, const float *b2, uint32_t hd,
                                        int positive, float weight, uint32_t R, float neg_weight, uint64_t seed, uint32_t epoch,
                                        float beta, float *G, size_t ldg, float *row_loss, uint32_t *row_correct) {
    if (!require_walk({Hb, ldhb, 2, image}, n_rows, n_cols, indptr, indices, nnz, d, hd, b1, w2, b2, R, G, ldg, row_loss, row_correct))
        return;
    const bool vec = rows16(G, ldg);
    const unsigned grid = (unsigned)std::min<size_t>(((size_t)n_rows + 3) / 4, kLinkMlpWalkGrid);
    mlp_dispatch(d, hd, [&](auto db, auto hb) {
        hipLaunchKernelGGL((link_mlp_loss_b16_kernel<db.value, hb.value>), dim3(grid), dim3(256), 0, as_stream(stream), n_rows,
                           indptr, indices, Hb, ldhb, image, b1, w2, b2, positive != 0, weight, nnz ? R : 0u, neg_weight, n_cols,
                           (uint32_t)(seed & 0xFFFFFFFFull), (uint32_t)(seed >> 32), epoch, beta, G, ldg, vec, row_loss, row_correct);
        MGGCN_CHECK_LAUNCH();
    });
}

MGGCN_API void mggcn_link_mlp_pairs_bf16(mggcn_stream_t stream, const uint32_t *src, const uint32_t *dst, size_t m,
                                         const uint32_t *head, const uint32_t *indices, size_t M, uint32_t R, uint32_t n_draw,
                                         uint64_t seed, uint32_t epoch, int positive, float weight, float neg_weight,
                                         const uint16_t *Hb, size_t ldhb, size_t n_rows, uint32_t d, const uint16_t *image,
                                         const float *b1, const float *w2, const float *b2, uint32_t hd, float *out, float *grads,
                                         float *partials) {
    m = require_pairs({Hb, ldhb, 2, image}, src, dst, m, head, indices, M, R, n_draw, n_rows, d, hd, b1, w2, b2, out, grads,
                      partials, mggcn_link_mlp_partial_floats(d, hd));
    const hipStream_t st = as_stream(stream);
    unsigned grid = 0;
    if (m) {
        grid = (unsigned)std::min<size_t>((m + 31) / 32, kLinkMlpPairsGrid);
        mlp_dispatch(d, hd, [&](auto db, auto hb) {
            hipLaunchKernelGGL((link_mlp_pairs_b16_kernel<db.value, hb.value>), dim3(grid), dim3(256), 0, st, src, dst, m, head,
                               indices, R, n_draw, (uint32_t)(seed & 0xFFFFFFFFull), (uint32_t)(seed >> 32), epoch, positive != 0,
                               weight, neg_weight, Hb, ldhb, image, b1, w2, b2, out, partials);
            MGGCN_CHECK_LAUNCH();
        });
    }
    if (grads != nullptr) pairs_final(st, partials, grid, d, hd, grads);
}
