// link_rank.hip -- the ranking metrics of the link head (include/mggcn.h, "link prediction, ranking"): for every positive pair
// i the two integers greater[i] = #{negatives of i: s_neg > s_i} and equal[i] = #{s_neg == s_i}, counts[2 i] and
// counts[2 i + 1], from which the host forms MRR and Hits@K.  No score is stored.  No reference counterpart.  No atomics, no
// scratch; only integers are summed, so no result depends on an order.  A NaN compares false both ways: a NaN negative is
// counted nowhere, a NaN positive gets (0, 0); the sorted path ranks a NaN where sort_key.h puts its bit pattern.
//
// link_rank_dot_kernel -- per-positive tails, the dot decoder.  link_dot_loss_kernel's layout (link.hip, gat_internal.h)
// without its gradient: one wave per positive, H[src[i]] in registers, the positive's tail scored first (by every group: the
// same bits on every lane), then the K tails of row i walked by entry_chunks over tails + i K, a lane group owning one entry
// at a time, float4 or element gathers, the butterfly group_sum.  Every lane of a group holds the same score and counts in
// lane; fold_groups_u32 adds one lane of each group and lane 0 stores the pair.  No axpy and no accumulator rows: the registers
// the loss walk spends on acc go to a deeper unroll (rank_unroll: U gathers of a group in flight).  A score is
// group_sum(dot_head_row(H[u], H[v])) on the geometry of head_geometry_for, exactly mggcn_edge_dot_f32's expression: the same
// bits, whatever group or step scores the pair.
//
// link_rank_mlp_kernel / link_rank_mlp_b16_kernel -- per-positive tails, the MLP decoder, forward only.  The walk kernels'
// tile (link_mlp.hip, link_mlp_b16.hip): a persistent grid, W1 in LDS once per workgroup, one wave per positive, H[u] in a
// per-wave LDS strip, 32 pairs per tile with lane = (pair t, half h), Z^T [hd x 32] = W1^T X^T in the accumulators with
// x = H[u] (.) H[y_t] as the B operand, the score summed in lane.  The list of a positive is its own tail followed by its K
// tails: entry 0 of tile 0 is the positive, its score is broadcast from lane 0, and the counts are population counts of
// ballots over the half h = 0 of the tile's valid lanes.  The next tile's indices are loaded before the current tile's
// products.  To give a pair the bits mggcn_link_mlp_pairs_f32 / _bf16 give it, both kernels follow the PAIR kernels' sums, not
// the walks':
//   z     fp32: k-step kk holds the columns 2 kk (h = 0) and 2 kk + 1 (h = 1), as the pair kernel's Z = X W1 has them.  A lane
//         loads the 16 bytes at 8 g + 4 h of every 8 columns (the walk's loads), forms its four products and trades two of
//         them with lane ^ 32: h = 0 ends with the even columns, h = 1 with the odd ones.
//         bf16: the walk's own slots (slot e of half h in step s is column 16 s + 8 (e / 4) + 4 h + e % 4) are the pair
//         kernel's; nothing is traded.
//   s     the pair kernel adds w2_j a_j over the 32 hidden units of a block by half_dot (link_mlp_internal.h): four DPP
//         rotations inside each row of 16 lanes and one exchange between the rows; it stores what lane 0 holds, then adds the
//         blocks in order, then b2.  half_dot's first step is written as an fma: lane l holds
//         fma(w2_l, a_l, rnd(w2_(l^8) a_(l^8))), so the lanes of a row do not hold the same bits and lane 0's tree is the sum
//         over the units 0, 12, 14, 10, 15, 11, 13, 9 of those terms, in that shape.  Here row i of the A operand holds hidden
//         unit pi(i) = i with bits 2 and 4 swapped (W1, b1 and w2 are permuted as they are staged), so a lane half holds 16
//         consecutive units of a block in its own registers: that tree is spelled out in lane, with contraction off as in
//         half_dot, and the two rows meet in one exchange with lane ^ 32.
//
// link_rank_sorted_kernel -- the shared list.  The negatives' scores, as sort_key.h keys sorted ascending by
// mggcn_radix_sort_pairs_u32, and per positive one lower-bound and one upper-bound bisection on its own key:
// greater = m_neg - upper, equal = upper - lower.
#include "gat_internal.h"
#include "link_mlp_internal.h"
#include "sort_key.h"

namespace {

// ---------------------------------------------------------------- the dot decoder
// gathers of one group in flight: z[U][NT][VEC] is at most 64 registers (the loss walk holds acc as well and stops at 16)
template <int VEC, int NT>
constexpr int rank_unroll() { return VEC * NT <= 4 ? 8 : 4; }

template <int VEC, int NT, int U>
__global__ __launch_bounds__(256) void link_rank_dot_kernel(uint32_t m, const uint32_t *__restrict__ src,
                                                            const uint32_t *__restrict__ dst,
                                                            const uint32_t *__restrict__ tails, uint32_t K,
                                                            const float *__restrict__ H, size_t ldh, uint32_t d, uint32_t lg,
                                                            uint32_t *__restrict__ counts) {
    MGGCN_GAT_WAVE_ROW(m);
    float h[NT][VEC];
    load_head_row<VEC, NT>(h, H + (size_t)src[row] * ldh, lpr, sub, d);
    float s_pos;
    {
        float z[NT][VEC];
        load_head_row<VEC, NT>(z, H + (size_t)dst[row] * ldh, lpr, sub, d);
        s_pos = group_sum(dot_head_row<VEC, NT>(h, z), lpr);
    }
    uint32_t gt = 0, eq = 0;                    // of my group: every lane of a group holds the same numbers

    const uint32_t *__restrict__ mine = tails + row * K;
    entry_chunks<0> ch;
    ch.start(mine, 0, K, lane, no_scalars);
    for (uint32_t base = 0; base < K; base += 64) {
        ch.next(mine, base, K, lane, no_scalars);
        for (uint32_t j = 0; j < ch.cnt; j += n_grp * U) {
            float p[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const chunk_entry e = ch.pick(j, u, n_grp, grp);
                float z[NT][VEC];
                ok[u] = e.ok;
                load_head_row<VEC, NT>(z, H + (size_t)e.c * ldh, lpr, sub, d, e.ok);
                p[u] = dot_head_row<VEC, NT>(h, z);
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const float s = group_sum(p[u], lpr);
                gt += ok[u] && s > s_pos ? 1u : 0u;
                eq += ok[u] && s == s_pos ? 1u : 0u;
            }
        }
    }
    gt = fold_groups_u32(gt, lpr);
    eq = fold_groups_u32(eq, lpr);
    if (lane == 0) *reinterpret_cast<uint2 *>(counts + 2 * row) = make_uint2(gt, eq);
}

// ---------------------------------------------------------------- the MLP decoder
__host__ __device__ __forceinline__ constexpr uint32_t pi32(uint32_t i) { return (i & ~20u) | ((i & 4u) << 2) | ((i & 16u) >> 2); }

// the register of a lane that holds unit 16 h + l of a block: c_row(r, h) = pi32(16 h + l)
__device__ __forceinline__ constexpr int rank_reg(int l) { return (l & 3) | ((l & 4) << 1) | ((l & 8) >> 1); }

// the score of my lane's pair from Z^T in the C layout, with the bits of the pair kernels' sum (the file's text); w2s is
// staged in row order: w2s[32 jb + i] = w2[32 jb + pi32(i)]
template <int HB>
__device__ __forceinline__ float rank_score(const f32x16 (&z)[HB], const float *w2s, uint32_t h, float b2) {
#pragma clang fp contract(off)
    float s = 0.f;
#pragma unroll
    for (int jb = 0; jb < HB; jb++) {
        float w[16], a[16], q[16];                              // by unit l of my 16: register rank_reg(l)
#pragma unroll
        for (int l = 0; l < 16; l++) {
            w[l] = w2s[32 * jb + c_row(rank_reg(l), h)];
            a[l] = gat_lrelu(z[jb][rank_reg(l)], kLinkMlpSlope);
            q[l] = w[l] * a[l];
        }
        // lane 0 of a 16-lane row after row_ror 8, 4, 2, 1 (lane l takes lane l - n): the units 0, 12, 14, 10, 15, 11, 13, 9,
        // each entering as fma(w2 a, its partner's rounded product) -- half_dot's first step
        const auto v = [&](int l) { return fmaf(w[l], a[l], q[l ^ 8]); };
        float p = ((v(0) + v(12)) + (v(14) + v(10))) + ((v(15) + v(11)) + (v(13) + v(9)));
        p = p + __shfl_xor(p, 32);                              // lane 16 of the pair kernel: my other half
        s = jb == 0 ? p : s + p;
    }
    return s + b2;
}

// entry e of positive `row`'s list: its own tail, then its K tails
__device__ __forceinline__ uint32_t rank_entry(const uint32_t *__restrict__ dst, const uint32_t *__restrict__ tails, size_t row,
                                               uint32_t K, uint32_t e) {
    if (e == 0) return dst[row];
    return e <= K ? tails[row * K + (e - 1)] : 0u;
}

// the counts of one tile: lanes of half 0 whose entry exists and is not the positive itself; wave-uniform
__device__ __forceinline__ void rank_count(float s, float s_pos, bool live, uint32_t &gt, uint32_t &eq) {
    gt += (uint32_t)__popcll(__ballot(live && s > s_pos));
    eq += (uint32_t)__popcll(__ballot(live && s == s_pos));
}

template <int DB, int HB>
__global__ __launch_bounds__(256) void link_rank_mlp_kernel(uint32_t m, const uint32_t *__restrict__ src,
                                                            const uint32_t *__restrict__ dst,
                                                            const uint32_t *__restrict__ tails, uint32_t K,
                                                            const float *__restrict__ H, size_t ldh, bool vec,
                                                            const float *__restrict__ W1, const float *__restrict__ b1,
                                                            const float *__restrict__ w2, const float *__restrict__ b2p,
                                                            uint32_t *__restrict__ counts) {
    constexpr int D = 32 * DB, HD = 32 * HB;
    __shared__ __attribute__((aligned(16))) float W1s[D * HD];      // W1s[c][32 jb + i] = W1[c][32 jb + pi32(i)]
    __shared__ float b1s[HD], w2s[HD];
    __shared__ __attribute__((aligned(16))) float hxs[4][D];
    for (int i = threadIdx.x; i < D * HD; i += 256) W1s[i] = W1[(i & ~31) | (int)pi32(i & 31)];
    if (threadIdx.x < HD) {
        const uint32_t j = (threadIdx.x & ~31u) | pi32(threadIdx.x & 31u);
        b1s[threadIdx.x] = b1[j];
        w2s[threadIdx.x] = w2[j];
    }
    __syncthreads();
    const float b2 = *b2p;
    const uint32_t lane = threadIdx.x & 63, t = lane & 31, h = lane >> 5;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float *hx = hxs[wave];

    for (size_t row = (size_t)blockIdx.x * 4 + wave; row < m; row += (size_t)gridDim.x * 4) {
        __builtin_amdgcn_wave_barrier();            // the strip's readers of the row before are done (one wave, in order)
        const float *hu = H + (size_t)src[row] * ldh;
        for (uint32_t c = lane; c < D; c += 64) hx[c] = hu[c];
        __builtin_amdgcn_wave_barrier();
        uint32_t gt = 0, eq = 0;
        float s_pos = 0.f;
        uint32_t c_next = rank_entry(dst, tails, row, K, t);
        for (uint32_t e0 = 0; e0 <= K; e0 += 32) {
            const uint32_t c_t = c_next;
            const bool ok = e0 + t <= K;
            c_next = rank_entry(dst, tails, row, K, e0 + 32 + t);
            // ---- my columns 32 b + 8 q + 4 h + i of H[y_t] ----
            float y[DB][4][4];
            const float *yp = H + (size_t)c_t * ldh + 4 * h;
#pragma unroll
            for (int b = 0; b < DB; b++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if (ok) load4(y[b][q], yp + 32 * b + 8 * q, vec);
                    else y[b][q][0] = y[b][q][1] = y[b][q][2] = y[b][q][3] = 0.f;
                }
            // ---- z = b1 + W1^T x, the columns in the pair kernel's order ----
            f32x16 z[HB];
#pragma unroll
            for (int jb = 0; jb < HB; jb++)
#pragma unroll
                for (int r = 0; r < 16; r++) z[jb][r] = b1s[32 * jb + c_row(r, h)];
#pragma unroll
            for (int b = 0; b < DB; b++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const float4 hx4 = *reinterpret_cast<const float4 *>(hx + 32 * b + 8 * q + 4 * h);
                    const float x[4] = {hx4.x * y[b][q][0], hx4.y * y[b][q][1], hx4.z * y[b][q][2], hx4.w * y[b][q][3]};
                    // half 0 holds columns 0 .. 3 of the eight and keeps 0 and 2, half 1 holds 4 .. 7 and keeps 5 and 7
                    const float r0 = __shfl_xor(h ? x[0] : x[1], 32), r1 = __shfl_xor(h ? x[2] : x[3], 32);
                    const float xk[4] = {h ? r0 : x[0], h ? r1 : x[2], h ? x[1] : r0, h ? x[3] : r1};
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const float *wrow = W1s + (32 * b + 8 * q + 2 * i + h) * HD + t;
#pragma unroll
                        for (int jb = 0; jb < HB; jb++) z[jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(wrow[32 * jb], xk[i], z[jb], 0, 0, 0);
                    }
                    MLP_SCHED_FENCE();
                }
            const float s = rank_score<HB>(z, w2s, h, b2);
            if (e0 == 0) s_pos = __shfl(s, 0);
            rank_count(s, s_pos, ok && h == 0 && e0 + t != 0, gt, eq);
        }
        if (lane == 0) *reinterpret_cast<uint2 *>(counts + 2 * row) = make_uint2(gt, eq);
    }
}

template <int DB, int HB>
__global__ __launch_bounds__(256) void link_rank_mlp_b16_kernel(uint32_t m, const uint32_t *__restrict__ src,
                                                                const uint32_t *__restrict__ dst,
                                                                const uint32_t *__restrict__ tails, uint32_t K,
                                                                const uint16_t *__restrict__ Hb, size_t ldhb,
                                                                const uint16_t *__restrict__ image, const float *__restrict__ b1,
                                                                const float *__restrict__ w2, const float *__restrict__ b2p,
                                                                uint32_t *__restrict__ counts) {
    constexpr int D = 32 * DB, HD = 32 * HB, LDF = D + kPad, ROW16 = LDF / 8;
    __shared__ __attribute__((aligned(16))) uint16_t Fs[HD * LDF];      // row 32 jb + i = row 32 jb + pi32(i) of the image's F
    __shared__ float b1s[HD], w2s[HD];
    __shared__ __attribute__((aligned(16))) float hxs[4][D];
    for (int i = threadIdx.x; i < HD * ROW16; i += 256) {
        const int r = i / ROW16, c = i % ROW16;
        reinterpret_cast<uint4 *>(Fs)[i] = reinterpret_cast<const uint4 *>(image)[((r & ~31) | (int)pi32(r & 31)) * ROW16 + c];
    }
    if (threadIdx.x < HD) {
        const uint32_t j = (threadIdx.x & ~31u) | pi32(threadIdx.x & 31u);
        b1s[threadIdx.x] = b1[j];
        w2s[threadIdx.x] = w2[j];
    }
    __syncthreads();
    const float b2 = *b2p;
    const uint32_t lane = threadIdx.x & 63, t = lane & 31, h = lane >> 5;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float *hx = hxs[wave];

    for (size_t row = (size_t)blockIdx.x * 4 + wave; row < m; row += (size_t)gridDim.x * 4) {
        __builtin_amdgcn_wave_barrier();            // the strip's readers of the row before are done (one wave, in order)
        const uint16_t *hu = Hb + (size_t)src[row] * ldhb;
        for (uint32_t c = 2 * lane; c < D; c += 128) {
            const uint32_t p = *reinterpret_cast<const uint32_t *>(hu + c);
            hx[c] = widen_lo(p);
            hx[c + 1] = widen_hi(p);
        }
        __builtin_amdgcn_wave_barrier();
        uint32_t gt = 0, eq = 0;
        float s_pos = 0.f;
        uint32_t c_next = rank_entry(dst, tails, row, K, t);
        for (uint32_t e0 = 0; e0 <= K; e0 += 32) {
            const uint32_t c_t = c_next;
            const bool ok = e0 + t <= K;
            c_next = rank_entry(dst, tails, row, K, e0 + 32 + t);
            // ---- my columns 32 b + 8 q + 4 h + i of Hb[y_t], packed ----
            uint2 y[DB][4];
            const uint16_t *yp = Hb + (size_t)c_t * ldhb + 4 * h;
#pragma unroll
            for (int b = 0; b < DB; b++)
#pragma unroll
                for (int q = 0; q < 4; q++)
                    y[b][q] = ok ? *reinterpret_cast<const uint2 *>(yp + 32 * b + 8 * q) : make_uint2(0u, 0u);
            // ---- z = b1 + W1b^T x, x rounded as it is formed ----
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
                        z[jb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                            __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(wrow + 32 * jb * LDF)),
                            __builtin_bit_cast(bf16x8, x), z[jb], 0, 0, 0);
                    MLP_SCHED_FENCE();
                }
            const float s = rank_score<HB>(z, w2s, h, b2);
            if (e0 == 0) s_pos = __shfl(s, 0);
            rank_count(s, s_pos, ok && h == 0 && e0 + t != 0, gt, eq);
        }
        if (lane == 0) *reinterpret_cast<uint2 *>(counts + 2 * row) = make_uint2(gt, eq);
    }
}

// ---------------------------------------------------------------- the shared list
__global__ __launch_bounds__(256) void link_rank_sorted_kernel(const float *__restrict__ pos_scores, uint32_t m,
                                                               const uint32_t *__restrict__ keys, uint32_t m_neg,
                                                               uint32_t *__restrict__ counts) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const uint32_t key = sortable_key(pos_scores[i]);
    uint32_t lo = 0, hi = m_neg;                // lower bound: keys[j] < key for j < lo, >= key for j >= hi
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    const uint32_t lower = lo;
    hi = m_neg;                                 // upper bound, from the lower one on: keys[j] <= key for j < lo
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] <= key) lo = mid + 1;
        else hi = mid;
    }
    *reinterpret_cast<uint2 *>(counts + 2 * i) = make_uint2(m_neg - lo, lo - lower);
}

// what every per-positive entry asks of its lists
void require_rank_lists(const char *what, size_t m, uint32_t K, const uint32_t *src, const uint32_t *dst, const uint32_t *tails,
                        const uint32_t *counts, size_t n_rows) {
    MGGCN_REQUIRE(m < ((size_t)1 << 31) && m * (K ? K : 1) < ((size_t)1 << 31), what);
    MGGCN_REQUIRE(src != nullptr && dst != nullptr && counts != nullptr && n_rows != 0 && (K == 0 || tails != nullptr), what);
    MGGCN_REQUIRE((reinterpret_cast<uintptr_t>(counts) & 7u) == 0, "link rank: counts must be 8-byte aligned");
    const size_t c_bytes = m * 8;
    MGGCN_REQUIRE(!overlap(counts, c_bytes, src, m * 4) && !overlap(counts, c_bytes, dst, m * 4) &&
                      !overlap(counts, c_bytes, tails, m * K * 4),
                  "link rank: counts must not overlap a list");
}

// the MLP entries; false: there is nothing to launch
bool require_rank_mlp(const mlp_inputs &in, const uint32_t *src, const uint32_t *dst, size_t m, const uint32_t *tails, uint32_t K,
                      size_t n_rows, uint32_t d, uint32_t hd, const float *b1, const float *w2, const float *b2,
                      const uint32_t *counts) {
    require_mlp_shape(d, hd);
    MGGCN_REQUIRE(in.ldh >= d, "link rank: leading dimension < d");
    if (!m) return false;
    require_rank_lists("link rank mlp: null operand, or m K >= 2^31", m, K, src, dst, tails, counts, n_rows);
    MGGCN_REQUIRE(in.H != nullptr && in.W != nullptr && b1 != nullptr && w2 != nullptr && b2 != nullptr, "link rank mlp: null operand");
    require_images(in);
    MGGCN_REQUIRE(!overlap(counts, m * 8, in.H, in.h_bytes(n_rows, d)) && !overlap(counts, m * 8, in.W, in.w_bytes(d, hd)),
                  in.image() ? "link rank: counts must not overlap Hb or the image" : "link rank: counts must not overlap H or W1");
    return true;
}

}  // namespace

MGGCN_API void mggcn_link_rank_dot_f32(mggcn_stream_t stream, const uint32_t *src, const uint32_t *dst, size_t m,
                                       const uint32_t *tails, uint32_t K, const float *H, size_t ldh, size_t n_rows, uint32_t d,
                                       uint32_t *counts) {
    MGGCN_REQUIRE(d >= 1 && d <= MGGCN_GAT_MAX_WIDTH, "link rank: the embedding width must be 1 <= d <= 1024");
    MGGCN_REQUIRE(ldh >= d, "link rank: leading dimension < d");
    if (!m) return;
    require_rank_lists("link rank dot: null operand, or m K >= 2^31", m, K, src, dst, tails, counts, n_rows);
    MGGCN_REQUIRE(H != nullptr, "link rank dot: null operand");
    MGGCN_REQUIRE(!overlap(counts, m * 8, H, matrix_bytes(n_rows, ldh, d)), "link rank: counts must not overlap H");
    const bool vec = d % 4 == 0 && rows16(H, ldh);              // mggcn_edge_dot_f32's rule: the same path, the same bits
    const head_geometry hg = head_geometry_for(d, vec);
    gat_dispatch(vec, hg.nt, [&](auto v) {
        launch_rows(link_rank_dot_kernel<v.VEC, v.NT, rank_unroll<v.VEC, v.NT>()>, m, stream, (uint32_t)m, src, dst, tails, K, H,
                    ldh, d, hg.lg, counts);
    });
}

MGGCN_API void mggcn_link_rank_mlp_f32(mggcn_stream_t stream, const uint32_t *src, const uint32_t *dst, size_t m,
                                       const uint32_t *tails, uint32_t K, const float *H, size_t ldh, size_t n_rows, uint32_t d,
                                       const float *W1, const float *b1, const float *w2, const float *b2, uint32_t hd,
                                       uint32_t *counts) {
    if (!require_rank_mlp({H, ldh, 4, W1}, src, dst, m, tails, K, n_rows, d, hd, b1, w2, b2, counts)) return;
    const bool vec = rows16(H, ldh);
    const unsigned grid = (unsigned)std::min<size_t>((m + 3) / 4, kLinkMlpWalkGrid);
    mlp_dispatch(d, hd, [&](auto db, auto hb) {
        hipLaunchKernelGGL((link_rank_mlp_kernel<db.value, hb.value>), dim3(grid), dim3(256), 0, as_stream(stream), (uint32_t)m,
                           src, dst, tails, K, H, ldh, vec, W1, b1, w2, b2, counts);
        MGGCN_CHECK_LAUNCH();
    });
}

MGGCN_API void mggcn_link_rank_mlp_bf16(mggcn_stream_t stream, const uint32_t *src, const uint32_t *dst, size_t m,
                                        const uint32_t *tails, uint32_t K, const uint16_t *Hb, size_t ldhb, size_t n_rows,
                                        uint32_t d, const uint16_t *image, const float *b1, const float *w2, const float *b2,
                                        uint32_t hd, uint32_t *counts) {
    if (!require_rank_mlp({Hb, ldhb, 2, image}, src, dst, m, tails, K, n_rows, d, hd, b1, w2, b2, counts)) return;
    const unsigned grid = (unsigned)std::min<size_t>((m + 3) / 4, kLinkMlpWalkGrid);
    mlp_dispatch(d, hd, [&](auto db, auto hb) {
        hipLaunchKernelGGL((link_rank_mlp_b16_kernel<db.value, hb.value>), dim3(grid), dim3(256), 0, as_stream(stream),
                           (uint32_t)m, src, dst, tails, K, Hb, ldhb, image, b1, w2, b2, counts);
        MGGCN_CHECK_LAUNCH();
    });
}

MGGCN_API void mggcn_link_rank_sorted_u32(mggcn_stream_t stream, const float *pos_scores, size_t m, const uint32_t *sorted_keys,
                                          size_t m_neg, uint32_t *counts) {
    MGGCN_REQUIRE(m < ((size_t)1 << 31) && m_neg < ((size_t)1 << 31), "link rank sorted: both lists must be shorter than 2^31");
    if (!m) return;
    MGGCN_REQUIRE(pos_scores != nullptr && counts != nullptr && (m_neg == 0 || sorted_keys != nullptr), "link rank sorted: null operand");
    MGGCN_REQUIRE((reinterpret_cast<uintptr_t>(counts) & 7u) == 0, "link rank: counts must be 8-byte aligned");
    MGGCN_REQUIRE(!overlap(counts, m * 8, pos_scores, m * 4) && !overlap(counts, m * 8, sorted_keys, m_neg * 4),
                  "link rank sorted: counts must not overlap an input");
    hipLaunchKernelGGL(link_rank_sorted_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, as_stream(stream), pos_scores,
                       (uint32_t)m, sorted_keys, (uint32_t)m_neg, counts);
    MGGCN_CHECK_LAUNCH();
}
