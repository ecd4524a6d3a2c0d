// gat.hip -- graph attention (GAT) on gfx950: attention scores, the edge-softmax fused with the gather, and the
// backward pass (per-edge dot products + weighted transposed gather + the column sums behind G_att).
//
// Layout of the three sparse kernels: the row-split form of spmm.hip without a plan -- one wave per CSR row, the row's
// entries in 64-entry chunks, software-pipelined (entry_chunks of gat_internal.h is the walk).  The heads of a row are
// walked one after the other.  Within a head the wave is cut into G = 64 / LPR groups of LPR lanes (LPR: the power of two
// that covers one head's dh columns, 64 at the most): a group holds one head-row of a dense operand, VEC columns per lane
// and NT column tiles when dh > LPR * VEC, so one wave-instruction gathers the head-rows of G neighbours.
//   * per chunk, the lane that owns an entry has its index and its [rows x K] scalars (scores, lse, D) from the walk and
//     evaluates exp ONCE per (entry, head); the groups pick index and weight up through ds_bpermute (chunk_entry);
//   * the forward makes ONE pass over a row: a running maximum, the sum and the accumulators rescaled chunk by chunk;
//   * the per-edge dot product (SDDMM) is a butterfly over the LPR lanes of a group -- log2(LPR) steps per G edges;
//   * the sums over a row's entries fold the G groups in a fixed order at the end: no atomics anywhere, the same bits on
//     every call.
// No per-edge array exists: alpha is recomputed from s_dst, s_src and lse wherever it is needed.  The one exception is on
// request: gat_alpha_kernel (mggcn_gat_alpha_f32) runs the same walk and writes alpha out for the user; nothing reads it back.
// VEC = 4 (16-byte loads) when dh % 4 == 0 and every dense operand and leading dimension is 16-byte aligned -- a float4
// must not straddle two heads, so K * dh % 4 == 0 alone is not enough -- and VEC = 1 otherwise.
// Heavy rows are slow here (one wave walks a whole row, ~21 k entries on the Reddit-shaped graph) but correct: cutting
// them with a fixed-order combine is what the SpMM's plan does and is left to a plan for these kernels.
// Attention dropout (DROP = true, the mggcn_gat_*_drop_f32 entry points): the lane that owns an entry draws its keep bit
// from Philox on (source, destination, head) next to the exp, and the factor q = keep ? 1 / (1 - p) : 0 travels to the
// groups through the same __shfl as the weight.  The softmax itself (maximum, sum, lse) takes every entry.  Nothing is
// stored: the backward kernels draw the same words again, backward_src with the roles of row and entry swapped.  Duplicate
// entries (i, j) share one bit.  DROP = false compiles to the kernels as they were.
// The packed destination record (REC = true, the mggcn_gat_backward_src_rec*_f32 entry points): backward_src reads (s_dst,
// lse, D) of an entry's destination as ONE 16-byte load from rec[(i K + k) 4 + {0, 1, 2}] (gat_pack_dst_kernel writes it; the
// fourth float is padding nobody reads) where the plain kernel gathers three 4-byte scalars.  Only the loads differ: the
// arithmetic, and so every bit of ds_src and G_Z, is the plain kernel's.  REC = false compiles to the kernels as they were.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "gat_internal.h"
#include "philox.h"
#include "reduce.h"

namespace {

// what a DROP kernel needs to draw the mask: threshold = floor(p 2^32), scale = fp32(1 / (1 - p)), the key (seed low, seed
// high), the dropout stream and the global indices of the call's first destination and first source
struct gat_drop {
    uint32_t threshold;
    float scale;
    uint32_t k0, k1, stream, dst0, src0;
};

// q of entry (global destination i, global source j, head k): word k & 3 of Philox(counter = (j, i, 2^31 | k >> 2, stream)).
// The set top bit of the third word keeps these counters apart from mggcn_dropout_f32's (row >> 32 there) under one
// (seed, stream).  k is wave-uniform, so the word is picked by selects on a scalar condition.
__device__ __forceinline__ float gat_keep_scale(const gat_drop &dp, uint32_t i, uint32_t j, uint32_t k) {
    const philox4 r = philox4x32_10(j, i, 0x80000000u | (k >> 2), dp.stream, dp.k0, dp.k1);
    const uint32_t word = (k & 2) ? ((k & 1) ? r.w[3] : r.w[2]) : ((k & 1) ? r.w[1] : r.w[0]);
    return word >= dp.threshold ? dp.scale : 0.f;
}

// ---------------------------------------------------------------------------
// s_dst[r, k] = Z[r, head k] . att[0, head k],  s_src[r, k] = Z[r, head k] . att[1, head k]
// one wave per row, G heads at a time (one per group)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gat_scores_kernel(const float *__restrict__ Z, size_t ldz, const float *__restrict__ att,
                                                         float *__restrict__ s_dst, float *__restrict__ s_src, size_t n_rows,
                                                         uint32_t K, uint32_t dh, uint32_t lg) {
    MGGCN_GAT_WAVE_ROW(n_rows);
    const float *__restrict__ z = Z + row * ldz;
    const uint32_t width = K * dh;
    for (uint32_t k0 = 0; k0 < K; k0 += n_grp) {
        const uint32_t k = k0 + grp;
        float pd = 0.f, ps = 0.f;
        if (k < K)
            for (uint32_t c = sub; c < dh; c += lpr) {
                const float v = z[k * dh + c];
                pd = fmaf(v, att[k * dh + c], pd);
                ps = fmaf(v, att[width + k * dh + c], ps);
            }
        pd = group_sum(pd, lpr);
        ps = group_sum(ps, lpr);
        if (k < K && sub == 0) {
            if (s_dst) s_dst[row * K + k] = pd;
            if (s_src) s_src[row * K + k] = ps;
        }
    }
}

// ---------------------------------------------------------------------------
// forward: lse[i, k] and out[i, head k] = sum_j alpha_ijk Z[j, head k] over the entries j of row i
// ---------------------------------------------------------------------------
// DROP: out[i, head k] = sum_j (alpha_ijk q_ijk) Z[j, head k]; lse, the maximum and the sum are those of DROP = false
template <int VEC, int NT, int U, bool DROP>
__global__ __launch_bounds__(256) void gat_forward_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                          const uint32_t *__restrict__ indices, const float *__restrict__ Z,
                                                          size_t ldz, const float *__restrict__ s_dst,
                                                          const float *__restrict__ s_src, uint32_t K, uint32_t dh, float slope,
                                                          uint32_t lg, float *__restrict__ out, size_t ldo,
                                                          float *__restrict__ lse, gat_drop dp) {
    MGGCN_GAT_WAVE_ROW(n_rows);
    const uint32_t beg = indptr[row], end = indptr[row + 1];
    for (uint32_t k = 0; k < K; k++) {
        const float sd = s_dst[row * K + k];
        const float *__restrict__ Zk = Z + (size_t)k * dh;
        // One pass over the row with a running maximum (the softmax of flash attention): per chunk, lane l owns entry l,
        // m <- max(m, the chunk's scores), the sum and the accumulators are rescaled by exp(m_old - m_new), and the chunk is
        // gathered with the weights exp(e - m).  out = acc / sum at the end: the weights of a row add up to one within
        // rounding whatever the magnitude of the scores.  The walk fetches s_src of the entry.
        float m = -INFINITY, sum = 0.f;
        float acc[NT][VEC];
        zero_head_row<VEC, NT>(acc);
        const auto fetch = [&](uint32_t c, float *s) { s[0] = s_src[(size_t)c * K + k]; };
        entry_chunks<1> ch;
        ch.start(indices, beg, end, lane, fetch);
        for (uint32_t base = beg; base < end; base += 64) {
            ch.next(indices, base, end, lane, fetch);
            const uint32_t cnt = ch.cnt;
            const float my_x = ch.my_s[0];
            const float e = lane < cnt ? gat_lrelu(sd + my_x, slope) : -INFINITY;
            const float m_new = fmaxf(m, wave_max(e));
            const float scale = expf(m - m_new);            // 0 at the first chunk (m = -inf), where sum and acc are 0
            float my_a = lane < cnt ? expf(e - m_new) : 0.f;
            sum = fmaf(sum, scale, wave_sum(my_a));
            m = m_new;
            if constexpr (DROP) {                            // after the sum: only the accumulator's weight carries q
                if (lane < cnt) my_a *= gat_keep_scale(dp, dp.dst0 + (uint32_t)row, dp.src0 + ch.my_c, k);
            }
            if (scale != 1.f) {                              // wave-uniform
#pragma unroll
                for (int t = 0; t < NT; t++)
#pragma unroll
                    for (int v = 0; v < VEC; v++) acc[t][v] *= scale;
            }
            for (uint32_t j = 0; j < cnt; j += n_grp * U) {
                float z[U][NT][VEC], a[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const chunk_entry en = ch.pick(j, u, n_grp, grp);
                    const float av = en.of(my_a);
                    a[u] = en.ok ? av : 0.f;
                    load_head_row<VEC, NT>(z[u], Zk + (size_t)en.c * ldz, lpr, sub, dh, en.ok);
                }
#pragma unroll
                for (int u = 0; u < U; u++) axpy_head_row<VEC, NT>(acc, a[u], z[u]);
            }
        }
        const float inv = beg < end ? 1.f / sum : 0.f;
        if (lane == 0) lse[row * K + k] = beg < end ? m + logf(sum) : 0.f;
        fold_store_head_row<VEC, NT>(out + row * ldo + (size_t)k * dh, acc, lpr, sub, grp, dh,
                                     [&](int, int, float x) { return x * inv; });      // an empty row: +0.0
    }
}

// ---------------------------------------------------------------------------
// backward over the rows of F:  D[i, k] = G[i, head k] . out[i, head k]
//   ds_dst[i, k] = sum_j alpha_ijk (G[i, head k] . Z[j, head k] - D[i, k]) lrelu'(x_ijk)
// ---------------------------------------------------------------------------
// DROP: ds_ijk = alpha_ijk (q_ijk dalpha_ijk - D[i, k]) lrelu'(x_ijk); D = G . out as before (out is the dropped forward's)
template <int VEC, int NT, int U, bool DROP>
__global__ __launch_bounds__(256) void gat_backward_dst_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                               const uint32_t *__restrict__ indices,
                                                               const float *__restrict__ Z, size_t ldz,
                                                               const float *__restrict__ s_dst, const float *__restrict__ s_src,
                                                               const float *__restrict__ lse, const float *__restrict__ G,
                                                               size_t ldg, const float *__restrict__ out, size_t ldo, uint32_t K,
                                                               uint32_t dh, float slope, uint32_t lg, float *__restrict__ D,
                                                               float *__restrict__ ds_dst, gat_drop dp) {
    MGGCN_GAT_WAVE_ROW(n_rows);
    const uint32_t beg = indptr[row], end = indptr[row + 1];
    for (uint32_t k = 0; k < K; k++) {
        float g[NT][VEC];
        load_head_row<VEC, NT>(g, G + row * ldg + (size_t)k * dh, lpr, sub, dh);
        const float Dk = head_row_D<VEC, NT>(g, out + row * ldo + (size_t)k * dh, lpr, sub, grp, dh);
        const float sd = s_dst[row * K + k], ls = lse[row * K + k];
        const float *__restrict__ Zk = Z + (size_t)k * dh;
        float acc = 0.f;
        const auto fetch = [&](uint32_t c, float *s) { s[0] = s_src[(size_t)c * K + k]; };      // the entry's score
        entry_chunks<1> ch;
        ch.start(indices, beg, end, lane, fetch);
        for (uint32_t base = beg; base < end; base += 64) {
            ch.next(indices, base, end, lane, fetch);
            const uint32_t cnt = ch.cnt;
            const float my_x = ch.my_s[0];
            float my_w = 0.f;                       // alpha lrelu'(x) of my entry
            [[maybe_unused]] float my_q = 0.f;
            if (lane < cnt) {
                const float x = sd + my_x;
                my_w = expf(gat_lrelu(x, slope) - ls) * (x > 0.f ? 1.f : slope);
                if constexpr (DROP) my_q = gat_keep_scale(dp, dp.dst0 + (uint32_t)row, dp.src0 + ch.my_c, k);
            }
            for (uint32_t j = 0; j < cnt; j += n_grp * U) {
                float p[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const chunk_entry en = ch.pick(j, u, n_grp, grp);
                    float z[NT][VEC];
                    load_head_row<VEC, NT>(z, Zk + (size_t)en.c * ldz, lpr, sub, dh, en.ok);
                    p[u] = dot_head_row<VEC, NT>(g, z);
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const chunk_entry en = ch.pick(j, u, n_grp, grp);
                    const float w = en.of(my_w);
                    float da = group_sum(p[u], lpr);
                    if constexpr (DROP) da *= en.of(my_q);
                    acc += en.ok ? w * (da - Dk) : 0.f;
                }
            }
        }
        acc = fold_groups(acc, lpr);                // every lane of a group holds the group's sum: one per group is added
        if (lane == 0) {
            D[row * K + k] = Dk;
            ds_dst[row * K + k] = acc;
        }
    }
}

// ---------------------------------------------------------------------------
// backward over the rows of F^T (row j lists the destinations i that gather j):
//   ds_src[j, k] = sum_i alpha_ijk (G[i, head k] . Z[j, head k] - D[i, k]) lrelu'(x_ijk)
//   G_Z[j, head k] = sum_i alpha_ijk G[i, head k] + ds_dst[j, k] att[0, head k] + ds_src[j, k] att[1, head k]
// ---------------------------------------------------------------------------
// DROP: the row is the source and the entry the destination, so the counter is (row, entry) here: the words of the forward
// REC: s_dst, lse and D are not read; the three scalars of destination i and head k come from rec + (i K + k) 4
template <int VEC, int NT, int U, bool DROP, bool REC>
__global__ __launch_bounds__(256) void gat_backward_src_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                               const uint32_t *__restrict__ indices,
                                                               const float *__restrict__ Z, size_t ldz,
                                                               const float *__restrict__ s_dst, const float *__restrict__ s_src,
                                                               const float *__restrict__ lse, const float *__restrict__ D,
                                                               const float *__restrict__ rec,
                                                               const float *__restrict__ G, size_t ldg,
                                                               const float *__restrict__ att, const float *__restrict__ ds_dst,
                                                               uint32_t K, uint32_t dh, float slope, uint32_t lg,
                                                               float *__restrict__ ds_src, float *__restrict__ G_Z, size_t ldgz,
                                                               gat_drop dp) {
    MGGCN_GAT_WAVE_ROW(n_rows);
    const uint32_t beg = indptr[row], end = indptr[row + 1];
    const uint32_t width = K * dh;
    for (uint32_t k = 0; k < K; k++) {
        float zr[NT][VEC], acc[NT][VEC];
        load_head_row<VEC, NT>(zr, Z + row * ldz + (size_t)k * dh, lpr, sub, dh);
        zero_head_row<VEC, NT>(acc);
        const float ss = s_src[row * K + k];
        const float *__restrict__ Gk = G + (size_t)k * dh;
        float acc_ds = 0.f;
        const auto fetch = [&](uint32_t c, float *s) {          // s_dst, lse and D of the entry's destination
            const size_t ik = (size_t)c * K + k;
            if constexpr (REC) {
                const float4 t = *reinterpret_cast<const float4 *>(rec + ik * 4);
                s[0] = t.x; s[1] = t.y; s[2] = t.z;
            } else {
                s[0] = s_dst[ik]; s[1] = lse[ik]; s[2] = D[ik];
            }
        };
        entry_chunks<3> ch;
        ch.start(indices, beg, end, lane, fetch);
        for (uint32_t base = beg; base < end; base += 64) {
            ch.next(indices, base, end, lane, fetch);
            const uint32_t cnt = ch.cnt;
            const float my_x = ch.my_s[0], my_l = ch.my_s[1], my_D = ch.my_s[2];
            float my_a = 0.f, my_w = 0.f;
            [[maybe_unused]] float my_q = 0.f;
            if (lane < cnt) {
                const float x = my_x + ss;
                my_a = expf(gat_lrelu(x, slope) - my_l);
                my_w = my_a * (x > 0.f ? 1.f : slope);
                if constexpr (DROP) {
                    my_q = gat_keep_scale(dp, dp.dst0 + ch.my_c, dp.src0 + (uint32_t)row, k);
                    my_a *= my_q;                   // the gather's weight alpha q; my_w keeps the plain alpha
                }
            }
            for (uint32_t j = 0; j < cnt; j += n_grp * U) {
                float gv[U][NT][VEC], p[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const chunk_entry en = ch.pick(j, u, n_grp, grp);
                    load_head_row<VEC, NT>(gv[u], Gk + (size_t)en.c * ldg, lpr, sub, dh, en.ok);
                    p[u] = dot_head_row<VEC, NT>(zr, gv[u]);
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const chunk_entry en = ch.pick(j, u, n_grp, grp);
                    const float a = en.of(my_a), w = en.of(my_w), Dv = en.of(my_D);
                    float da = group_sum(p[u], lpr);
                    if constexpr (DROP) da *= en.of(my_q);
                    acc_ds += en.ok ? w * (da - Dv) : 0.f;
                    axpy_head_row<VEC, NT>(acc, en.ok ? a : 0.f, gv[u]);
                }
            }
        }
        acc_ds = fold_groups(acc_ds, lpr);
        if (lane == 0) ds_src[row * K + k] = acc_ds;
        const float dd = ds_dst ? ds_dst[row * K + k] : 0.f;
#pragma unroll
        for (int t = 0; t < NT; t++) {
#pragma unroll
            for (int v = 0; v < VEC; v++) acc[t][v] = fold_groups(acc[t][v], lpr);
            const uint32_t col = (t * lpr + sub) * VEC;
            if (grp == 0 && col < dh) {
                float a0[VEC], a1[VEC];
                loadv<VEC>(a0, att + (size_t)k * dh + col);
                loadv<VEC>(a1, att + width + (size_t)k * dh + col);
#pragma unroll
                for (int v = 0; v < VEC; v++) acc[t][v] = fmaf(acc_ds, a1[v], fmaf(dd, a0[v], acc[t][v]));
                storev<VEC>(G_Z + row * ldgz + (size_t)k * dh + col, acc[t]);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// rec[(i K + k) 4 + {0, 1, 2, 3}] = s_dst[i, k], lse[i, k], D[i, k], 0: one thread per (destination, head), one 16-byte store
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gat_pack_dst_kernel(const float *__restrict__ s_dst, const float *__restrict__ lse,
                                                           const float *__restrict__ D, size_t n, float4 *__restrict__ rec) {
    const size_t ik = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (ik < n) rec[ik] = make_float4(s_dst[ik], lse[ik], D[ik], 0.f);
}

// ---------------------------------------------------------------------------
// the export: alpha[p, k] = exp(lrelu(s_dst[i, k] + s_src[j, k]) - lse[i, k]) for entry p = (i, j) of the indices array --
// the float expression of the two backward kernels above.  The same walk, KV heads at a time: the lane that owns an entry
// has its KV source scores from the walk and stores its KV coefficients (KV = 4: one 16-byte store).  No groups, no
// reduction, no LDS; a value depends on its entry and its row's lse alone.
// ---------------------------------------------------------------------------
template <int KV>
__global__ __launch_bounds__(256) void gat_alpha_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                        const uint32_t *__restrict__ indices,
                                                        const float *__restrict__ s_dst, const float *__restrict__ s_src,
                                                        const float *__restrict__ lse, uint32_t K, float slope,
                                                        float *__restrict__ alpha, size_t lda) {
    const uint32_t lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (row >= n_rows) return;
    const uint32_t beg = indptr[row], end = indptr[row + 1];
    for (uint32_t k0 = 0; k0 < K; k0 += KV) {
        float sd[KV], ls[KV];
#pragma unroll
        for (int v = 0; v < KV; v++) {
            sd[v] = s_dst[row * K + k0 + v];
            ls[v] = lse[row * K + k0 + v];
        }
        const auto fetch = [&](uint32_t c, float *s) {          // the entry's scores of heads k0 .. k0 + KV
#pragma unroll
            for (int v = 0; v < KV; v++) s[v] = s_src[(size_t)c * K + k0 + v];
        };
        entry_chunks<KV> ch;
        ch.start(indices, beg, end, lane, fetch);
        for (uint32_t base = beg; base < end; base += 64) {
            ch.next(indices, base, end, lane, fetch);
            if (lane < ch.cnt) {
                float a[KV];
#pragma unroll
                for (int v = 0; v < KV; v++) a[v] = expf(gat_lrelu(sd[v] + ch.my_s[v], slope) - ls[v]);
                storev<KV>(alpha + ((size_t)base + lane) * lda + k0, a);
            }
        }
    }
}

// G_att[0, c] = sum_i ds_dst[i, k(c)] Z_dst[i, c],  G_att[1, c] = sum_j ds_src[j, k(c)] Z_src[j, c]: the term of
// gat_column_sums, side 0 the destinations and side 1 the sources
struct gat_scores_term {
    const float *ds[2], *Z[2];
    size_t ld[2], n[2];
    uint32_t K, dh;
    __device__ size_t rows(int side) const { return n[side]; }
    __device__ uint32_t head(uint32_t c) const { return c / dh; }
    __device__ float operator()(int side, size_t r, uint32_t c, uint32_t k, float acc) const {
        return fmaf(ds[side][r * K + k], Z[side][r * ld[side] + c], acc);
    }
};

// the mask's operands of a _drop entry point; both index ranges of the call must fit the 32-bit counter words
gat_drop make_gat_drop(uint32_t threshold, float scale, uint64_t seed, uint32_t dropout_stream, uint32_t dst0, uint32_t n_dst,
                       uint32_t src0, uint32_t n_src) {
    MGGCN_REQUIRE((uint64_t)dst0 + n_dst <= 0x100000000ull && (uint64_t)src0 + n_src <= 0x100000000ull,
                  "gat dropout: dst0 + destinations and src0 + sources must not exceed 2^32");
    return {threshold, scale, (uint32_t)seed, (uint32_t)(seed >> 32), dropout_stream, dst0, src0};
}

// The bodies of the plain entry points and of their _drop twins: dp == nullptr launches the DROP = false kernels.
void gat_forward(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr, const uint32_t *indices,
                 const float *Z, size_t ldz, const float *s_dst, const float *s_src, uint32_t K, uint32_t dh, float slope,
                 float *out, size_t ldo, float *lse, const gat_drop *dp) {
    require_heads(K, dh);
    MGGCN_REQUIRE(ldz >= (size_t)K * dh && ldo >= (size_t)K * dh, "gat forward: leading dimension < heads * width per head");
    if (!n_rows) return;
    MGGCN_REQUIRE(indptr != nullptr && s_dst != nullptr && out != nullptr && lse != nullptr, "gat forward: null operand");
    MGGCN_REQUIRE(n_cols == 0 || (indices != nullptr && Z != nullptr && s_src != nullptr), "gat forward: null operand");
    MGGCN_REQUIRE(out != Z, "gat forward: out must not alias Z");
    const bool vec = dh % 4 == 0 && rows16(Z, ldz) && rows16(out, ldo);
    const head_geometry hg = head_geometry_for(dh, vec);
    const gat_drop d = dp ? *dp : gat_drop{};
    gat_dispatch(vec, hg.nt, [&](auto v) {
        with_flag(dp != nullptr, [&](auto drop) {
            launch_rows(gat_forward_kernel<v.VEC, v.NT, v.U, drop>, n_rows, stream, n_rows, indptr, indices, Z, ldz, s_dst, s_src,
                        K, dh, slope, hg.lg, out, ldo, lse, d);
        });
    });
}

void gat_backward_dst(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr, const uint32_t *indices,
                      const float *Z, size_t ldz, const float *s_dst, const float *s_src, const float *lse, const float *G,
                      size_t ldg, const float *out, size_t ldo, uint32_t K, uint32_t dh, float slope, float *D, float *ds_dst,
                      const gat_drop *dp) {
    require_heads(K, dh);
    const size_t width = (size_t)K * dh;
    MGGCN_REQUIRE(ldz >= width && ldg >= width && ldo >= width, "gat backward: leading dimension < heads * width per head");
    if (!n_rows) return;
    MGGCN_REQUIRE(indptr != nullptr && s_dst != nullptr && lse != nullptr && G != nullptr && out != nullptr && D != nullptr &&
                      ds_dst != nullptr,
                  "gat backward: null operand");
    MGGCN_REQUIRE(n_cols == 0 || (indices != nullptr && Z != nullptr && s_src != nullptr), "gat backward: null operand");
    const bool vec = dh % 4 == 0 && rows16(Z, ldz) && rows16(G, ldg) && rows16(out, ldo);
    const head_geometry hg = head_geometry_for(dh, vec);
    const gat_drop d = dp ? *dp : gat_drop{};
    gat_dispatch(vec, hg.nt, [&](auto v) {
        with_flag(dp != nullptr, [&](auto drop) {
            launch_rows(gat_backward_dst_kernel<v.VEC, v.NT, v.U, drop>, n_rows, stream, n_rows, indptr, indices, Z, ldz, s_dst,
                        s_src, lse, G, ldg, out, ldo, K, dh, slope, hg.lg, D, ds_dst, d);
        });
    });
}

// rec != nullptr launches the REC = true kernels, which read it in place of s_dst, lse and D (all three nullptr then)
void gat_backward_src(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                      const uint32_t *t_indices, const float *Z, size_t ldz, const float *s_dst, const float *s_src,
                      const float *lse, const float *D, const float *rec, const float *G, size_t ldg, const float *att,
                      const float *ds_dst, uint32_t K, uint32_t dh, float slope, float *ds_src, float *G_Z, size_t ldgz,
                      const gat_drop *dp) {
    require_heads(K, dh);
    const size_t width = (size_t)K * dh;
    MGGCN_REQUIRE(ldz >= width && ldg >= width && ldgz >= width, "gat backward: leading dimension < heads * width per head");
    if (!n_rows) return;
    MGGCN_REQUIRE(t_indptr != nullptr && Z != nullptr && s_src != nullptr && att != nullptr && ds_src != nullptr &&
                      G_Z != nullptr,
                  "gat backward: null operand");
    MGGCN_REQUIRE(n_cols == 0 || (t_indices != nullptr && G != nullptr &&
                                  (rec != nullptr || (s_dst != nullptr && lse != nullptr && D != nullptr))),
                  "gat backward: null operand");
    MGGCN_REQUIRE(G_Z != G && G_Z != Z, "gat backward: G_Z must not alias G or Z");
    const bool vec = dh % 4 == 0 && rows16(Z, ldz) && rows16(G, ldg) && rows16(G_Z, ldgz) && aligned16(att);
    const head_geometry hg = head_geometry_for(dh, vec);
    const gat_drop d = dp ? *dp : gat_drop{};
    gat_dispatch(vec, hg.nt, [&](auto v) {
        with_flag(dp != nullptr, [&](auto drop) {
            with_flag(rec != nullptr, [&](auto packed) {
                launch_rows(gat_backward_src_kernel<v.VEC, v.NT, v.U, drop, packed>, n_rows, stream, n_rows, t_indptr, t_indices,
                            Z, ldz, s_dst, s_src, lse, D, rec, G, ldg, att, ds_dst, K, dh, slope, hg.lg, ds_src, G_Z, ldgz, d);
            });
        });
    });
}

}  // namespace

// ============================ C ABI =========================================
MGGCN_API void mggcn_gat_scores_f32(mggcn_stream_t stream, const float *Z, size_t ldz, const float *att, float *s_dst,
                                    float *s_src, size_t n_rows, uint32_t K, uint32_t dh) {
    require_heads(K, dh);
    MGGCN_REQUIRE(ldz >= (size_t)K * dh, "gat scores: ldz < heads * width per head");
    MGGCN_REQUIRE(n_rows <= 0xFFFFFFFFu, "gat scores: more than 2^32 - 1 rows");
    if (!n_rows || (!s_dst && !s_src)) return;
    MGGCN_REQUIRE(Z != nullptr && att != nullptr, "gat scores: null operand");
    const uint32_t lg = std::min(ceil_log2(dh), 6u);
    launch_rows(gat_scores_kernel, n_rows, stream, Z, ldz, att, s_dst, s_src, n_rows, K, dh, lg);
}

MGGCN_API void mggcn_gat_forward_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                     const uint32_t *indices, const float *Z, size_t ldz, const float *s_dst,
                                     const float *s_src, uint32_t K, uint32_t dh, float slope, float *out, size_t ldo,
                                     float *lse) {
    gat_forward(stream, n_rows, n_cols, indptr, indices, Z, ldz, s_dst, s_src, K, dh, slope, out, ldo, lse, nullptr);
}

MGGCN_API void mggcn_gat_backward_dst_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                          const uint32_t *indices, const float *Z, size_t ldz, const float *s_dst,
                                          const float *s_src, const float *lse, const float *G, size_t ldg, const float *out,
                                          size_t ldo, uint32_t K, uint32_t dh, float slope, float *D, float *ds_dst) {
    gat_backward_dst(stream, n_rows, n_cols, indptr, indices, Z, ldz, s_dst, s_src, lse, G, ldg, out, ldo, K, dh, slope, D, ds_dst,
                     nullptr);
}

MGGCN_API void mggcn_gat_backward_src_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                                          const uint32_t *t_indices, const float *Z, size_t ldz, const float *s_dst,
                                          const float *s_src, const float *lse, const float *D, const float *G, size_t ldg,
                                          const float *att, const float *ds_dst, uint32_t K, uint32_t dh, float slope,
                                          float *ds_src, float *G_Z, size_t ldgz) {
    gat_backward_src(stream, n_rows, n_cols, t_indptr, t_indices, Z, ldz, s_dst, s_src, lse, D, nullptr, G, ldg, att, ds_dst, K,
                     dh, slope, ds_src, G_Z, ldgz, nullptr);
}

// The _drop twins: threshold == 0 (p = 0: every entry kept, scale = 1) launches the plain kernels, so the bits are the plain
// entry point's by construction; the index ranges are still checked.
MGGCN_API void mggcn_gat_forward_drop_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                          const uint32_t *indices, const float *Z, size_t ldz, const float *s_dst,
                                          const float *s_src, uint32_t K, uint32_t dh, float slope, float *out, size_t ldo,
                                          float *lse, uint32_t threshold, float scale, uint64_t seed, uint32_t dropout_stream,
                                          uint32_t dst0, uint32_t src0) {
    const gat_drop dp = make_gat_drop(threshold, scale, seed, dropout_stream, dst0, n_rows, src0, n_cols);
    gat_forward(stream, n_rows, n_cols, indptr, indices, Z, ldz, s_dst, s_src, K, dh, slope, out, ldo, lse,
                threshold ? &dp : nullptr);
}

MGGCN_API void mggcn_gat_backward_dst_drop_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                               const uint32_t *indices, const float *Z, size_t ldz, const float *s_dst,
                                               const float *s_src, const float *lse, const float *G, size_t ldg,
                                               const float *out, size_t ldo, uint32_t K, uint32_t dh, float slope, float *D,
                                               float *ds_dst, uint32_t threshold, float scale, uint64_t seed,
                                               uint32_t dropout_stream, uint32_t dst0, uint32_t src0) {
    const gat_drop dp = make_gat_drop(threshold, scale, seed, dropout_stream, dst0, n_rows, src0, n_cols);
    gat_backward_dst(stream, n_rows, n_cols, indptr, indices, Z, ldz, s_dst, s_src, lse, G, ldg, out, ldo, K, dh, slope, D, ds_dst,
                     threshold ? &dp : nullptr);
}

// rows of F^T are sources (offset src0), its entries destinations (offset dst0)
MGGCN_API void mggcn_gat_backward_src_drop_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                                               const uint32_t *t_indices, const float *Z, size_t ldz, const float *s_dst,
                                               const float *s_src, const float *lse, const float *D, const float *G, size_t ldg,
                                               const float *att, const float *ds_dst, uint32_t K, uint32_t dh, float slope,
                                               float *ds_src, float *G_Z, size_t ldgz, uint32_t threshold, float scale,
                                               uint64_t seed, uint32_t dropout_stream, uint32_t dst0, uint32_t src0) {
    const gat_drop dp = make_gat_drop(threshold, scale, seed, dropout_stream, dst0, n_cols, src0, n_rows);
    gat_backward_src(stream, n_rows, n_cols, t_indptr, t_indices, Z, ldz, s_dst, s_src, lse, D, nullptr, G, ldg, att, ds_dst, K,
                     dh, slope, ds_src, G_Z, ldgz, threshold ? &dp : nullptr);
}

// The packed destination record: rec[(i K + k) 4 + {0, 1, 2, 3}] = s_dst[i, k], lse[i, k], D[i, k], 0
MGGCN_API void mggcn_gat_pack_dst_f32(mggcn_stream_t stream, const float *s_dst, const float *lse, const float *D,
                                      size_t n_rows, uint32_t K, float *rec) {
    MGGCN_REQUIRE(K >= 1 && K <= MGGCN_GAT_MAX_HEADS, "gat supports 1 <= heads <= 16");
    MGGCN_REQUIRE(n_rows <= 0xFFFFFFFFu, "gat pack: more than 2^32 - 1 rows");
    if (!n_rows) return;
    MGGCN_REQUIRE(s_dst != nullptr && lse != nullptr && D != nullptr && rec != nullptr, "gat pack: null operand");
    MGGCN_REQUIRE(aligned16(rec), "gat pack: rec must be 16-byte aligned");
    const size_t n = n_rows * K;
    hipLaunchKernelGGL(gat_pack_dst_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), s_dst, lse, D, n,
                       reinterpret_cast<float4 *>(rec));
    MGGCN_CHECK_LAUNCH();
}

// backward_src on the record: rec in the place of s_dst, lse and D; the bits of the plain call on the arrays it was packed from
MGGCN_API void mggcn_gat_backward_src_rec_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                                              const uint32_t *t_indices, const float *Z, size_t ldz, const float *rec,
                                              const float *s_src, const float *G, size_t ldg, const float *att,
                                              const float *ds_dst, uint32_t K, uint32_t dh, float slope, float *ds_src,
                                              float *G_Z, size_t ldgz) {
    MGGCN_REQUIRE(!n_rows || !n_cols || (rec != nullptr && aligned16(rec)), "gat backward: rec must be 16-byte aligned");
    gat_backward_src(stream, n_rows, n_cols, t_indptr, t_indices, Z, ldz, nullptr, s_src, nullptr, nullptr, rec, G, ldg, att,
                     ds_dst, K, dh, slope, ds_src, G_Z, ldgz, nullptr);
}

MGGCN_API void mggcn_gat_backward_src_rec_drop_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols,
                                                   const uint32_t *t_indptr, const uint32_t *t_indices, const float *Z,
                                                   size_t ldz, const float *rec, const float *s_src, const float *G, size_t ldg,
                                                   const float *att, const float *ds_dst, uint32_t K, uint32_t dh, float slope,
                                                   float *ds_src, float *G_Z, size_t ldgz, uint32_t threshold, float scale,
                                                   uint64_t seed, uint32_t dropout_stream, uint32_t dst0, uint32_t src0) {
    MGGCN_REQUIRE(!n_rows || !n_cols || (rec != nullptr && aligned16(rec)), "gat backward: rec must be 16-byte aligned");
    const gat_drop dp = make_gat_drop(threshold, scale, seed, dropout_stream, dst0, n_cols, src0, n_rows);
    gat_backward_src(stream, n_rows, n_cols, t_indptr, t_indices, Z, ldz, nullptr, s_src, nullptr, nullptr, rec, G, ldg, att,
                     ds_dst, K, dh, slope, ds_src, G_Z, ldgz, threshold ? &dp : nullptr);
}

// The export of the coefficients: the only GAT call that writes something of nnz x K, and nothing calls it but the user
MGGCN_API void mggcn_gat_alpha_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                   const uint32_t *indices, const float *s_dst, const float *s_src, const float *lse,
                                   uint32_t K, float slope, float *alpha, size_t lda) {
    MGGCN_REQUIRE(K >= 1 && K <= MGGCN_GAT_MAX_HEADS, "gat supports 1 <= heads <= 16");
    MGGCN_REQUIRE(lda >= K, "gat alpha: lda < heads");
    if (!n_rows) return;
    MGGCN_REQUIRE(indptr != nullptr && s_dst != nullptr && lse != nullptr, "gat alpha: null operand");
    MGGCN_REQUIRE(n_cols == 0 || (indices != nullptr && s_src != nullptr && alpha != nullptr), "gat alpha: null operand");
    MGGCN_REQUIRE(alpha != s_dst && alpha != s_src && alpha != lse, "gat alpha: alpha must not alias s_dst, s_src or lse");
    if (K % 4 == 0 && rows16(alpha, lda))
        launch_rows(gat_alpha_kernel<4>, n_rows, stream, n_rows, indptr, indices, s_dst, s_src, lse, K, slope, alpha, lda);
    else
        launch_rows(gat_alpha_kernel<1>, n_rows, stream, n_rows, indptr, indices, s_dst, s_src, lse, K, slope, alpha, lda);
}

MGGCN_API void mggcn_gat_scores_backward_f32(mggcn_stream_t stream, const float *ds_dst, const float *Z_dst, size_t ldzd,
                                             size_t n_dst, const float *ds_src, const float *Z_src, size_t ldzs, size_t n_src,
                                             uint32_t K, uint32_t dh, float *G_att) {
    require_heads(K, dh);
    const uint32_t width = K * dh;
    MGGCN_REQUIRE(ldzd >= width && ldzs >= width, "gat scores backward: leading dimension < heads * width per head");
    MGGCN_REQUIRE(G_att != nullptr, "gat scores backward: null gradient");
    MGGCN_REQUIRE(n_dst == 0 || (ds_dst != nullptr && Z_dst != nullptr), "gat scores backward: null operand");
    MGGCN_REQUIRE(n_src == 0 || (ds_src != nullptr && Z_src != nullptr), "gat scores backward: null operand");
    gat_column_sums<2>(stream, gat_scores_term{{ds_dst, ds_src}, {Z_dst, Z_src}, {ldzd, ldzs}, {n_dst, n_src}, K, dh},
                       std::max(n_dst, n_src), width, G_att);
}
