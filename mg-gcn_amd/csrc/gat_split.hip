// gat_split.hip -- the three sparse GAT kernels over a PLAN that cuts long rows (mggcn_gat_*_split_f32; gat(row_split=S)).
//
// gat.hip gives one wave a whole CSR row; on a graph with hubs the few waves that walk the longest rows set the time of the
// launch.  Here the unit of work is an ITEM of mggcn_plan::rowsplit_build (plan_host.cpp, the table the SpMM's plan and
// spmm_dev.hip use): a row of at most 1.5 x split entries is one item with slot = kNoSlot, a longer row ceil(len / split)
// contiguous slices with a partial slot each.  One wave per item, four items per workgroup, in the table's longest-first
// order, so the launch starts with the heavy items and ends with the short ones.
//   * an item walks all K heads over its [beg, end) with the walk, the groups and the (VEC, NT, U) variants of gat.hip
//     (gat_internal.h); the statements between the item's bounds and its epilogue are those of gat_kernels.h;
//   * an item without a slot ends as the plain kernel ends: an un-split row has the plain call's bits;
//   * a slice stores its state after fold_groups instead -- per (slot, head) two scalars and, for forward and backward_src,
//     one head-row of K dh-strided accumulators -- into buffers the plan owns;
//   * a second launch merges the slices of every split row in SLOT ORDER (the order of the entries): one wave per (split
//     row, head), lane l owning columns l, l + 64, ...; backward_dst has scalars only and takes one thread per (row, head).
// forward: a slice's state is (m_s, sum_s, acc_s) of the one-pass softmax over its entries; the merge rescales every slice to
// M = max_s m_s: sum = sum_s sum_s exp(m_s - M), out = (sum_s acc_s exp(m_s - M)) / sum, lse = M + log(sum).  A slice is never
// empty, so every m_s is finite, the slice that holds M enters with the factor 1 and sum >= 1: a factor may underflow to 0,
// nothing becomes inf - inf.
// backward_dst: every slice loads the row's own G head-row and forms D = G . out itself (the same bits in every slice), so
// its share of ds_dst is formed against the D the merge then writes out once.
// backward_src: a slice stores its share of ds_src and its unfinished sum alpha G; the merge adds both in slot order and only
// then applies the epilogue fmaf(ds_src, att[1], fmaf(ds_dst, att[0], acc)).
// Attention dropout is keyed by (destination, source, head), not by position: a slice draws the plain kernel's words.
// No atomics: a result depends on the matrix, split and the operands alone, not on the grid, the item order or the call.
#include <algorithm>
#include <chrono>
#include <cmath>

#include "common.h"
#include "gat_internal.h"
#include "gat_kernels.h"
#include "philox.h"
#include "plan_host.h"
#include "reduce.h"

using mggcn_plan::kNoSlot;
using mggcn_plan::SplitRow;
using mggcn_plan::SpmmItem;

struct mggcn_gat_split_plan {
    uint32_t n_rows = 0, split = 0, max_heads = 0, max_width = 0;
    uint32_t n_items = 0, n_split_rows = 0, n_slots = 0;
    uint64_t nnz = 0;
    SpmmItem *d_items = nullptr;
    SplitRow *d_split = nullptr;
    float *d_rows = nullptr;        // n_slots x max_width: a slice's head-rows, at the stride K dh of the call
    float *d_scalars = nullptr;     // n_slots x max_heads x 2: (m, sum) | (share of ds_dst, D) | (share of ds_src, -)
    size_t bytes = 0;
    double build_s = 0.0;
};

namespace {

// one wave per item, four items per workgroup: the geometry of MGGCN_GAT_WAVE_ROW with the row and its bounds from the table
#define MGGCN_GAT_WAVE_ITEM(n_items, items)                                                                   \
    const uint32_t lane = threadIdx.x & 63;                                                                   \
    const uint32_t lpr = 1u << lg, n_grp = 64u >> lg, sub = lane & (lpr - 1), grp = lane >> lg;               \
    const uint32_t item = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);                  \
    if (item >= (n_items)) return;                                                                            \
    const size_t row = (items)[item].row;                                                                     \
    const uint32_t beg = (items)[item].beg, end = (items)[item].end, slot = (items)[item].slot;               \
    const bool whole = slot == kNoSlot

// ---------------------------------------------------------------------------
// forward over the items
// ---------------------------------------------------------------------------
template <int VEC, int NT, int U, bool DROP>
__global__ __launch_bounds__(256) void gat_split_forward_kernel(uint32_t n_items, const SpmmItem *__restrict__ items,
                                                                const uint32_t *__restrict__ indices,
                                                                const float *__restrict__ Z, size_t ldz,
                                                                const float *__restrict__ s_dst, const float *__restrict__ s_src,
                                                                uint32_t K, uint32_t dh, float slope, uint32_t lg,
                                                                float *__restrict__ out, size_t ldo, float *__restrict__ lse,
                                                                float *__restrict__ p_rows, float *__restrict__ p_scalars,
                                                                gat_drop dp) {
    MGGCN_GAT_WAVE_ITEM(n_items, items);
    for (uint32_t k = 0; k < K; k++) {
        const float sd = s_dst[row * K + k];
        const float *__restrict__ Zk = Z + (size_t)k * dh;
        float m = -INFINITY, sum = 0.f;
        float acc[NT][VEC];
        zero_head_row<VEC, NT>(acc);
        const auto fetch = [&](uint32_t c, float *s) { s[0] = s_src[(size_t)c * K + k]; };
        entry_chunks<1> ch;
        ch.start(indices, beg, end, lane, fetch);
        for (uint32_t base = beg; base < end; base += 64) {
            ch.next(indices, base, end, lane, fetch);
            const uint32_t cnt = ch.cnt;
            const float x = sd + ch.my_s[0];
            const float e = lane < cnt ? gat_lrelu(x, slope) : -INFINITY;
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
        if (whole) {                                         // the plain kernel's end
            const float inv = beg < end ? 1.f / sum : 0.f;
            if (lane == 0) lse[row * K + k] = beg < end ? m + logf(sum) : 0.f;
            fold_store_head_row<VEC, NT>(out + row * ldo + (size_t)k * dh, acc, lpr, sub, grp, dh,
                                         [&](int, int, float x) { return x * inv; });      // an empty row: +0.0
        } else {                                             // (m_s, sum_s) and the un-normalised head-row
            if (lane == 0) {
                p_scalars[((size_t)slot * K + k) * 2] = m;
                p_scalars[((size_t)slot * K + k) * 2 + 1] = sum;
            }
            fold_store_head_row<VEC, NT>(p_rows + ((size_t)slot * K + k) * dh, acc, lpr, sub, grp, dh);
        }
    }
}

// one wave per (split row, head): the slices meet at M = max_s m_s, in slot order
constexpr int kMergeTiles = MGGCN_GAT_MAX_WIDTH / 64;       // columns per lane at the widest head
__global__ __launch_bounds__(256) void gat_split_forward_merge_kernel(uint32_t n_split, const SplitRow *__restrict__ split_rows,
                                                                      const float *__restrict__ p_rows,
                                                                      const float *__restrict__ p_scalars, uint32_t K,
                                                                      uint32_t dh, float *__restrict__ out, size_t ldo,
                                                                      float *__restrict__ lse) {
    const uint32_t lane = threadIdx.x & 63;
    const size_t w = (size_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (w >= (size_t)n_split * K) return;
    const uint32_t k = (uint32_t)(w % K);
    const SplitRow sr = split_rows[w / K];
    float M = -INFINITY;
    for (uint32_t s = 0; s < sr.n_slots; s++) M = fmaxf(M, p_scalars[((size_t)(sr.first_slot + s) * K + k) * 2]);
    float sum = 0.f, acc[kMergeTiles];
#pragma unroll
    for (int t = 0; t < kMergeTiles; t++) acc[t] = 0.f;
    for (uint32_t s = 0; s < sr.n_slots; s++) {
        const size_t sk = (size_t)(sr.first_slot + s) * K + k;
        const float f = expf(p_scalars[sk * 2] - M);         // <= 1; 0 where the slice lies far below the row's maximum
        sum = fmaf(p_scalars[sk * 2 + 1], f, sum);
#pragma unroll
        for (int t = 0; t < kMergeTiles; t++) {
            const uint32_t c = t * 64 + lane;
            if (c < dh) acc[t] = fmaf(p_rows[sk * dh + c], f, acc[t]);
        }
    }
    if (lane == 0) lse[(size_t)sr.row * K + k] = M + logf(sum);
#pragma unroll
    for (int t = 0; t < kMergeTiles; t++) {
        const uint32_t c = t * 64 + lane;
        if (c < dh) out[(size_t)sr.row * ldo + (size_t)k * dh + c] = acc[t] / sum;
    }
}

// ---------------------------------------------------------------------------
// backward over the items of F
// ---------------------------------------------------------------------------
template <int VEC, int NT, int U, bool DROP>
__global__ __launch_bounds__(256) void gat_split_backward_dst_kernel(uint32_t n_items, const SpmmItem *__restrict__ items,
                                                                     const uint32_t *__restrict__ indices,
                                                                     const float *__restrict__ Z, size_t ldz,
                                                                     const float *__restrict__ s_dst,
                                                                     const float *__restrict__ s_src,
                                                                     const float *__restrict__ lse, const float *__restrict__ G,
                                                                     size_t ldg, const float *__restrict__ out, size_t ldo,
                                                                     uint32_t K, uint32_t dh, float slope, uint32_t lg,
                                                                     float *__restrict__ D, float *__restrict__ ds_dst,
                                                                     float *__restrict__ p_scalars, gat_drop dp) {
    MGGCN_GAT_WAVE_ITEM(n_items, items);
    for (uint32_t k = 0; k < K; k++) {
        float g[NT][VEC];
        load_head_row<VEC, NT>(g, G + row * ldg + (size_t)k * dh, lpr, sub, dh);
        const float Dk = head_row_D<VEC, NT>(g, out + row * ldo + (size_t)k * dh, lpr, sub, grp, dh);
        const float sd = s_dst[row * K + k], ls = lse[row * K + k];
        const float *__restrict__ Zk = Z + (size_t)k * dh;
        float acc = 0.f;
        const auto fetch = [&](uint32_t c, float *s) { s[0] = s_src[(size_t)c * K + k]; };
        entry_chunks<1> ch;
        ch.start(indices, beg, end, lane, fetch);
        for (uint32_t base = beg; base < end; base += 64) {
            ch.next(indices, base, end, lane, fetch);
            const uint32_t cnt = ch.cnt;
            float my_w = 0.f;                       // alpha lrelu'(x) of my entry
            [[maybe_unused]] float my_q = 0.f;
            if (lane < cnt) {
                const float x = sd + ch.my_s[0];
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
            if (whole) {
                D[row * K + k] = Dk;
                ds_dst[row * K + k] = acc;
            } else {                                // my share, and the D it was formed against (every slice has these bits)
                p_scalars[((size_t)slot * K + k) * 2] = acc;
                p_scalars[((size_t)slot * K + k) * 2 + 1] = Dk;
            }
        }
    }
}

// one thread per (split row, head): the shares in slot order, D once
__global__ __launch_bounds__(256) void gat_split_backward_dst_merge_kernel(uint32_t n_split, const SplitRow *__restrict__ split_rows,
                                                                           const float *__restrict__ p_scalars, uint32_t K,
                                                                           float *__restrict__ D, float *__restrict__ ds_dst) {
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= (size_t)n_split * K) return;
    const uint32_t k = (uint32_t)(w % K);
    const SplitRow sr = split_rows[w / K];
    float acc = 0.f;
    for (uint32_t s = 0; s < sr.n_slots; s++) acc += p_scalars[((size_t)(sr.first_slot + s) * K + k) * 2];
    D[(size_t)sr.row * K + k] = p_scalars[((size_t)sr.first_slot * K + k) * 2 + 1];
    ds_dst[(size_t)sr.row * K + k] = acc;
}

// ---------------------------------------------------------------------------
// backward over the items of F^T
// ---------------------------------------------------------------------------
template <int VEC, int NT, int U, bool DROP>
__global__ __launch_bounds__(256) void gat_split_backward_src_kernel(uint32_t n_items, const SpmmItem *__restrict__ items,
                                                                     const uint32_t *__restrict__ indices,
                                                                     const float *__restrict__ Z, size_t ldz,
                                                                     const float *__restrict__ s_dst,
                                                                     const float *__restrict__ s_src,
                                                                     const float *__restrict__ lse, const float *__restrict__ D,
                                                                     const float *__restrict__ G, size_t ldg,
                                                                     const float *__restrict__ att,
                                                                     const float *__restrict__ ds_dst, uint32_t K, uint32_t dh,
                                                                     float slope, uint32_t lg, float *__restrict__ ds_src,
                                                                     float *__restrict__ G_Z, size_t ldgz,
                                                                     float *__restrict__ p_rows, float *__restrict__ p_scalars,
                                                                     gat_drop dp) {
    MGGCN_GAT_WAVE_ITEM(n_items, items);
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
            s[0] = s_dst[ik]; s[1] = lse[ik]; s[2] = D[ik];
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
                const float x = my_x + ss;          // s_dst[i] + s_src[j]: the forward's sum
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
        if (!whole) {                               // my share of ds_src and the unfinished sum alpha G
            if (lane == 0) p_scalars[((size_t)slot * K + k) * 2] = acc_ds;
            fold_store_head_row<VEC, NT>(p_rows + ((size_t)slot * K + k) * dh, acc, lpr, sub, grp, dh);
            continue;
        }
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

// one wave per (split row, head): shares and head-rows in slot order, then the plain kernel's epilogue
__global__ __launch_bounds__(256) void gat_split_backward_src_merge_kernel(uint32_t n_split, const SplitRow *__restrict__ split_rows,
                                                                           const float *__restrict__ p_rows,
                                                                           const float *__restrict__ p_scalars,
                                                                           const float *__restrict__ att,
                                                                           const float *__restrict__ ds_dst, uint32_t K,
                                                                           uint32_t dh, float *__restrict__ ds_src,
                                                                           float *__restrict__ G_Z, size_t ldgz) {
    const uint32_t lane = threadIdx.x & 63;
    const size_t w = (size_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (w >= (size_t)n_split * K) return;
    const uint32_t k = (uint32_t)(w % K), width = K * dh;
    const SplitRow sr = split_rows[w / K];
    float acc_ds = 0.f, acc[kMergeTiles];
#pragma unroll
    for (int t = 0; t < kMergeTiles; t++) acc[t] = 0.f;
    for (uint32_t s = 0; s < sr.n_slots; s++) {
        const size_t sk = (size_t)(sr.first_slot + s) * K + k;
        acc_ds += p_scalars[sk * 2];
#pragma unroll
        for (int t = 0; t < kMergeTiles; t++) {
            const uint32_t c = t * 64 + lane;
            if (c < dh) acc[t] += p_rows[sk * dh + c];
        }
    }
    if (lane == 0) ds_src[(size_t)sr.row * K + k] = acc_ds;
    const float dd = ds_dst ? ds_dst[(size_t)sr.row * K + k] : 0.f;
#pragma unroll
    for (int t = 0; t < kMergeTiles; t++) {
        const uint32_t c = t * 64 + lane;
        if (c < dh)
            G_Z[(size_t)sr.row * ldgz + (size_t)k * dh + c] =
                fmaf(acc_ds, att[width + (size_t)k * dh + c], fmaf(dd, att[(size_t)k * dh + c], acc[t]));
    }
}

// what every entry point checks of its plan, and the drop descriptor as the kernels take it
void require_plan(const mggcn_gat_split_plan *plan, uint32_t n_rows, uint32_t K, uint32_t dh) {
    MGGCN_REQUIRE(plan != nullptr, "gat split: null plan");
    MGGCN_REQUIRE(plan->n_rows == n_rows, "gat split: the plan was built for another number of rows");
    MGGCN_REQUIRE(K <= plan->max_heads && (size_t)K * dh <= plan->max_width,
                  "gat split: heads or width above what the plan was created for");
}
gat_drop drop_of(const mggcn_gat_drop *drop, uint32_t n_dst, uint32_t n_src) {
    if (!drop || !drop->threshold) return gat_drop{};
    return make_gat_drop(drop->threshold, drop->scale, drop->seed, drop->dropout_stream, drop->dst0, n_dst, drop->src0, n_src);
}

template <class... P, class... A>
void launch_waves(void (*kernel)(P...), size_t n_waves, mggcn_stream_t stream, A... args) {
    if (!n_waves) return;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n_waves + 3) / 4)), dim3(256), 0, as_stream(stream), args...);
    MGGCN_CHECK_LAUNCH();
}

}  // namespace

// ============================ C ABI =========================================
MGGCN_API mggcn_gat_split_plan *mggcn_gat_split_plan_create(uint32_t n_rows, const uint32_t *host_indptr, uint32_t split,
                                                            uint32_t max_heads, uint32_t max_width) {
    MGGCN_REQUIRE(host_indptr != nullptr, "gat split plan needs the host copy of indptr");
    MGGCN_REQUIRE(split >= 64 && split % 64 == 0, "gat split plan: split must be a multiple of 64, at least 64");
    MGGCN_REQUIRE(max_heads >= 1 && max_heads <= MGGCN_GAT_MAX_HEADS && max_width >= max_heads && max_width <= MGGCN_GAT_MAX_WIDTH,
                  "gat split plan: 1 <= max_heads <= 16 and max_heads <= max_width <= 1024");
    const auto t0 = std::chrono::steady_clock::now();
    const mggcn_plan::RowSplitHost rs = mggcn_plan::rowsplit_build(n_rows, host_indptr, split);
    auto *plan = new mggcn_gat_split_plan;
    plan->n_rows = n_rows; plan->split = split; plan->max_heads = max_heads; plan->max_width = max_width;
    plan->n_items = (uint32_t)rs.items.size();
    plan->n_split_rows = (uint32_t)rs.split_rows.size();
    plan->n_slots = rs.n_slots;
    plan->nnz = (uint64_t)host_indptr[n_rows] - host_indptr[0];
    const size_t ib = rs.items.size() * sizeof(SpmmItem), sb = rs.split_rows.size() * sizeof(SplitRow);
    const size_t rb = (size_t)rs.n_slots * max_width * sizeof(float), cb = (size_t)rs.n_slots * max_heads * 2 * sizeof(float);
    if (ib) {
        MGGCN_CHECK_HIP(hipMalloc(&plan->d_items, ib));
        MGGCN_CHECK_HIP(hipMemcpy(plan->d_items, rs.items.data(), ib, hipMemcpyHostToDevice));
    }
    if (sb) {
        MGGCN_CHECK_HIP(hipMalloc(&plan->d_split, sb));
        MGGCN_CHECK_HIP(hipMemcpy(plan->d_split, rs.split_rows.data(), sb, hipMemcpyHostToDevice));
    }
    if (rb) MGGCN_CHECK_HIP(hipMalloc(&plan->d_rows, rb));
    if (cb) MGGCN_CHECK_HIP(hipMalloc(&plan->d_scalars, cb));
    plan->bytes = ib + sb + rb + cb;
    plan->build_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return plan;
}

MGGCN_API void mggcn_gat_split_plan_destroy(mggcn_gat_split_plan *plan) {
    if (!plan) return;
    if (plan->d_items) MGGCN_CHECK_HIP(hipFree(plan->d_items));
    if (plan->d_split) MGGCN_CHECK_HIP(hipFree(plan->d_split));
    if (plan->d_rows) MGGCN_CHECK_HIP(hipFree(plan->d_rows));
    if (plan->d_scalars) MGGCN_CHECK_HIP(hipFree(plan->d_scalars));
    delete plan;
}

MGGCN_API uint32_t mggcn_gat_split_plan_num_items(const mggcn_gat_split_plan *plan) { return plan->n_items; }
MGGCN_API uint32_t mggcn_gat_split_plan_num_split_rows(const mggcn_gat_split_plan *plan) { return plan->n_split_rows; }
MGGCN_API uint32_t mggcn_gat_split_plan_num_slots(const mggcn_gat_split_plan *plan) { return plan->n_slots; }
MGGCN_API size_t mggcn_gat_split_plan_bytes(const mggcn_gat_split_plan *plan) { return plan->bytes; }

// The checks of each call are the plain entry point's (gat_kernels.h), then the plan's.
MGGCN_API void mggcn_gat_forward_split_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                           const uint32_t *indices, const float *Z, size_t ldz, const float *s_dst,
                                           const float *s_src, uint32_t K, uint32_t dh, float slope, float *out, size_t ldo,
                                           float *lse, const mggcn_gat_split_plan *plan, const mggcn_gat_drop *drop) {
    require_heads(K, dh);
    MGGCN_REQUIRE(ldz >= (size_t)K * dh && ldo >= (size_t)K * dh, "gat forward: leading dimension < heads * width per head");
    require_plan(plan, n_rows, K, dh);
    const gat_drop d = drop_of(drop, n_rows, n_cols);
    if (!n_rows) return;
    MGGCN_REQUIRE(indptr != nullptr && s_dst != nullptr && out != nullptr && lse != nullptr, "gat forward: null operand");
    MGGCN_REQUIRE(n_cols == 0 || (indices != nullptr && Z != nullptr && s_src != nullptr), "gat forward: null operand");
    MGGCN_REQUIRE(out != Z, "gat forward: out must not alias Z");
    MGGCN_REQUIRE(n_cols != 0 || plan->nnz == 0, "gat split: the plan has entries, the call has no columns");
    const bool vec = dh % 4 == 0 && rows16(Z, ldz) && rows16(out, ldo);
    const head_geometry hg = head_geometry_for(dh, vec);
    gat_dispatch(vec, hg.nt, [&](auto v) {
        with_flag(drop != nullptr && drop->threshold != 0, [&](auto dropped) {
            launch_waves(gat_split_forward_kernel<v.VEC, v.NT, v.U, dropped>, plan->n_items, stream, plan->n_items, plan->d_items,
                         indices, Z, ldz, s_dst, s_src, K, dh, slope, hg.lg, out, ldo, lse, plan->d_rows, plan->d_scalars, d);
        });
    });
    launch_waves(gat_split_forward_merge_kernel, (size_t)plan->n_split_rows * K, stream, plan->n_split_rows, plan->d_split,
                 plan->d_rows, plan->d_scalars, K, dh, out, ldo, lse);
}

MGGCN_API void mggcn_gat_backward_dst_split_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                                const uint32_t *indices, const float *Z, size_t ldz, const float *s_dst,
                                                const float *s_src, const float *lse, const float *G, size_t ldg,
                                                const float *out, size_t ldo, uint32_t K, uint32_t dh, float slope, float *D,
                                                float *ds_dst, const mggcn_gat_split_plan *plan, const mggcn_gat_drop *drop) {
    require_heads(K, dh);
    const size_t width = (size_t)K * dh;
    MGGCN_REQUIRE(ldz >= width && ldg >= width && ldo >= width, "gat backward: leading dimension < heads * width per head");
    require_plan(plan, n_rows, K, dh);
    const gat_drop d = drop_of(drop, n_rows, n_cols);
    if (!n_rows) return;
    MGGCN_REQUIRE(indptr != nullptr && s_dst != nullptr && lse != nullptr && G != nullptr && out != nullptr && D != nullptr &&
                      ds_dst != nullptr,
                  "gat backward: null operand");
    MGGCN_REQUIRE(n_cols == 0 || (indices != nullptr && Z != nullptr && s_src != nullptr), "gat backward: null operand");
    MGGCN_REQUIRE(n_cols != 0 || plan->nnz == 0, "gat split: the plan has entries, the call has no columns");
    const bool vec = dh % 4 == 0 && rows16(Z, ldz) && rows16(G, ldg) && rows16(out, ldo);
    const head_geometry hg = head_geometry_for(dh, vec);
    gat_dispatch(vec, hg.nt, [&](auto v) {
        with_flag(drop != nullptr && drop->threshold != 0, [&](auto dropped) {
            launch_waves(gat_split_backward_dst_kernel<v.VEC, v.NT, v.U, dropped>, plan->n_items, stream, plan->n_items,
                         plan->d_items, indices, Z, ldz, s_dst, s_src, lse, G, ldg, out, ldo, K, dh, slope, hg.lg, D, ds_dst,
                         plan->d_scalars, d);
        });
    });
    const size_t n = (size_t)plan->n_split_rows * K;
    if (n) {
        hipLaunchKernelGGL(gat_split_backward_dst_merge_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream),
                           plan->n_split_rows, plan->d_split, plan->d_scalars, K, D, ds_dst);
        MGGCN_CHECK_LAUNCH();
    }
}

// rows of F^T are sources (offset src0), its entries destinations (offset dst0)
MGGCN_API void mggcn_gat_backward_src_split_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *t_indptr,
                                                const uint32_t *t_indices, const float *Z, size_t ldz, const float *s_dst,
                                                const float *s_src, const float *lse, const float *D, const float *G, size_t ldg,
                                                const float *att, const float *ds_dst, uint32_t K, uint32_t dh, float slope,
                                                float *ds_src, float *G_Z, size_t ldgz, const mggcn_gat_split_plan *plan,
                                                const mggcn_gat_drop *drop) {
    require_heads(K, dh);
    const size_t width = (size_t)K * dh;
    MGGCN_REQUIRE(ldz >= width && ldg >= width && ldgz >= width, "gat backward: leading dimension < heads * width per head");
    require_plan(plan, n_rows, K, dh);
    const gat_drop d = drop_of(drop, n_cols, n_rows);
    if (!n_rows) return;
    MGGCN_REQUIRE(t_indptr != nullptr && Z != nullptr && s_src != nullptr && att != nullptr && ds_src != nullptr &&
                      G_Z != nullptr,
                  "gat backward: null operand");
    MGGCN_REQUIRE(n_cols == 0 || (t_indices != nullptr && G != nullptr && s_dst != nullptr && lse != nullptr && D != nullptr),
                  "gat backward: null operand");
    MGGCN_REQUIRE(G_Z != G && G_Z != Z, "gat backward: G_Z must not alias G or Z");
    MGGCN_REQUIRE(n_cols != 0 || plan->nnz == 0, "gat split: the plan has entries, the call has no columns");
    const bool vec = dh % 4 == 0 && rows16(Z, ldz) && rows16(G, ldg) && rows16(G_Z, ldgz) && aligned16(att);
    const head_geometry hg = head_geometry_for(dh, vec);
    gat_dispatch(vec, hg.nt, [&](auto v) {
        with_flag(drop != nullptr && drop->threshold != 0, [&](auto dropped) {
            launch_waves(gat_split_backward_src_kernel<v.VEC, v.NT, v.U, dropped>, plan->n_items, stream, plan->n_items,
                         plan->d_items, t_indices, Z, ldz, s_dst, s_src, lse, D, G, ldg, att, ds_dst, K, dh, slope, hg.lg, ds_src,
                         G_Z, ldgz, plan->d_rows, plan->d_scalars, d);
        });
    });
    launch_waves(gat_split_backward_src_merge_kernel, (size_t)plan->n_split_rows * K, stream, plan->n_split_rows, plan->d_split,
                 plan->d_rows, plan->d_scalars, att, ds_dst, K, dh, ds_src, G_Z, ldgz);
}
