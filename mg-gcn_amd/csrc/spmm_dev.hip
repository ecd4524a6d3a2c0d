// spmm_dev.hip -- the row-split CSR SpMM over a DEVICE-RESIDENT matrix whose plan is built on the device (gfx950).
//
// The per-epoch edge sample of gcn / sage(aggr="mean") (edge_sample.hip) is a fresh CSR every training forward that the host
// never sees: the sweep plan (a second of host work over host arrays) is out of reach, the row-split form of spmm.hip is not --
// it consumes a table of SpmmItem {row, beg, end, slot}, a table of SplitRow and a partial-sum buffer, and only its BUILDER
// (plan_host.cpp: rowsplit_build) is host code.  This file is that builder as three kernels, and the row-split kernels and the
// combine kernel again, reading their item / split-row counts from device memory.
//
//   capacity   rowsplit_build's rule is monotone in the row length (len <= split + split/2: one item; else ceil(len / split)
//              slices), and a sample's row is never longer than its parent's: the parent's item, slot and split-row counts,
//              summed on the host at plan_create, bound every sample of it.  Nothing else is known on the host.
//   build      (1) per row: is it split, and into how many slices; (2) two exclusive scans (mggcn_edge_sample_scan_u32: no
//              workgroup waits on another): S over the split flags, T over the slice counts; (3) per row, the tables in ROW
//              ORDER: a whole row r is item r - S[r] + T[r], a split row its slices from there on with slots T[r].., split-row
//              record S[r]; the slice boundaries are rowsplit_build's (b + len k / parts in 64-bit).  The three totals stay in
//              device memory.  There is no sort: the host builder's longest-first (LPT) order is not reproduced -- every item
//              is computed alone and the slices of a row are summed in slot order, so the ORDER of the table changes no bit.
//   multiply   launch geometry from the capacities, true counts from device memory, surplus waves leave at once.
//
// The bodies below restate spmm.hip's vec4_body / scalar_body / spmm_combine_kernel for HAS_ITEMS = true, operation for
// operation (tests/test_gpu_edge_sample_val.py holds the two forms to the same bits on the same matrix and split).  They live
// here, not behind a shared header, because the sources of the existing SpMM kernels are pinned: profiles/spmm_hbm_traffic.json
// carries their content hash.  No atomics, no LDS, the same bits on every call.
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "plan_host.h"

using mggcn_plan::env_u32;
using mggcn_plan::kNoSlot;
using mggcn_plan::SplitRow;
using mggcn_plan::SpmmItem;

namespace {

__device__ __forceinline__ float lrelu(float x, float slope) {
    const float y = slope * x;
    return x > y ? x : y;
}

__device__ __forceinline__ float4 load4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ float4 load4(const uint16_t *p) {
    const uint2 w = *reinterpret_cast<const uint2 *>(p);
    return make_float4(__builtin_bit_cast(float, w.x << 16), __builtin_bit_cast(float, w.x & 0xFFFF0000u),
                       __builtin_bit_cast(float, w.y << 16), __builtin_bit_cast(float, w.y & 0xFFFF0000u));
}
__device__ __forceinline__ float load1(const float *p) { return *p; }
__device__ __forceinline__ float load1(const uint16_t *p) { return __builtin_bit_cast(float, (uint32_t)*p << 16); }

__device__ __forceinline__ float4 fma4(float s, float4 b, float4 a) {
    a.x = fmaf(s, b.x, a.x);
    a.y = fmaf(s, b.y, a.y);
    a.z = fmaf(s, b.z, a.z);
    a.w = fmaf(s, b.w, a.w);
    return a;
}

enum { kTotalItems = 0, kTotalSlots = 1, kTotalSplit = 2 };

#define MGGCN_DEV_PARAMS(TB)                                                                                                  \
    const SpmmItem *__restrict__ items, const uint32_t *__restrict__ totals, uint32_t cap_items,                              \
        const uint32_t *__restrict__ indices, const float *__restrict__ values, const TB *__restrict__ B, size_t ldb,         \
        float *__restrict__ C, size_t ldc, float *__restrict__ partial, uint32_t d, float alpha, float beta, uint32_t flags,  \
        float slope

// spmm.hip: vec4_body<LPR, UNROLL, true, TB> with the item count read from the device
template <int LPR, int UNROLL, typename TB>
__global__ __launch_bounds__(256) void spmm_dev_vec4_kernel(MGGCN_DEV_PARAMS(TB)) {
    constexpr int G = 64 / LPR;
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane((uint32_t)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (wave >= min(totals[kTotalItems], cap_items)) return;
    const SpmmItem it = items[wave];
    const uint32_t row = it.row, beg = it.beg, end = it.end, slot = it.slot;
    const int sub = lane % LPR;
    const int grp = lane / LPR;

    for (uint32_t col0 = 0; col0 < d; col0 += LPR * 4) {
        const uint32_t col = col0 + sub * 4;
        const bool active = col < d;
        const TB *__restrict__ Bc = B + col;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        uint32_t nxt_c = 0;
        float nxt_v = 0.f;
        if (beg + lane < end) { nxt_c = indices[beg + lane]; nxt_v = values[beg + lane]; }
        for (uint32_t base = beg; base < end; base += 64) {
            const uint32_t my_c = nxt_c;
            const float my_v = nxt_v;
            const uint32_t e_next = base + 64 + lane;
            nxt_c = 0; nxt_v = 0.f;
            if (e_next < end) { nxt_c = indices[e_next]; nxt_v = values[e_next]; }
            const uint32_t cnt = min(64u, end - base);
            for (uint32_t j = 0; j < cnt; j += G * UNROLL) {
                float4 b[UNROLL];
                float v[UNROLL];
#pragma unroll
                for (int u = 0; u < UNROLL; u++) {
                    const uint32_t src = j + u * G + grp;
                    const uint32_t c = __shfl(my_c, src & 63);
                    const float vv = __shfl(my_v, src & 63);
                    const bool ok = active && src < cnt;
                    v[u] = ok ? vv : 0.f;
                    b[u] = ok ? load4(Bc + (size_t)c * ldb) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int u = 0; u < UNROLL; u++) acc = fma4(v[u], b[u], acc);
            }
        }
#pragma unroll
        for (int off = LPR; off < 64; off <<= 1) {
            acc.x += __shfl_xor(acc.x, off);
            acc.y += __shfl_xor(acc.y, off);
            acc.z += __shfl_xor(acc.z, off);
            acc.w += __shfl_xor(acc.w, off);
        }
        if (grp == 0 && active) {
            if (slot == kNoSlot) {
                float4 o = make_float4(alpha * acc.x, alpha * acc.y, alpha * acc.z, alpha * acc.w);
                float4 *cp = reinterpret_cast<float4 *>(C + (size_t)row * ldc + col);
                if (beta != 0.f) {
                    const float4 c0 = *cp;
                    o.x = fmaf(beta, c0.x, o.x); o.y = fmaf(beta, c0.y, o.y);
                    o.z = fmaf(beta, c0.z, o.z); o.w = fmaf(beta, c0.w, o.w);
                }
                if (flags & MGGCN_SPMM_LEAKY_RELU) {
                    o.x = lrelu(o.x, slope); o.y = lrelu(o.y, slope);
                    o.z = lrelu(o.z, slope); o.w = lrelu(o.w, slope);
                }
                *cp = o;
            } else {
                *reinterpret_cast<float4 *>(partial + (size_t)slot * d + col) = acc;
            }
        }
    }
}

// spmm.hip: scalar_body<UNROLL, true, TB> with the item count read from the device
template <int UNROLL, typename TB>
__global__ __launch_bounds__(256) void spmm_dev_scalar_kernel(MGGCN_DEV_PARAMS(TB)) {
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane((uint32_t)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (wave >= min(totals[kTotalItems], cap_items)) return;
    const SpmmItem it = items[wave];
    const uint32_t row = it.row, beg = it.beg, end = it.end, slot = it.slot;
    for (uint32_t col0 = 0; col0 < d; col0 += 64) {
        const uint32_t col = col0 + lane;
        const bool active = col < d;
        const TB *__restrict__ Bc = B + (active ? col : 0);
        float acc = 0.f;
        uint32_t nxt_c = 0;
        float nxt_v = 0.f;
        if (beg + lane < end) { nxt_c = indices[beg + lane]; nxt_v = values[beg + lane]; }
        for (uint32_t base = beg; base < end; base += 64) {
            const uint32_t my_c = nxt_c;
            const float my_v = nxt_v;
            const uint32_t e_next = base + 64 + lane;
            nxt_c = 0; nxt_v = 0.f;
            if (e_next < end) { nxt_c = indices[e_next]; nxt_v = values[e_next]; }
            const uint32_t cnt = min(64u, end - base);
            for (uint32_t j = 0; j < cnt; j += UNROLL) {
                float b[UNROLL], v[UNROLL];
#pragma unroll
                for (int u = 0; u < UNROLL; u++) {
                    const uint32_t src = (j + u) & 63;     // wave-uniform
                    const uint32_t c = __builtin_amdgcn_readlane(my_c, src);
                    const float vv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(uint32_t, my_v), src));
                    const bool ok = (j + u) < cnt;
                    v[u] = ok ? vv : 0.f;
                    b[u] = (ok && active) ? load1(Bc + (size_t)c * ldb) : 0.f;
                }
#pragma unroll
                for (int u = 0; u < UNROLL; u++) acc = fmaf(v[u], b[u], acc);
            }
        }
        if (active) {
            if (slot == kNoSlot) {
                float o = alpha * acc;
                float *cp = C + (size_t)row * ldc + col;
                if (beta != 0.f) o = fmaf(beta, *cp, o);
                if (flags & MGGCN_SPMM_LEAKY_RELU) o = lrelu(o, slope);
                *cp = o;
            } else {
                partial[(size_t)slot * d + col] = acc;
            }
        }
    }
}

// spmm.hip: spmm_combine_kernel with the split-row count read from the device
__global__ __launch_bounds__(256) void spmm_dev_combine_kernel(const SplitRow *__restrict__ rows, const uint32_t *__restrict__ totals,
                                                               uint32_t cap_split, const float *__restrict__ partial,
                                                               float *__restrict__ C, size_t ldc, uint32_t d, float alpha, float beta,
                                                               uint32_t flags, float slope) {
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane((uint32_t)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (wave >= min(totals[kTotalSplit], cap_split)) return;
    const SplitRow sr = rows[wave];
    for (uint32_t col = lane; col < d; col += 64) {
        float acc = 0.f;
        for (uint32_t s = 0; s < sr.n_slots; s++) acc += partial[(size_t)(sr.first_slot + s) * d + col];
        float o = alpha * acc;
        float *cp = C + (size_t)sr.row * ldc + col;
        if (beta != 0.f) o = fmaf(beta, *cp, o);
        if (flags & MGGCN_SPMM_LEAKY_RELU) o = lrelu(o, slope);
        *cp = o;
    }
}

// ---- the builder -------------------------------------------------------------------------------------------------------------
__device__ __host__ __forceinline__ bool row_is_split(uint32_t len, uint32_t split) { return len > split + split / 2; }
__device__ __host__ __forceinline__ uint32_t row_parts(uint32_t len, uint32_t split) { return (len + split - 1) / split; }

// (1) per row: 1 / 0 for "split", and its slice count (0 for a whole row)
__global__ __launch_bounds__(256) void spmm_dev_plan_count_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr, uint32_t split,
                                                                  uint32_t *__restrict__ is_split, uint32_t *__restrict__ n_parts) {
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const uint32_t len = indptr[r + 1] - indptr[r];
    const bool s = row_is_split(len, split);
    is_split[r] = s ? 1u : 0u;
    n_parts[r] = s ? row_parts(len, split) : 0u;
}

// (3) the tables in row order, from the two scans S (split rows in front of r) and T (slices in front of r); thread 0 of the
// grid leaves the totals.  A store at or beyond a table's capacity is never issued.
__global__ __launch_bounds__(256) void spmm_dev_plan_fill_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr, uint32_t split,
                                                                 const uint32_t *__restrict__ S, const uint32_t *__restrict__ T,
                                                                 SpmmItem *__restrict__ items, uint32_t cap_items,
                                                                 SplitRow *__restrict__ split_rows, uint32_t cap_split,
                                                                 uint32_t cap_slots, uint32_t *__restrict__ totals) {
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r == 0) {
        totals[kTotalItems] = n_rows - S[n_rows] + T[n_rows];
        totals[kTotalSlots] = T[n_rows];
        totals[kTotalSplit] = S[n_rows];
    }
    if (r >= n_rows) return;
    const uint32_t b = indptr[r], e = indptr[r + 1], len = e - b;
    const uint32_t at = (uint32_t)r - S[r] + T[r];
    if (!row_is_split(len, split)) {
        if (at < cap_items) items[at] = {(uint32_t)r, b, e, kNoSlot};
        return;
    }
    const uint32_t parts = row_parts(len, split), slot0 = T[r];
    if (S[r] < cap_split && slot0 + parts <= cap_slots) split_rows[S[r]] = {(uint32_t)r, slot0, parts, 0};
    for (uint32_t k = 0; k < parts; k++) {
        const uint32_t kb = b + (uint32_t)((uint64_t)len * k / parts);
        const uint32_t ke = b + (uint32_t)((uint64_t)len * (k + 1) / parts);
        if (at + k < cap_items && slot0 + k < cap_slots) items[at + k] = {(uint32_t)r, kb, ke, slot0 + k};
    }
}

}  // namespace

struct mggcn_spmm_dev_plan {
    uint32_t n_rows = 0, max_d = 0, split = 0;
    uint32_t cap_items = 0, cap_slots = 0, cap_split = 0;
    SpmmItem *d_items = nullptr;
    SplitRow *d_split = nullptr;
    float *d_partial = nullptr;
    uint32_t *d_work = nullptr;        // is_split[n], n_parts[n], S[n + 1], T[n + 1], totals[3]
    size_t bytes = 0;
    bool built = false;
    uint32_t *is_split() const { return d_work; }
    uint32_t *n_parts() const { return d_work + n_rows; }
    uint32_t *S() const { return d_work + 2 * (size_t)n_rows; }
    uint32_t *T() const { return d_work + 3 * (size_t)n_rows + 1; }
    uint32_t *totals() const { return d_work + 4 * (size_t)n_rows + 2; }
};

MGGCN_API void mggcn_spmm_dev_plan_capacity(uint32_t n_rows, const uint32_t *host_parent_indptr, uint32_t split, uint32_t *out3) {
    MGGCN_REQUIRE(out3 != nullptr && (host_parent_indptr != nullptr || n_rows == 0), "dev plan capacity: null operand");
    if (split == 0) split = env_u32("MGGCN_SPMM_SPLIT", 512u);
    split = std::max<uint32_t>(64u, split);
    uint64_t items = 0, slots = 0, rows = 0;
    for (uint32_t r = 0; r < n_rows; r++) {
        MGGCN_REQUIRE(host_parent_indptr[r + 1] >= host_parent_indptr[r], "indptr must be non-decreasing");
        const uint32_t len = host_parent_indptr[r + 1] - host_parent_indptr[r];
        if (row_is_split(len, split)) {
            const uint32_t parts = row_parts(len, split);
            items += parts; slots += parts; rows++;
        } else {
            items++;
        }
    }
    MGGCN_REQUIRE(items < (1ull << 32), "dev plan: more than 2^32 - 1 work items");
    out3[0] = (uint32_t)items; out3[1] = (uint32_t)slots; out3[2] = (uint32_t)rows;
}

MGGCN_API mggcn_spmm_dev_plan *mggcn_spmm_dev_plan_create(uint32_t n_rows, const uint32_t *host_parent_indptr, uint32_t max_d,
                                                          uint32_t split) {
    MGGCN_REQUIRE(max_d > 0, "max_d must be positive");
    if (split == 0) split = env_u32("MGGCN_SPMM_SPLIT", 512u);
    split = std::max<uint32_t>(64u, split);
    uint32_t cap[3];
    mggcn_spmm_dev_plan_capacity(n_rows, host_parent_indptr, split, cap);
    auto *plan = new mggcn_spmm_dev_plan;
    plan->n_rows = n_rows; plan->max_d = max_d; plan->split = split;
    plan->cap_items = cap[0]; plan->cap_slots = cap[1]; plan->cap_split = cap[2];
    const size_t ib = (size_t)cap[0] * sizeof(SpmmItem), sb = (size_t)cap[2] * sizeof(SplitRow);
    const size_t pb = (size_t)cap[1] * max_d * sizeof(float), wb = (4 * (size_t)n_rows + 5) * sizeof(uint32_t);
    // the tables start as 0xFF bytes: what a build does not reach stays recognisable (mggcn_spmm_dev_plan_read)
    if (ib) { MGGCN_CHECK_HIP(hipMalloc(&plan->d_items, ib)); MGGCN_CHECK_HIP(hipMemset(plan->d_items, 0xFF, ib)); }
    if (sb) { MGGCN_CHECK_HIP(hipMalloc(&plan->d_split, sb)); MGGCN_CHECK_HIP(hipMemset(plan->d_split, 0xFF, sb)); }
    if (pb) MGGCN_CHECK_HIP(hipMalloc(&plan->d_partial, pb));
    MGGCN_CHECK_HIP(hipMalloc(&plan->d_work, wb));
    MGGCN_CHECK_HIP(hipMemset(plan->d_work, 0, wb));
    MGGCN_CHECK_HIP(hipDeviceSynchronize());               // the fills are done before any stream builds into the tables
    plan->bytes = ib + sb + pb + wb;
    return plan;
}

MGGCN_API void mggcn_spmm_dev_plan_destroy(mggcn_spmm_dev_plan *plan) {
    if (!plan) return;
    if (plan->d_items) MGGCN_CHECK_HIP(hipFree(plan->d_items));
    if (plan->d_split) MGGCN_CHECK_HIP(hipFree(plan->d_split));
    if (plan->d_partial) MGGCN_CHECK_HIP(hipFree(plan->d_partial));
    if (plan->d_work) MGGCN_CHECK_HIP(hipFree(plan->d_work));
    delete plan;
}

MGGCN_API size_t mggcn_spmm_dev_plan_bytes(const mggcn_spmm_dev_plan *plan) { return plan ? plan->bytes : 0; }

MGGCN_API void mggcn_spmm_dev_plan_describe(const mggcn_spmm_dev_plan *plan, uint32_t *out5) {
    MGGCN_REQUIRE(plan != nullptr && out5 != nullptr, "dev plan describe: null operand");
    out5[0] = plan->cap_items; out5[1] = plan->cap_slots; out5[2] = plan->cap_split; out5[3] = plan->split; out5[4] = plan->max_d;
}

MGGCN_API void mggcn_spmm_dev_plan_build(mggcn_stream_t stream, mggcn_spmm_dev_plan *plan, const uint32_t *indptr_dev) {
    MGGCN_REQUIRE(plan != nullptr, "dev plan build: null plan");
    MGGCN_REQUIRE(indptr_dev != nullptr, "dev plan build: null operand");
    const hipStream_t st = as_stream(stream);
    const uint32_t n = plan->n_rows;
    const unsigned grid = (unsigned)std::max<size_t>(1, ((size_t)n + 255) / 256);
    if (n) {
        hipLaunchKernelGGL(spmm_dev_plan_count_kernel, dim3(grid), dim3(256), 0, st, n, indptr_dev, plan->split, plan->is_split(),
                           plan->n_parts());
        MGGCN_CHECK_LAUNCH();
    }
    mggcn_edge_sample_scan_u32(stream, plan->is_split(), n, plan->S());
    mggcn_edge_sample_scan_u32(stream, plan->n_parts(), n, plan->T());
    hipLaunchKernelGGL(spmm_dev_plan_fill_kernel, dim3(grid), dim3(256), 0, st, n, indptr_dev, plan->split, plan->S(), plan->T(),
                       plan->d_items, plan->cap_items, plan->d_split, plan->cap_split, plan->cap_slots, plan->totals());
    MGGCN_CHECK_LAUNCH();
    plan->built = true;
}

// tests and reports: the whole tables (capacity entries each; NULL skips one) and the three totals, after a synchronisation
MGGCN_API void mggcn_spmm_dev_plan_read(const mggcn_spmm_dev_plan *plan, uint32_t *host_items, uint32_t *host_split_rows,
                                        uint32_t *host_totals) {
    MGGCN_REQUIRE(plan != nullptr, "dev plan read: null plan");
    MGGCN_CHECK_HIP(hipDeviceSynchronize());
    if (host_items && plan->cap_items)
        MGGCN_CHECK_HIP(hipMemcpy(host_items, plan->d_items, (size_t)plan->cap_items * sizeof(SpmmItem), hipMemcpyDeviceToHost));
    if (host_split_rows && plan->cap_split)
        MGGCN_CHECK_HIP(hipMemcpy(host_split_rows, plan->d_split, (size_t)plan->cap_split * sizeof(SplitRow), hipMemcpyDeviceToHost));
    if (host_totals) MGGCN_CHECK_HIP(hipMemcpy(host_totals, plan->totals(), 3 * sizeof(uint32_t), hipMemcpyDeviceToHost));
}

namespace {

template <typename TB>
void spmm_csr_dev(mggcn_stream_t stream, const mggcn_spmm_dev_plan *plan, uint32_t n_rows, uint32_t n_cols, const uint32_t *indices,
                  const float *values, const TB *B, size_t ldb, float *C, size_t ldc, uint32_t d, float alpha, float beta,
                  uint32_t flags, float slope) {
    if (n_rows == 0 || d == 0) return;
    MGGCN_REQUIRE(plan != nullptr && plan->built, "spmm dev: the plan has not been built");
    MGGCN_REQUIRE(plan->n_rows == n_rows, "plan built for another matrix");
    MGGCN_REQUIRE(B && C, "null operand");
    MGGCN_REQUIRE(ldb >= d && ldc >= d, "leading dimension smaller than the feature width");
    MGGCN_REQUIRE((const void *)B != (const void *)C, "C must not alias B");
    MGGCN_REQUIRE((uint64_t)n_cols * ldb < (1ull << 40), "B too large");
    MGGCN_REQUIRE(d <= plan->max_d || plan->cap_slots == 0, "feature width exceeds the plan's max_d");
    const hipStream_t st = as_stream(stream);
    const unsigned grid = (plan->cap_items + 3) / 4;
    const bool vec_ok = (d % 4 == 0) && (ldb % 4 == 0) && (ldc % 4 == 0) && reinterpret_cast<uintptr_t>(B) % (4 * sizeof(TB)) == 0 &&
                        aligned16(C);
#define MGGCN_DEV_LAUNCH(KERNEL)                                                                                                   \
    hipLaunchKernelGGL((KERNEL), dim3(grid), dim3(256), 0, st, plan->d_items, plan->totals(), plan->cap_items, indices, values, B, \
                       ldb, C, ldc, plan->d_partial, d, alpha, beta, flags, slope)
    if (vec_ok && d > 64) MGGCN_DEV_LAUNCH((spmm_dev_vec4_kernel<32, 8, TB>));
    else if (vec_ok && d > 32) MGGCN_DEV_LAUNCH((spmm_dev_vec4_kernel<16, 4, TB>));
    else if (vec_ok) MGGCN_DEV_LAUNCH((spmm_dev_vec4_kernel<8, 2, TB>));
    else MGGCN_DEV_LAUNCH((spmm_dev_scalar_kernel<8, TB>));
#undef MGGCN_DEV_LAUNCH
    MGGCN_CHECK_LAUNCH();
    if (plan->cap_split) {
        hipLaunchKernelGGL(spmm_dev_combine_kernel, dim3((plan->cap_split + 3) / 4), dim3(256), 0, st, plan->d_split, plan->totals(),
                           plan->cap_split, plan->d_partial, C, ldc, d, alpha, beta, flags, slope);
        MGGCN_CHECK_LAUNCH();
    }
}

}  // namespace

MGGCN_API void mggcn_spmm_csr_dev_f32(mggcn_stream_t stream, const mggcn_spmm_dev_plan *plan, uint32_t n_rows, uint32_t n_cols,
                                      const uint32_t *indptr, const uint32_t *indices, const float *values, const float *B,
                                      size_t ldb, float *C, size_t ldc, uint32_t d, float alpha, float beta, uint32_t flags,
                                      float slope) {
    (void)indptr;                                          // the items carry the row bounds the plan was built from
    spmm_csr_dev<float>(stream, plan, n_rows, n_cols, indices, values, B, ldb, C, ldc, d, alpha, beta, flags, slope);
}

MGGCN_API void mggcn_spmm_csr_dev_bf16(mggcn_stream_t stream, const mggcn_spmm_dev_plan *plan, uint32_t n_rows, uint32_t n_cols,
                                       const uint32_t *indptr, const uint32_t *indices, const float *values, const uint16_t *B,
                                       size_t ldb, float *C, size_t ldc, uint32_t d, float alpha, float beta, uint32_t flags,
                                       float slope) {
    (void)indptr;
    spmm_csr_dev<uint16_t>(stream, plan, n_rows, n_cols, indices, values, B, ldb, C, ldc, d, alpha, beta, flags, slope);
}
