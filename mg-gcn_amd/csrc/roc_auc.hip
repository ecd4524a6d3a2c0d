// roc_auc.hip -- the integers behind ROC-AUC of a multi-label model (gfx950): sortable keys from the logits, and, over the
// segments that mggcn_radix_sort_pairs_u32 has sorted, the Mann-Whitney statistic of every class and slot.
//
//   keys    a [64 rows x 64 columns] tile per workgroup: the logits, targets and sets are read along the rows (whole lines of
//           the row-major matrices), key and value cross an LDS tile of 65-word rows, and the class-major arrays are stored
//           64 consecutive rows per wave instruction.
//           key   = x = logit + 0.0f (-0.0 becomes +0.0), u = bits(x), (u >> 31) ? ~u : (u | 0x80000000): monotone over every
//                   finite value and the infinities; a NaN lands where this map puts its bit pattern (above +inf with the
//                   sign bit clear, below -inf with it set) -- nothing treats it specially.
//           value = slot << 1 | (target != 0), slot 0 train / 1 val / 2 test / 3 anything else; without sets every row is slot 0.
//   stats   stats[c][k] = (2U, P, N) as three u64, k = train, val, test, other, all ("all": every row, whatever its slot):
//           P / N the positives / negatives of the view, 2U = sum over its positives p of 2 #{negatives with key < key_p}
//           + #{negatives with key == key_p}.  With less(e) = the members of the view with the OTHER label and a key strictly
//           below e's,
//               2U = sum_p less(p) + P N - sum_n less(n)
//           (sum_p #{n: key_n <= key_p} = sum_n (P - #{p: key_p < key_n})), so only the START of a tie group is ever needed.
//           A value has eight categories (slot, label); everything is a count of categories in a prefix of the sorted segment:
//             count   one wave per chunk of kChunk pairs: the chunk's eight category counts (ballots and population counts).
//             scan    one workgroup per class: the exclusive scan of the chunk counts, in place, and the class totals.
//             walk    one wave per chunk in 64-pair rounds, the running category counts and the counts at the start of the
//                     tie group in progress carried from round to round.  A lane's group starts at the last head (key !=
//                     the key before it) at or below it in the round, else where the carried group started.  A chunk whose
//                     first pair continues a group of an earlier chunk finds that group's start by a binary search over the
//                     sorted keys in front of it and counts the categories up to there: the chunk's scanned word plus one
//                     partial chunk.  Tie groups of any length, across any number of chunks, cost one search per chunk.
//                     Each lane adds +less / -less into five 64-bit sums; the wave's sums go out as one partial per chunk.
//             final   one workgroup per class, reduce.h's layout in integers: thread t adds chunks t, t + 256, ... in order,
//                     a butterfly, four waves through LDS.  Integer sums: exact in any order; the order is fixed all the same.
// No atomics, no scratch, no host read.
#include "common.h"

namespace {

constexpr uint32_t kChunk = MGGCN_ROC_AUC_CHUNK;            // pairs per wave
constexpr uint32_t kViews = 5;                              // train, val, test, other, all
constexpr uint32_t kCats = 8;                               // slot << 1 | label

// ---------------------------------------------------------------- keys
__device__ __forceinline__ uint32_t sortable_key(float logit) {
    const uint32_t u = __float_as_uint(logit + 0.0f);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(256) void roc_auc_keys_kernel(const float *__restrict__ logits, size_t ld_logits,
                                                           const int32_t *__restrict__ targets, size_t ld_targets,
                                                           const int32_t *__restrict__ sets, uint32_t n, uint32_t c0, uint32_t nc,
                                                           uint32_t col_tiles, uint32_t *__restrict__ keys,
                                                           uint32_t *__restrict__ vals) {
    __shared__ uint32_t tk[64][65], tv[64][65];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t row0 = (blockIdx.x / col_tiles) * 64, col0 = (blockIdx.x % col_tiles) * 64;
    const uint32_t col = col0 + lane;
    for (uint32_t r = wave; r < 64; r += 4) {                       // a wave reads 64 consecutive columns of one row
        const uint32_t row = row0 + r;
        if (row < n && col < nc) {
            uint32_t slot = 0;
            if (sets != nullptr) {
                const uint32_t s = (uint32_t)sets[row];
                slot = s < 3u ? s : 3u;
            }
            tk[r][lane] = sortable_key(logits[(size_t)row * ld_logits + c0 + col]);
            tv[r][lane] = slot << 1 | (targets[(size_t)row * ld_targets + c0 + col] != 0 ? 1u : 0u);
        }
    }
    __syncthreads();
    const uint32_t row = row0 + lane;
    for (uint32_t c = wave; c < 64; c += 4) {                       // a wave stores 64 consecutive rows of one class
        if (row < n && col0 + c < nc) {
            const size_t at = (size_t)(col0 + c) * n + row;
            keys[at] = tk[lane][c];
            vals[at] = tv[lane][c];
        }
    }
}

// ---------------------------------------------------------------- stats
__device__ __forceinline__ int64_t wave_sum_i64(int64_t v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// the eight category counts of vals[beg, end) of one segment, wave-uniform (every lane ends with the same numbers)
__device__ __forceinline__ void count_categories(const uint32_t *__restrict__ vals, uint32_t beg, uint32_t end, uint32_t lane,
                                                 uint32_t (&count)[kCats]) {
#pragma unroll
    for (uint32_t c = 0; c < kCats; c++) count[c] = 0;
    for (uint32_t i0 = beg; i0 < end; i0 += 64) {                   // wave-uniform trip count: the ballots want every lane
        const uint32_t i = i0 + lane;
        const uint32_t cat = i < end ? (vals[i] & 7u) : kCats;
#pragma unroll
        for (uint32_t c = 0; c < kCats; c++) count[c] += (uint32_t)__popcll(__ballot(cat == c));
    }
}

__global__ __launch_bounds__(256) void roc_auc_count_kernel(const uint32_t *__restrict__ vals, uint32_t n, uint32_t n_chunks,
                                                            uint32_t blocks_per_class, uint32_t *__restrict__ counts) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t cls = blockIdx.x / blocks_per_class;
    const uint32_t chunk = (blockIdx.x % blocks_per_class) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (chunk >= n_chunks) return;
    const uint32_t beg = chunk * kChunk, end = min(beg + kChunk, n);
    uint32_t count[kCats];
    count_categories(vals + (size_t)cls * n, beg, end, lane, count);
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t c = 0; c < kCats; c++) mine = lane == c ? count[c] : mine;
    if (lane < kCats) counts[((size_t)cls * n_chunks + chunk) * kCats + lane] = mine;
}

// one workgroup per class: counts[cls][chunk][cat] becomes its exclusive scan over the chunks, totals[cls][cat] the sum.
// Thread t owns category t & 7 of the chunks [part len, (part + 1) len), part = t >> 3.
__global__ __launch_bounds__(256) void roc_auc_scan_kernel(uint32_t n_chunks, uint32_t *__restrict__ counts,
                                                           uint32_t *__restrict__ totals) {
    __shared__ uint32_t part_sum[32][kCats];
    const uint32_t cat = threadIdx.x & 7, part = threadIdx.x >> 3;
    const uint32_t len = (n_chunks + 31) / 32;
    const uint32_t beg = min(part * len, n_chunks), end = min(beg + len, n_chunks);
    uint32_t *mine = counts + (size_t)blockIdx.x * n_chunks * kCats + cat;
    uint32_t sum = 0;
    for (uint32_t q = beg; q < end; q++) sum += mine[(size_t)q * kCats];
    part_sum[part][cat] = sum;
    __syncthreads();
    uint32_t run = 0;
    for (uint32_t p = 0; p < part; p++) run += part_sum[p][cat];
    for (uint32_t q = beg; q < end; q++) {
        const uint32_t c = mine[(size_t)q * kCats];
        mine[(size_t)q * kCats] = run;
        run += c;
    }
    if (part == 31) totals[(size_t)blockIdx.x * kCats + cat] = run;     // the last part ends with everything in front of it
}

__global__ __launch_bounds__(256) void roc_auc_walk_kernel(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                           uint32_t n, uint32_t n_chunks, uint32_t blocks_per_class,
                                                           const uint32_t *__restrict__ prefix, int64_t *__restrict__ partials) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t cls = blockIdx.x / blocks_per_class;
    const uint32_t chunk = (blockIdx.x % blocks_per_class) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (chunk >= n_chunks) return;
    const uint32_t *k = keys + (size_t)cls * n, *v = vals + (size_t)cls * n;
    const uint32_t *pre = prefix + (size_t)cls * n_chunks * kCats;
    const uint32_t beg = chunk * kChunk, end = min(beg + kChunk, n);
    const uint64_t below = ((uint64_t)1 << lane) - 1;

    uint32_t run[kCats], start[kCats];      // categories in [0, round start) / in [0, start of the tie group in progress)
#pragma unroll
    for (uint32_t c = 0; c < kCats; c++) run[c] = start[c] = pre[(size_t)chunk * kCats + c];
    uint32_t prev_key = 0;                                          // the key in front of the round
    bool have_prev = false;
    if (beg > 0) {
        prev_key = k[beg - 1];
        have_prev = true;
        const uint32_t first = k[beg];
        if (prev_key == first) {                                    // the chunk opens inside a tie group: find where it began
            uint32_t lo = 0, hi = beg - 1;                          // the first index in [0, beg) whose key is `first`
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (k[mid] < first) lo = mid + 1;
                else hi = mid;
            }
            const uint32_t q = lo / kChunk;
            uint32_t part[kCats];
            count_categories(v, q * kChunk, lo, lane, part);
#pragma unroll
            for (uint32_t c = 0; c < kCats; c++) start[c] = pre[(size_t)q * kCats + c] + part[c];
        }
    }

    int64_t acc[kViews] = {0, 0, 0, 0, 0};
    for (uint32_t i0 = beg; i0 < end; i0 += 64) {                   // wave-uniform trip count
        const uint32_t i = i0 + lane;
        const bool valid = i < end;
        const uint32_t key = valid ? k[i] : 0u;
        const uint32_t cat = valid ? (v[i] & 7u) : kCats;
        const uint32_t up = __shfl_up(key, 1);
        const uint32_t before = lane == 0 ? prev_key : up;
        const bool head = valid && (!(lane != 0 || have_prev) || key != before);
        const uint64_t heads = __ballot(head);
        const uint64_t mine = heads & (below | ((uint64_t)1 << lane));      // the heads at or below me
        const bool inside = mine != 0;                                      // my group starts in this round
        const uint32_t h = inside ? 63u - (uint32_t)__clzll(mine) : 0u;
        const uint64_t front = ((uint64_t)1 << h) - 1;                      // the lanes in front of my group's head
        const uint32_t label = cat & 1u, want = cat ^ 1u;
        uint32_t less_slot = 0, less_all = 0;
        uint64_t bits[kCats];
#pragma unroll
        for (uint32_t c = 0; c < kCats; c++) {
            bits[c] = __ballot(cat == c);
            const uint32_t at_start = inside ? run[c] + (uint32_t)__popcll(bits[c] & front) : start[c];
            less_slot = c == want ? at_start : less_slot;
            less_all += (c & 1u) != label ? at_start : 0u;
        }
        if (valid) {
            const int64_t s = label ? (int64_t)less_slot : -(int64_t)less_slot;
            const uint32_t slot = cat >> 1;
#pragma unroll
            for (uint32_t w = 0; w < 4; w++) acc[w] += slot == w ? s : 0;
            acc[4] += label ? (int64_t)less_all : -(int64_t)less_all;
        }
        if (heads != 0) {                                           // the group in progress now starts at the round's last head
            const uint64_t to_last = ((uint64_t)1 << (63u - (uint32_t)__clzll(heads))) - 1;
#pragma unroll
            for (uint32_t c = 0; c < kCats; c++) start[c] = run[c] + (uint32_t)__popcll(bits[c] & to_last);
        }
#pragma unroll
        for (uint32_t c = 0; c < kCats; c++) run[c] += (uint32_t)__popcll(bits[c]);
        prev_key = __shfl(key, 63);                                 // only a full round has a successor
        have_prev = true;
    }
#pragma unroll
    for (uint32_t w = 0; w < kViews; w++) acc[w] = wave_sum_i64(acc[w]);
    int64_t out = 0;
#pragma unroll
    for (uint32_t w = 0; w < kViews; w++) out = lane == w ? acc[w] : out;
    if (lane < kViews) partials[((size_t)cls * n_chunks + chunk) * kViews + lane] = out;
}

// one workgroup per class: the chunk partials in a fixed order, then stats[cls][view] = (S + P N, P, N)
__global__ __launch_bounds__(256) void roc_auc_final_kernel(const int64_t *__restrict__ partials, uint32_t n_chunks,
                                                            const uint32_t *__restrict__ totals, uint64_t *__restrict__ stats) {
    __shared__ int64_t w[kViews][4];
    const int64_t *mine = partials + (size_t)blockIdx.x * n_chunks * kViews;
    int64_t s[kViews] = {0, 0, 0, 0, 0};
    for (uint32_t q = threadIdx.x; q < n_chunks; q += 256) {
#pragma unroll
        for (uint32_t j = 0; j < kViews; j++) s[j] += mine[(size_t)q * kViews + j];
    }
#pragma unroll
    for (uint32_t j = 0; j < kViews; j++) s[j] = wave_sum_i64(s[j]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (uint32_t j = 0; j < kViews; j++) w[j][threadIdx.x >> 6] = s[j];
    }
    __syncthreads();
    if (threadIdx.x < kViews) {
        const uint32_t view = threadIdx.x;
        const uint32_t *t = totals + (size_t)blockIdx.x * kCats;
        uint64_t P = 0, N = 0;
        if (view < 4) {
            N = t[2 * view];
            P = t[2 * view + 1];
        } else {
            for (uint32_t slot = 0; slot < 4; slot++) {
                N += t[2 * slot];
                P += t[2 * slot + 1];
            }
        }
        const int64_t sum = (w[view][0] + w[view][1]) + (w[view][2] + w[view][3]);
        uint64_t *out = stats + ((size_t)blockIdx.x * kViews + view) * 3;
        out[0] = (uint64_t)(sum + (int64_t)(P * N));
        out[1] = P;
        out[2] = N;
    }
}

size_t round256(size_t bytes) { return (bytes + 255) / 256 * 256; }

struct stats_layout {
    size_t n_chunks, counts, totals, partials, bytes;       // byte offsets into work
};

stats_layout layout_of(size_t n, size_t nc) {
    stats_layout l{};
    l.n_chunks = (n + kChunk - 1) / kChunk;
    l.counts = 0;
    l.totals = round256(nc * l.n_chunks * kCats * sizeof(uint32_t));
    l.partials = l.totals + round256(nc * kCats * sizeof(uint32_t));
    l.bytes = l.partials + round256(nc * l.n_chunks * kViews * sizeof(int64_t));
    return l;
}

}  // namespace

// ============================ C ABI =========================================
MGGCN_API void mggcn_roc_auc_keys_f32(mggcn_stream_t stream, const float *logits, size_t ld_logits, const int32_t *targets,
                                      size_t ld_targets, const int32_t *sets, size_t n, size_t c0, size_t nc, uint32_t *keys,
                                      uint32_t *vals) {
    if (n == 0 || nc == 0) return;
    MGGCN_REQUIRE(n < ((size_t)1 << 31) && nc < ((size_t)1 << 31) && n * nc < ((size_t)1 << 31),
                  "roc-auc keys: n * nc must be below 2^31");
    MGGCN_REQUIRE(c0 + nc <= ld_logits && c0 + nc <= ld_targets, "roc-auc keys: the column window exceeds a leading dimension");
    MGGCN_REQUIRE(logits != nullptr && targets != nullptr && keys != nullptr && vals != nullptr, "roc-auc keys: null operand");
    MGGCN_REQUIRE(keys != vals, "roc-auc keys: keys must not alias vals");
    const size_t row_tiles = (n + 63) / 64, col_tiles = (nc + 63) / 64;
    MGGCN_REQUIRE(row_tiles * col_tiles < ((size_t)1 << 31), "roc-auc keys: too many tiles for one grid");
    hipLaunchKernelGGL(roc_auc_keys_kernel, dim3((unsigned)(row_tiles * col_tiles)), dim3(256), 0, as_stream(stream), logits,
                       ld_logits, targets, ld_targets, sets, (uint32_t)n, (uint32_t)c0, (uint32_t)nc, (uint32_t)col_tiles, keys,
                       vals);
    MGGCN_CHECK_LAUNCH();
}

MGGCN_API size_t mggcn_roc_auc_stats_work_bytes(size_t n, size_t nc) {
    if (n == 0 || nc == 0) return 0;
    return layout_of(n, nc).bytes;
}

MGGCN_API void mggcn_roc_auc_stats_u64(mggcn_stream_t stream, const uint32_t *keys, const uint32_t *vals, size_t n, size_t nc,
                                       uint64_t *stats, void *work, size_t work_bytes) {
    if (nc == 0) return;
    MGGCN_REQUIRE(stats != nullptr, "roc-auc stats: null operand");
    const hipStream_t st = as_stream(stream);
    if (n == 0) {                                                   // no row: every (2U, P, N) is zero
        MGGCN_CHECK_HIP(hipMemsetAsync(stats, 0, nc * kViews * 3 * sizeof(uint64_t), st));
        return;
    }
    MGGCN_REQUIRE(n < ((size_t)1 << 31) && nc < ((size_t)1 << 31) && n * nc < ((size_t)1 << 31),
                  "roc-auc stats: n * nc must be below 2^31");
    MGGCN_REQUIRE(keys != nullptr && vals != nullptr, "roc-auc stats: null operand");
    const stats_layout l = layout_of(n, nc);
    MGGCN_REQUIRE(work != nullptr && work_bytes >= l.bytes, "roc-auc stats: work is smaller than mggcn_roc_auc_stats_work_bytes");
    MGGCN_REQUIRE((reinterpret_cast<uintptr_t>(work) & 7u) == 0, "roc-auc stats: work must be 8-byte aligned");
    char *base = static_cast<char *>(work);
    uint32_t *counts = reinterpret_cast<uint32_t *>(base + l.counts), *totals = reinterpret_cast<uint32_t *>(base + l.totals);
    int64_t *partials = reinterpret_cast<int64_t *>(base + l.partials);
    const uint32_t n_chunks = (uint32_t)l.n_chunks, blocks_per_class = (n_chunks + 3) / 4;
    MGGCN_REQUIRE((size_t)blocks_per_class * nc < ((size_t)1 << 31), "roc-auc stats: too many chunks for one grid");
    const dim3 chunk_grid((unsigned)((size_t)blocks_per_class * nc)), class_grid((unsigned)nc), block(256);
    hipLaunchKernelGGL(roc_auc_count_kernel, chunk_grid, block, 0, st, vals, (uint32_t)n, n_chunks, blocks_per_class, counts);
    MGGCN_CHECK_LAUNCH();
    hipLaunchKernelGGL(roc_auc_scan_kernel, class_grid, block, 0, st, n_chunks, counts, totals);
    MGGCN_CHECK_LAUNCH();
    hipLaunchKernelGGL(roc_auc_walk_kernel, chunk_grid, block, 0, st, keys, vals, (uint32_t)n, n_chunks, blocks_per_class, counts,
                       partials);
    MGGCN_CHECK_LAUNCH();
    hipLaunchKernelGGL(roc_auc_final_kernel, class_grid, block, 0, st, partials, n_chunks, totals, stats);
    MGGCN_CHECK_LAUNCH();
}
