// radix_sort.hip -- stable segmented LSD radix sort of (u32 key, u32 value) pairs on the device (gfx950): the library's one way
// to put anything in order.  n_seg segments of seg_len pairs each, every segment sorted on its own, ascending on the key bits
// [begin_bit, end_bit), equal keys in their input order.
//
// One pass per 8-bit digit (the last digit of a range may be narrower), three steps per pass, none of which waits on another
// workgroup -- no look-back, no flags:
//   histogram  one workgroup per tile of kSortTile pairs of one segment: the tile's count of every digit in integer LDS
//              counters (their result does not depend on the order of the adds), stored at hist[(seg 256 + digit) tiles + tile].
//   scan       ONE exclusive scan over the whole table with mggcn_edge_sample_scan_u32 (three launches).  The table is laid
//              out (segment, digit, tile) and every segment holds exactly seg_len pairs, so the scanned word IS the absolute
//              position seg seg_len + (pairs of smaller digits in the segment) + (pairs of this digit in earlier tiles).
//   scatter    the tile again, wave w owning its pairs [w kSortTile / 4, (w + 1) kSortTile / 4) in 64-pair rounds.  In a round
//              the lanes with my digit are eight ballots ANDed together; my rank among them is the population count of the lanes
//              below me, and a per-wave LDS counter per digit carries the count from round to round (read by all peers, bumped
//              by one of them; the wave runs in lock step).  After the rounds thread d turns the four wave counts of digit d
//              into four bases on top of the scanned word.  position = base[wave][digit] + rank: a function of the input alone
//              -- no atomic's arrival order is ever a position, so the sort is stable and every call gives the same bits.
// Source and destination swap between passes; an odd number of passes ends with a device-to-device copy so that the result
// is always in keys / vals.  Nothing outside [0, n_seg seg_len) of the four arrays is read or written.
#include <algorithm>

#include "common.h"

namespace {

constexpr uint32_t kSortTile = MGGCN_RADIX_SORT_TILE;       // pairs per workgroup
constexpr uint32_t kSortThreads = 256;
constexpr uint32_t kSortRounds = kSortTile / kSortThreads;  // 64-pair rounds per wave
constexpr uint32_t kDigits = 256;

struct sort_geometry {
    uint32_t seg_len, n_tiles;      // pairs per segment, tiles per segment
    uint32_t shift, mask;           // digit = (key >> shift) & mask
};

__global__ __launch_bounds__(256) void radix_sort_histogram_kernel(const uint32_t *__restrict__ keys, sort_geometry g,
                                                                   uint32_t *__restrict__ hist) {
    __shared__ uint32_t count[kDigits];
    const uint32_t seg = blockIdx.x / g.n_tiles, tile = blockIdx.x % g.n_tiles;
    count[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t beg = tile * kSortTile, end = min(beg + kSortTile, g.seg_len);
    const uint32_t *src = keys + (size_t)seg * g.seg_len;
    for (uint32_t i = beg + threadIdx.x; i < end; i += kSortThreads) atomicAdd(&count[(src[i] >> g.shift) & g.mask], 1u);
    __syncthreads();
    hist[((size_t)seg * kDigits + threadIdx.x) * g.n_tiles + tile] = count[threadIdx.x];
}

__global__ __launch_bounds__(256) void radix_sort_scatter_kernel(const uint32_t *__restrict__ keys_in,
                                                                 const uint32_t *__restrict__ vals_in, sort_geometry g,
                                                                 const uint32_t *__restrict__ offsets,
                                                                 uint32_t *__restrict__ keys_out, uint32_t *__restrict__ vals_out) {
    __shared__ uint32_t base[4][kDigits];                           // per wave: the running count, then the digit's base
    const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t seg = blockIdx.x / g.n_tiles, tile = blockIdx.x % g.n_tiles;
    const uint64_t below = ((uint64_t)1 << lane) - 1;               // the lanes in front of mine
#pragma unroll
    for (uint32_t w = 0; w < 4; w++) base[w][threadIdx.x] = 0;
    __syncthreads();

    const size_t seg0 = (size_t)seg * g.seg_len;
    const uint32_t first = tile * kSortTile + wave * (kSortTile / 4);
    uint32_t key[kSortRounds], val[kSortRounds], where[kSortRounds];    // where = rank inside the wave << 8 | digit
#pragma unroll
    for (uint32_t r = 0; r < kSortRounds; r++) {
        const uint32_t i = first + r * 64 + lane;
        key[r] = i < g.seg_len ? keys_in[seg0 + i] : 0u;
        val[r] = i < g.seg_len ? vals_in[seg0 + i] : 0u;
    }
#pragma unroll
    for (uint32_t r = 0; r < kSortRounds; r++) {
        const bool valid = first + r * 64 + lane < g.seg_len;
        const uint32_t digit = (key[r] >> g.shift) & g.mask;
        uint64_t peers = __ballot(valid);                           // the valid lanes that hold my digit
#pragma unroll
        for (uint32_t b = 0; b < 8; b++) {
            const bool bit = (digit >> b) & 1u;
            const uint64_t set = __ballot(valid && bit);
            peers &= bit ? set : ~set;
        }
        const uint32_t before = base[wave][digit];                  // every peer reads the same word
        __builtin_amdgcn_wave_barrier();
        where[r] = (before + (uint32_t)__popcll(peers & below)) << 8 | digit;
        if (valid && (peers & below) == 0) base[wave][digit] = before + (uint32_t)__popcll(peers);      // the first peer bumps it
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    {
        const uint32_t d = threadIdx.x;                             // thread d: the four waves' counts of digit d become bases
        uint32_t at = offsets[((size_t)seg * kDigits + d) * g.n_tiles + tile];
#pragma unroll
        for (uint32_t w = 0; w < 4; w++) {
            const uint32_t c = base[w][d];
            base[w][d] = at;
            at += c;
        }
    }
    __syncthreads();
    const size_t total_end = seg0 + g.seg_len;
#pragma unroll
    for (uint32_t r = 0; r < kSortRounds; r++) {
        const bool valid = first + r * 64 + lane < g.seg_len;
        const size_t at = (size_t)base[wave][where[r] & 255u] + (where[r] >> 8);
        if (valid && at >= seg0 && at < total_end) {                // holds by construction: histogram counted the same digits
            keys_out[at] = key[r];
            vals_out[at] = val[r];
        }
    }
}

size_t hist_words(size_t n_seg, size_t seg_len) {
    const size_t n_tiles = (seg_len + kSortTile - 1) / kSortTile;
    return n_seg * kDigits * n_tiles;
}

bool overlap(const void *a, const void *b, size_t bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + bytes && y < x + bytes;
}

}  // namespace

// ============================ C ABI =========================================
MGGCN_API size_t mggcn_radix_sort_work_bytes(size_t n_seg, size_t seg_len) {
    if (n_seg == 0 || seg_len == 0) return 0;
    return (2 * hist_words(n_seg, seg_len) + 1) * sizeof(uint32_t);      // the histogram and its scan (one word more)
}

MGGCN_API void mggcn_radix_sort_pairs_u32(mggcn_stream_t stream, size_t n_seg, size_t seg_len, uint32_t *keys, uint32_t *vals,
                                          uint32_t *keys_alt, uint32_t *vals_alt, int begin_bit, int end_bit, void *work,
                                          size_t work_bytes) {
    MGGCN_REQUIRE(0 <= begin_bit && begin_bit < end_bit && end_bit <= 32, "radix sort: 0 <= begin_bit < end_bit <= 32");
    if (n_seg == 0 || seg_len == 0) return;
    MGGCN_REQUIRE(seg_len < ((size_t)1 << 31) && n_seg < ((size_t)1 << 31) && n_seg * seg_len < ((size_t)1 << 31),
                  "radix sort: n_seg * seg_len must be below 2^31");
    const size_t total = n_seg * seg_len, bytes = total * sizeof(uint32_t);
    MGGCN_REQUIRE(keys != nullptr && vals != nullptr && keys_alt != nullptr && vals_alt != nullptr, "radix sort: null operand");
    const void *arrays[4] = {keys, vals, keys_alt, vals_alt};
    for (int a = 0; a < 4; a++)
        for (int b = a + 1; b < 4; b++)
            MGGCN_REQUIRE(!overlap(arrays[a], arrays[b], bytes), "radix sort: keys, vals, keys_alt and vals_alt must not overlap");
    MGGCN_REQUIRE(work != nullptr && work_bytes >= mggcn_radix_sort_work_bytes(n_seg, seg_len),
                  "radix sort: work is smaller than mggcn_radix_sort_work_bytes");
    const size_t words = hist_words(n_seg, seg_len);
    const size_t n_tiles = (seg_len + kSortTile - 1) / kSortTile;
    MGGCN_REQUIRE(n_seg * n_tiles < ((size_t)1 << 31), "radix sort: too many tiles for one grid");
    uint32_t *hist = static_cast<uint32_t *>(work), *offsets = hist + words;
    const hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)(n_seg * n_tiles)), block(kSortThreads);
    uint32_t *src_k = keys, *src_v = vals, *dst_k = keys_alt, *dst_v = vals_alt;
    for (int shift = begin_bit; shift < end_bit; shift += 8) {
        const int bits = std::min(8, end_bit - shift);
        const sort_geometry g{(uint32_t)seg_len, (uint32_t)n_tiles, (uint32_t)shift, (1u << bits) - 1u};
        hipLaunchKernelGGL(radix_sort_histogram_kernel, grid, block, 0, st, src_k, g, hist);
        MGGCN_CHECK_LAUNCH();
        mggcn_edge_sample_scan_u32(stream, hist, words, offsets);
        hipLaunchKernelGGL(radix_sort_scatter_kernel, grid, block, 0, st, src_k, src_v, g, offsets, dst_k, dst_v);
        MGGCN_CHECK_LAUNCH();
        std::swap(src_k, dst_k);
        std::swap(src_v, dst_v);
    }
    if (src_k != keys) {                                            // an odd number of passes left the result in the scratch
        MGGCN_CHECK_HIP(hipMemcpyAsync(keys, src_k, bytes, hipMemcpyDeviceToDevice, st));
        MGGCN_CHECK_HIP(hipMemcpyAsync(vals, src_v, bytes, hipMemcpyDeviceToDevice, st));
    }
}
