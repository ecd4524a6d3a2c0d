// label_input.hip -- masked label inputs of the attention models (gat(label_input=rate); the "label trick" of UniMP, Shi et al.
// 2021): a trained table E [n_classes x width] whose row E[y_i] is added to row i of layer 0's Z = H W + 1 b^T for the
// training rows that are FED this forward, which is [X | M onehot(y)] [W ; E] without the wider GEMM.
//
//   forward    Z[row] += E[cls]   for every listed (row, cls) that is fed;  S_out[row] = fed ? fed_set : kept_set
//   backward   G_E[c] = sum over the fed rows of class c of G_Z[row]
//
// Both walk the list of the training rows only: rows[t] (local row numbers) and cls[t], sorted by (class, row), with the
// segment of class c at [cls_ptr[c], cls_ptr[c + 1]).  Row t is fed when feed_all is set, or when word 0 of
// Philox4x32-10(counter = (0xFFFFFFFF, r & 0xffffffff, r >> 32, epoch), key = (seed & 0xffffffff, seed >> 32)), r = row0 +
// rows[t], is below the threshold: the mask is never stored, both passes regenerate it.  The first counter word is a
// column group that mggcn_dropout_f32 never reaches (its first word is column >> 2 of a row of fewer than 2^32 columns,
// so below 2^30), so a seed shared with dropout shares no bits.
//
// The backward uses no atomics: a class's segment is cut into chunks of kLabelChunk list entries, whatever the grid is; one
// workgroup sums the fed rows of one chunk in list order, a thread owning its columns, and stores one [width] partial in
// the stream's scratch; segsum_final_kernel (reduce.h) adds the partials of each class in chunk order.  Chunk q of class c
// is workgroup cls_ptr[c] / kLabelChunk + c + q: the slots of a class end before the next class's begin, so
// n_train / kLabelChunk + n_classes workgroups cover every chunk and the ones that own none leave at once.
#include "common.h"
#include "philox.h"
#include "reduce.h"
#include "scratch_internal.h"

namespace {

constexpr unsigned kLabelChunk = 64;                 // list entries per partial: one wave draws a chunk's mask
constexpr uint32_t kLabelColumnGroup = 0xFFFFFFFFu;  // the first counter word of every label-input draw
constexpr uint32_t kNoRow = 0xFFFFFFFFu;

__device__ __forceinline__ bool label_fed(uint64_t row, uint32_t threshold, int feed_all, uint64_t seed, uint32_t epoch) {
    if (feed_all) return true;
    const philox4 w = philox4x32_10(kLabelColumnGroup, (uint32_t)row, (uint32_t)(row >> 32), epoch, (uint32_t)seed,
                                    (uint32_t)(seed >> 32));
    return w.w[0] < threshold;
}

template <int V>
__device__ __forceinline__ void li_load(float (&v)[V], const float *p) {
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = *p;
    }
}
template <int V>
__device__ __forceinline__ void li_store(float *p, const float (&v)[V]) {
    if constexpr (V == 4) *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else *p = v[0];
}

// A wave takes 64 list entries at a time: lane l draws entry t0 + l and writes its set, then the wave adds E[cls] to
// Z[row] for the fed entries one after the other, its lanes across the columns.  An entry whose row or class is outside
// the operands is never dereferenced (the lists come from the host; this keeps a wrong one from writing out of bounds).
template <int V>
__global__ __launch_bounds__(256) void label_input_forward_kernel(const uint32_t *__restrict__ rows,
                                                                  const uint32_t *__restrict__ cls, uint32_t n_train,
                                                                  const float *__restrict__ E, size_t lde, uint32_t n_classes,
                                                                  uint32_t width, uint32_t threshold, int feed_all,
                                                                  uint64_t seed, uint32_t epoch, uint64_t row0,
                                                                  int32_t kept_set, int32_t fed_set, float *__restrict__ Z,
                                                                  size_t ldz, size_t n_rows, int32_t *__restrict__ S_out) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t stride = gridDim.x * 256;
    for (uint32_t t0 = (blockIdx.x * 4 + wave) * 64; t0 < n_train; t0 += stride) {
        const uint32_t t = t0 + lane;
        uint32_t row = kNoRow, c = 0;
        bool fed = false;
        if (t < n_train) {
            row = rows[t];
            c = cls[t];
            if (row < n_rows && c < n_classes) {
                fed = label_fed(row0 + row, threshold, feed_all, seed, epoch);
                if (S_out != nullptr) S_out[row] = fed ? fed_set : kept_set;
            }
        }
        unsigned long long todo = __ballot(fed);
        while (todo) {
            const int src = __ffsll(todo) - 1;
            todo &= todo - 1;
            const uint32_t r = __shfl(row, src), k = __shfl(c, src);
            float *z = Z + (size_t)r * ldz;
            const float *e = E + (size_t)k * lde;
            for (uint32_t col = lane * V; col < width; col += 64 * V) {
                float a[V], b[V];
                li_load<V>(a, z + col);
                li_load<V>(b, e + col);
#pragma unroll
                for (int v = 0; v < V; v++) a[v] += b[v];
                li_store<V>(z + col, a);
            }
        }
    }
}

// the first slot of class c; strictly increasing in c
__device__ __forceinline__ uint32_t label_slot0(const uint32_t *cls_ptr, uint32_t c) { return cls_ptr[c] / kLabelChunk + c; }

// One workgroup per slot.  The first wave draws the chunk's mask and packs the fed rows into LDS in list order (a lane's
// position is the number of fed lanes below it); every thread then sums its columns over those rows, in that order.
template <int V>
__global__ __launch_bounds__(256) void label_input_backward_kernel(const uint32_t *__restrict__ rows,
                                                                   const uint32_t *__restrict__ cls_ptr, uint32_t n_train,
                                                                   uint32_t n_classes, uint32_t width, uint32_t threshold,
                                                                   int feed_all, uint64_t seed, uint32_t epoch, uint64_t row0,
                                                                   const float *__restrict__ G, size_t ldg, size_t n_rows,
                                                                   float *__restrict__ partials) {
    __shared__ uint32_t s_row[kLabelChunk];
    __shared__ uint32_t s_count;
    const uint32_t slot = blockIdx.x;
    uint32_t lo = 0, hi = n_classes;                    // the class whose slots hold mine: the last c with slot0(c) <= slot
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (label_slot0(cls_ptr, mid) <= slot) lo = mid;
        else hi = mid;
    }
    const uint32_t seg_end = min(cls_ptr[lo + 1], n_train);
    const uint64_t begin = (uint64_t)cls_ptr[lo] + (uint64_t)(slot - label_slot0(cls_ptr, lo)) * kLabelChunk;
    if (begin >= seg_end) return;                       // a slot without a chunk (uniform: before any barrier)
    const uint32_t count = min(kLabelChunk, seg_end - (uint32_t)begin);
    if (threadIdx.x < 64) {
        uint32_t row = kNoRow;
        bool fed = false;
        if (threadIdx.x < count) {
            row = rows[begin + threadIdx.x];
            fed = row < n_rows && label_fed(row0 + row, threshold, feed_all, seed, epoch);
        }
        const unsigned long long mask = __ballot(fed);
        if (fed) s_row[__popcll(mask & ((1ull << threadIdx.x) - 1))] = row;
        if (threadIdx.x == 0) s_count = (uint32_t)__popcll(mask);
    }
    __syncthreads();
    const uint32_t n_fed = s_count;
    for (uint32_t col = threadIdx.x * V; col < width; col += blockDim.x * V) {
        float acc[V];
#pragma unroll
        for (int v = 0; v < V; v++) acc[v] = 0.f;
#pragma unroll 4
        for (uint32_t k = 0; k < n_fed; k++) {
            float g[V];
            li_load<V>(g, G + (size_t)s_row[k] * ldg + col);
#pragma unroll
            for (int v = 0; v < V; v++) acc[v] += g[v];
        }
        li_store<V>(partials + (size_t)slot * width + col, acc);
    }
}

bool rows_aligned16(const void *p, size_t ld) { return aligned16(p) && ld % 4 == 0; }

}  // namespace

// ============================ C ABI =========================================
MGGCN_API void mggcn_label_input_forward_f32(mggcn_stream_t stream, const uint32_t *rows, const uint32_t *cls, size_t n_train,
                                             const float *E, size_t lde, size_t n_classes, size_t width, uint32_t threshold,
                                             int feed_all, uint64_t seed, uint32_t epoch, uint64_t row0, int32_t kept_set,
                                             int32_t fed_set, float *Z, size_t ldz, size_t n_rows, int32_t *S_out) {
    MGGCN_REQUIRE(n_classes >= 1 && n_classes <= MGGCN_LABEL_INPUT_MAX_CLASSES, "label input supports 1 <= n_classes <= 256");
    MGGCN_REQUIRE(width >= 1 && width <= MGGCN_LABEL_INPUT_MAX_WIDTH, "label input supports 1 <= width <= 3072 columns");
    MGGCN_REQUIRE(lde >= width && ldz >= width, "label input: a leading dimension is below width");
    MGGCN_REQUIRE(n_train < (1u << 31) && n_rows < (1ull << 32), "label input: the row lists are 32-bit");
    if (!n_train) return;
    MGGCN_REQUIRE(rows != nullptr && cls != nullptr && E != nullptr && Z != nullptr, "label input: null operand");
    const unsigned grid = stream_grid(n_train);
    const bool vec = width % 4 == 0 && rows_aligned16(E, lde) && rows_aligned16(Z, ldz);
    if (vec)
        hipLaunchKernelGGL(label_input_forward_kernel<4>, dim3(grid), dim3(256), 0, as_stream(stream), rows, cls,
                           (uint32_t)n_train, E, lde, (uint32_t)n_classes, (uint32_t)width, threshold, feed_all, seed, epoch,
                           row0, kept_set, fed_set, Z, ldz, n_rows, S_out);
    else
        hipLaunchKernelGGL(label_input_forward_kernel<1>, dim3(grid), dim3(256), 0, as_stream(stream), rows, cls,
                           (uint32_t)n_train, E, lde, (uint32_t)n_classes, (uint32_t)width, threshold, feed_all, seed, epoch,
                           row0, kept_set, fed_set, Z, ldz, n_rows, S_out);
    MGGCN_CHECK_LAUNCH();
}

MGGCN_API void mggcn_label_input_backward_f32(mggcn_stream_t stream, const uint32_t *rows, const uint32_t *cls,
                                              const uint32_t *cls_ptr, size_t n_train, size_t n_classes, size_t width,
                                              uint32_t threshold, int feed_all, uint64_t seed, uint32_t epoch, uint64_t row0,
                                              const float *G_Z, size_t ldg, size_t n_rows, float *G_E, size_t ldge) {
    MGGCN_REQUIRE(n_classes >= 1 && n_classes <= MGGCN_LABEL_INPUT_MAX_CLASSES, "label input supports 1 <= n_classes <= 256");
    MGGCN_REQUIRE(width >= 1 && width <= MGGCN_LABEL_INPUT_MAX_WIDTH, "label input supports 1 <= width <= 3072 columns");
    MGGCN_REQUIRE(ldg >= width && ldge >= width, "label input backward: a leading dimension is below width");
    MGGCN_REQUIRE(n_train < (1u << 31) && n_rows < (1ull << 32), "label input: the row lists are 32-bit");
    MGGCN_REQUIRE(G_E != nullptr, "label input backward: null G_E");
    const hipStream_t st = as_stream(stream);
    const dim3 final_grid((unsigned)((width + 63) / 64), (unsigned)n_classes);
    if (!n_train) {                                     // the sums over no rows
        hipLaunchKernelGGL(segsum_final_kernel<kLabelChunk>, final_grid, dim3(256), 0, st, nullptr, nullptr, 0u,
                           (uint32_t)width, G_E, ldge);
        MGGCN_CHECK_LAUNCH();
        return;
    }
    MGGCN_REQUIRE(rows != nullptr && cls != nullptr && cls_ptr != nullptr && G_Z != nullptr,
                  "label input backward: null operand");
    const size_t slots = n_train / kLabelChunk + n_classes;
    float *partials = stream_scratch(st, scratch_kind::colsums, slots * width);
    // the partials are the scratch's own (hipMalloc: 256-byte aligned) and `width` floats apart
    const bool vec = width % 4 == 0 && rows_aligned16(G_Z, ldg);
    const size_t lanes = vec ? width / 4 : width;
    const unsigned block = (unsigned)(lanes >= 256 ? 256 : (lanes + 63) / 64 * 64);
    if (vec)
        hipLaunchKernelGGL(label_input_backward_kernel<4>, dim3((unsigned)slots), dim3(block), 0, st, rows, cls_ptr,
                           (uint32_t)n_train, (uint32_t)n_classes, (uint32_t)width, threshold, feed_all, seed, epoch, row0,
                           G_Z, ldg, n_rows, partials);
    else
        hipLaunchKernelGGL(label_input_backward_kernel<1>, dim3((unsigned)slots), dim3(block), 0, st, rows, cls_ptr,
                           (uint32_t)n_train, (uint32_t)n_classes, (uint32_t)width, threshold, feed_all, seed, epoch, row0,
                           G_Z, ldg, n_rows, partials);
    MGGCN_CHECK_LAUNCH();
    hipLaunchKernelGGL(segsum_final_kernel<kLabelChunk>, final_grid, dim3(256), 0, st, partials, cls_ptr, (uint32_t)n_train,
                       (uint32_t)width, G_E, ldge);
    MGGCN_CHECK_LAUNCH();
}
