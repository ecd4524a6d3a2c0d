// elementwise.hip -- the element-wise / row / loss / optimiser kernels of one epoch.
//
// One entry point per live launcher of the reference's device TU
// (src/cuda_utils.cu:229-390, kernels :12-227).  The reference launches
// min(ceil(size/1024),1280) x 1024 threads and walks rows with ONE THREAD PER ROW
// (serial, uncoalesced loop over the m columns: max_rows, max_row_indices, ...).
// Here: streaming kernels move 16 B per lane (float4) when the buffer allows it,
// row kernels give each row to a group of lanes inside a wave64 and reduce with
// DPP/LDS-crossbar shuffles, grids are sized for 256 CUs.  All of these are HBM
// passes over [n x m] fp32; none is reshaped into a GEMM.
#include <algorithm>

#include "common.h"
#include "philox.h"
#include "reduce.h"
#include "row_group.h"
#include "scratch_internal.h"

namespace {

__device__ __forceinline__ float lrelu(float x, float slope) {
    const float y = slope * x;
    return x > y ? x : y;
}

// ---- streaming helpers ----------------------------------------------------
template <typename F>
__global__ __launch_bounds__(256) void map1_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                   size_t size, F f) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < size; i += stride) out[i] = f(in[i]);
}

template <typename F>
__global__ __launch_bounds__(256) void map1_vec4_kernel(const float4 *__restrict__ in,
                                                        float4 *__restrict__ out, size_t size4, F f) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < size4; i += stride) {
        float4 x = in[i];
        x.x = f(x.x); x.y = f(x.y); x.z = f(x.z); x.w = f(x.w);
        out[i] = x;
    }
}

template <typename F>
__global__ __launch_bounds__(256) void map2_kernel(const float *__restrict__ a, const float *__restrict__ b,
                                                   float *__restrict__ out, size_t size, F f) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < size; i += stride)
        out[i] = f(a[i], b[i]);
}

template <typename F>
__global__ __launch_bounds__(256) void map2_vec4_kernel(const float4 *__restrict__ a,
                                                        const float4 *__restrict__ b,
                                                        float4 *__restrict__ out, size_t size4, F f) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < size4; i += stride) {
        const float4 x = a[i], y = b[i];
        float4 o;
        o.x = f(x.x, y.x); o.y = f(x.y, y.y); o.z = f(x.z, y.z); o.w = f(x.w, y.w);
        out[i] = o;
    }
}

template <typename F>
void launch_map1(hipStream_t st, const float *in, float *out, size_t size, F f) {
    if (!size) return;
    if (size % 4 == 0 && aligned16(in) && aligned16(out)) {
        hipLaunchKernelGGL(map1_vec4_kernel<F>, dim3(stream_grid(size / 4)), dim3(256), 0, st,
                           reinterpret_cast<const float4 *>(in), reinterpret_cast<float4 *>(out), size / 4, f);
    } else {
        hipLaunchKernelGGL(map1_kernel<F>, dim3(stream_grid(size)), dim3(256), 0, st, in, out, size, f);
    }
    MGGCN_CHECK_LAUNCH();
}

template <typename F>
void launch_map2(hipStream_t st, const float *a, const float *b, float *out, size_t size, F f) {
    if (!size) return;
    if (size % 4 == 0 && aligned16(a) && aligned16(b) && aligned16(out)) {
        hipLaunchKernelGGL(map2_vec4_kernel<F>, dim3(stream_grid(size / 4)), dim3(256), 0, st,
                           reinterpret_cast<const float4 *>(a), reinterpret_cast<const float4 *>(b),
                           reinterpret_cast<float4 *>(out), size / 4, f);
    } else {
        hipLaunchKernelGGL(map2_kernel<F>, dim3(stream_grid(size)), dim3(256), 0, st, a, b, out, size, f);
    }
    MGGCN_CHECK_LAUNCH();
}

struct LreluFwd { float s; __device__ float operator()(float x) const { return lrelu(x, s); } };
struct LreluBwd { float s; __device__ float operator()(float in, float g) const { return in > 0.f ? g : s * g; } };
// The contraction is written out: left to the compiler, a * x + b * y became fmaf(a, x, b * y) in the float4 kernel and
// two roundings in the scalar one, so the result depended on the pointers' alignment and on size % 4.
struct Axpby { float a, b; __device__ float operator()(float x, float y) const { return fmaf(a, x, b * y); } };
struct Aaxpby { float a, b; __device__ float operator()(float x, float y) const { return fmaf(a * x, x, b * y); } };
struct Axpy { float a; __device__ float operator()(float x, float y) const { return fmaf(a, x, y); } };
struct Scal { float a; __device__ float operator()(float x) const { return x * a; } };

// ---- row-indexed streaming kernels ----------------------------------------
// mat[i] (= | +=) row[i % m]          reference src/cuda_utils.cu:40-51
__global__ __launch_bounds__(256) void broadcast_rows_kernel(const float *__restrict__ row,
                                                             float *__restrict__ mat, size_t size,
                                                             size_t m, int discard) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < size; i += stride) {
        const float r = row[i % m];
        mat[i] = discard ? r : mat[i] + r;
    }
}

// mat[i] /= scalar[i / m]             reference src/cuda_utils.cu:75-79
__global__ __launch_bounds__(256) void scale_rows_kernel(float *__restrict__ mat,
                                                         const float *__restrict__ scalar, size_t size,
                                                         size_t m) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < size; i += stride)
        mat[i] /= scalar[i / m];
}

// out[i] = exp(mat[i] - scalar[i / m]) reference src/cuda_utils.cu:192-200
__global__ __launch_bounds__(256) void subtract_rows_exp_kernel(const float *__restrict__ mat,
                                                                const float *__restrict__ scalar,
                                                                float *__restrict__ out, size_t size,
                                                                size_t m) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < size; i += stride)
        out[i] = expf(mat[i] - scalar[i / m]);
}

// ---- one wave64 per row ---------------------------------------------------
// row max                              reference src/cuda_utils.cu:95-104
__global__ __launch_bounds__(256) void max_rows_kernel(const float *__restrict__ mat,
                                                       float *__restrict__ maxs, size_t n_rows, size_t m) {
    const int lane = threadIdx.x & 63;
    const size_t wstride = ((size_t)gridDim.x * blockDim.x) >> 6;
    for (size_t r = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; r < n_rows; r += wstride) {
        float mx = -INFINITY;
        for (size_t c = lane; c < m; c += 64) mx = fmaxf(mx, mat[r * m + c]);
        mx = wave_max(mx);
        if (lane == 0) maxs[r] = mx;
    }
}

// argmax, first maximum wins           reference src/cuda_utils.cu:119-133
__device__ __forceinline__ void argmax_combine(float &v, uint32_t &i, float ov, uint32_t oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}
__global__ __launch_bounds__(256) void max_row_indices_kernel(const float *__restrict__ mat,
                                                              int32_t *__restrict__ maxs, size_t n_rows,
                                                              size_t m) {
    const int lane = threadIdx.x & 63;
    const size_t wstride = ((size_t)gridDim.x * blockDim.x) >> 6;
    for (size_t r = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; r < n_rows; r += wstride) {
        float mx = -INFINITY;
        uint32_t idx = 0xFFFFFFFFu;
        for (size_t c = lane; c < m; c += 64) {
            const float x = mat[r * m + c];
            if (x > mx) { mx = x; idx = (uint32_t)c; }   // strict >: earlier column of this lane wins
        }
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            const float ov = __shfl_xor(mx, off);
            const uint32_t oi = __shfl_xor(idx, off);
            argmax_combine(mx, idx, ov, oi);
        }
        // all -inf / NaN row: the reference's strict `max < x` never fires -> index 0
        if (lane == 0) maxs[r] = idx == 0xFFFFFFFFu ? 0 : (int32_t)idx;
    }
}

// values[r] = log(mat[r, indices[r]])  reference src/cuda_utils.cu:142-150
__global__ __launch_bounds__(256) void index_log_rows_kernel(const float *__restrict__ mat,
                                                             const int32_t *__restrict__ indices,
                                                             float *__restrict__ values, size_t n_rows,
                                                             size_t m) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += stride)
        values[r] = logf(mat[r * m + (size_t)indices[r]]);
}

// mat[r, indices[r]] += alpha           reference src/cuda_utils.cu:159-164
__global__ __launch_bounds__(256) void add_indexed_rows_kernel(float *__restrict__ mat,
                                                               const int32_t *__restrict__ indices,
                                                               float alpha, size_t n_rows, size_t m) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += stride)
        mat[r * m + (size_t)indices[r]] += alpha;
}

// out[i] = (a[i] == b[i])               reference src/cuda_utils.cu:180-184
__global__ __launch_bounds__(256) void is_equal_kernel(const int32_t *__restrict__ a,
                                                       const int32_t *__restrict__ b,
                                                       float *__restrict__ out, size_t size) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < size; i += stride)
        out[i] = (float)(a[i] == b[i]);
}

// param -= step * m / (sqrt(v / c2) + eps)   reference src/cuda_utils.cu:208-218
__global__ __launch_bounds__(256) void adam_final_kernel(float *__restrict__ param,
                                                         const float *__restrict__ m,
                                                         const float *__restrict__ v, float step, float c2,
                                                         float eps, size_t size) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < size; i += stride)
        param[i] -= step * m[i] / (sqrtf(v[i] / c2) + eps);
}

// ---- |x| sum: the reduction tree of reduce.h (reproducible) -----------------
constexpr unsigned kAsumBlocks = 1024;
constexpr unsigned kXentBlocks = kNumCU * 8;               // grid cap of the fused losses (stream_grid)

__global__ __launch_bounds__(256) void abssum_partial_kernel(const float *__restrict__ A, size_t size,
                                                             float *__restrict__ partial) {
    __shared__ float wsum[1][4];
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    float s = 0.f;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < size; i += stride) s += fabsf(A[i]);
    const float v[1] = {wave_sum(s)};
    block_fold(v, wsum, partial + blockIdx.x);
}

// ---- fused softmax + cross-entropy + argmax + gradient ---------------------
// One wave64 per row; the row's m <= 64*K logits live in K registers per lane.
constexpr int kXentMaxPerLane = 16;  // m <= 1024

// R rows are in flight per wave (their loads issued together): with one row at a time every row is a dependent
// HBM round trip -- load, six shuffle steps, store -- and the pass was latency-bound at 0.7 TB/s (r01: 110 us for
// the 76 MB of the [233 k x 41] logits); four rows in flight hide it.
// (src and dst may be the same matrix: a row is read whole before any of it is written)
//
// Split = true is the split-aware instance (mggcn_softmax_xent_split_from_f32): S[r] is loaded next to Y[r], a row
// outside train_set stores +0.0 in every column, and the (loss, correct) pair of a row goes to the accumulator pair of
// its slot (0 train / 1 validation / 2 test / 3 anything else) by selects -- the other three add +0.0, which keeps their
// bits.  Grid, row order per wave and the order of every sum are those of Split = false, so with S == train_set
// everywhere the gradient and the training slot's pair are the bits of the plain pass.
constexpr int xent_slots(bool split) { return split ? 4 : 1; }
__device__ __forceinline__ uint32_t xent_slot(int32_t s) { return (uint32_t)s < 3u ? (uint32_t)s : 3u; }

// A row's (loss, correct) pair goes to its slot: slot 0 lives in the pair of scalars the plain form has, slots 1..3 in
// loss_x / corr_x.
__device__ __forceinline__ void xent_add_by_slot(int32_t set, float lt, float ct, float &loss_acc, float &corr_acc,
                                                 float (&loss_x)[3], float (&corr_x)[3]) {
    const uint32_t slot = xent_slot(set);
    loss_acc += slot == 0u ? lt : 0.f;
    corr_acc += slot == 0u ? ct : 0.f;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        loss_x[j] += slot == (uint32_t)(j + 1) ? lt : 0.f;
        corr_x[j] += slot == (uint32_t)(j + 1) ? ct : 0.f;
    }
}

// The end of both fused kernels: the wave-reduced pairs as [slot][loss, correct], one set per workgroup in the partials
// ([workgroup][slot][loss, correct]), summed by sums_final_kernel<2 * slots>.
template <bool Split>
__device__ __forceinline__ void xent_fold(float loss_acc, float corr_acc, const float (&loss_x)[3], const float (&corr_x)[3],
                                          float (*lds)[4], float *__restrict__ partials) {
    constexpr int NV = 2 * xent_slots(Split);
    float v[NV];
    v[0] = loss_acc; v[1] = corr_acc;
    if constexpr (Split) {
#pragma unroll
        for (int j = 0; j < 3; j++) { v[2 * j + 2] = loss_x[j]; v[2 * j + 3] = corr_x[j]; }
    }
    block_fold(v, lds, partials + (size_t)NV * blockIdx.x);
}

// (S and train_set come last: the arguments of the plain instances keep their places)
template <int K, int R, bool Split>
__global__ __launch_bounds__(256) void softmax_xent_fused_kernel(const float *src, float *dst,
                                                                 const int32_t *__restrict__ Y,
                                                                 size_t n_rows, size_t m, float grad_scale,
                                                                 float *__restrict__ partials,
                                                                 const int32_t *__restrict__ S, int32_t train_set) {
    __shared__ float s_sums[2 * xent_slots(Split)][4];    // [slot][loss, correct][wave]
    const int lane = threadIdx.x & 63;
    const size_t wstride = ((size_t)gridDim.x * blockDim.x) >> 6;
    float loss_acc = 0.f, corr_acc = 0.f;
    float loss_x[3] = {0.f, 0.f, 0.f}, corr_x[3] = {0.f, 0.f, 0.f};      // slots 1..3, Split only
    for (size_t r0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; r0 < n_rows; r0 += wstride * R) {
        float x[R][K];
        int32_t y[R], s[Split ? R : 1];
#pragma unroll
        for (int q = 0; q < R; q++) {                     // all loads first
            const size_t r = r0 + (size_t)q * wstride;
            const bool live = r < n_rows;                 // wave-uniform
            y[q] = live ? Y[r] : 0;
            if constexpr (Split) s[q] = live ? S[r] : 0;
#pragma unroll
            for (int k = 0; k < K; k++) {
                const size_t c = (size_t)lane + 64u * k;
                x[q][k] = (live && c < m) ? src[r * m + c] : -INFINITY;
            }
        }
#pragma unroll
        for (int q = 0; q < R; q++) {
            const size_t r = r0 + (size_t)q * wstride;
            if (r >= n_rows) break;                       // wave-uniform
            // row maximum (wave-uniform) and the FIRST column holding it (strict `<` of the reference, cuda_utils.cu:126)
            float mx = -INFINITY;
#pragma unroll
            for (int k = 0; k < K; k++) mx = fmaxf(mx, x[q][k]);
            mx = wave_max_dpp(mx);
            uint32_t idx = 0xFFFFFFFFu;
#pragma unroll
            for (int k = K - 1; k >= 0; k--) {
                const unsigned long long hit = __ballot(x[q][k] == mx && (size_t)lane + 64u * k < m);
                if (hit) idx = (uint32_t)__builtin_ctzll(hit) + 64u * (uint32_t)k;        // lower k = lower columns: last writer wins
            }
            float sum = 0.f;
#pragma unroll
            for (int k = 0; k < K; k++) {
                const size_t c = (size_t)lane + 64u * k;
                x[q][k] = c < m ? expf(x[q][k] - mx) : 0.f;
                sum += x[q][k];
            }
            sum = wave_sum_dpp(sum);
            float py = 0.f;                                    // p_y: read from the lane that holds column y
#pragma unroll
            for (int k = 0; k < K; k++) {
                const size_t c = (size_t)lane + 64u * k;
                if (c < m) {
                    const float o = x[q][k] / sum;
                    const bool hit = (int32_t)c == y[q];
                    const float g = (hit ? o - 1.f : o) * grad_scale;
                    if constexpr (Split) dst[r * m + c] = s[q] == train_set ? g : 0.f;
                    else dst[r * m + c] = g;
                    x[q][k] = o;
                }
            }
            if (y[q] >= 0 && (size_t)y[q] < m) {               // wave-uniform
#pragma unroll
                for (int k = 0; k < K; k++)
                    if ((y[q] >> 6) == k)
                        py = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x[q][k]), y[q] & 63));
            }
            if (lane == 0) {
                // argmax of the softmax output == argmax of the logits (exp is monotone);
                // a row whose maximum never beat -inf reports index 0 like the reference
                if constexpr (Split) {
                    xent_add_by_slot(s[q], fabsf(logf(py)), ((idx == 0xFFFFFFFFu ? 0 : (int32_t)idx) == y[q]) ? 1.f : 0.f,
                                     loss_acc, corr_acc, loss_x, corr_x);
                } else {
                    loss_acc += fabsf(logf(py));
                    corr_acc += ((idx == 0xFFFFFFFFu ? 0 : (int32_t)idx) == y[q]) ? 1.f : 0.f;
                }
            }
        }
    }
    xent_fold<Split>(loss_acc, corr_acc, loss_x, corr_x, s_sums, partials);
}

// m <= 64 (the logits layer: 41 classes, 48 at P = 8): one row per 16-LANE GROUP, KE = ceil(m / 16) logits per lane, so a
// wave works on four rows at once and every reduction is four DPP rotations inside the 16-lane row (row16_reduce: all 16
// lanes end with the same bits), no v_readlane, no cross-row step.  The wave-per-row form above keeps 41 of 64 lanes busy
// and spends a full wave reduction per row: 105 us for the [233 k x 41] logits (0.7 TB/s); this one issues a quarter of the
// instructions per row.
template <int KE, int R, bool Split>
__global__ __launch_bounds__(256) void softmax_xent_rows16_kernel(const float *src, float *dst,
                                                                  const int32_t *__restrict__ Y, size_t n_rows,
                                                                  uint32_t m, float grad_scale, float *__restrict__ partials,
                                                                  const int32_t *__restrict__ S, int32_t train_set) {
    __shared__ float s_sums[2 * xent_slots(Split)][4];    // [slot][loss, correct][wave]
    const int lane = threadIdx.x & 63;
    const uint32_t sub = lane & 15;
    const size_t gstride = ((size_t)gridDim.x * blockDim.x) >> 4;           // 16-lane groups in the grid
    const size_t g0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const size_t w0 = g0 & ~(size_t)3;                                       // first group of this wave
    float loss_acc = 0.f, corr_acc = 0.f;
    float loss_x[3] = {0.f, 0.f, 0.f}, corr_x[3] = {0.f, 0.f, 0.f};      // slots 1..3, Split only
    for (size_t base = 0; w0 + base < n_rows; base += gstride * R) {         // wave-uniform trip count
        float x[R][KE];
        int32_t y[R], s[Split ? R : 1];
#pragma unroll
        for (int q = 0; q < R; q++) {                                        // all loads first
            const size_t r = g0 + base + (size_t)q * gstride;
            const bool live = r < n_rows;
            y[q] = live ? Y[r] : 0;
            if constexpr (Split) s[q] = live ? S[r] : 0;
#pragma unroll
            for (int k = 0; k < KE; k++) {
                const uint32_t c = sub + 16u * k;
                x[q][k] = (live && c < m) ? src[r * m + c] : -INFINITY;
            }
        }
#pragma unroll
        for (int q = 0; q < R; q++) {
            const size_t r = g0 + base + (size_t)q * gstride;
            const bool live = r < n_rows;
            float mx = x[q][0];
#pragma unroll
            for (int k = 1; k < KE; k++) mx = fmaxf(mx, x[q][k]);
            mx = row16_reduce(mx, [](float a, float b) { return fmaxf(a, b); });
            // FIRST column holding the maximum (strict `<` of the reference, cuda_utils.cu:126); none (all -inf / NaN) -> 0
            uint32_t idx = 0xFFFFFFFFu;
#pragma unroll
            for (int k = KE - 1; k >= 0; k--)
                if (x[q][k] == mx && sub + 16u * k < m) idx = sub + 16u * k;
            idx = row16_reduce(idx, [](uint32_t a, uint32_t b) { return a < b ? a : b; });
            float sum = 0.f;
#pragma unroll
            for (int k = 0; k < KE; k++) {
                x[q][k] = sub + 16u * k < m ? expf(x[q][k] - mx) : 0.f;
                sum += x[q][k];
            }
            sum = row16_reduce(sum, [](float a, float b) { return a + b; });
            float py = 0.f;                                                  // p_y: exactly one lane / slot holds column y
#pragma unroll
            for (int k = 0; k < KE; k++) {
                const uint32_t c = sub + 16u * k;
                const float o = x[q][k] / sum;
                const bool hit = (int32_t)c == y[q];
                const float g = (hit ? o - 1.f : o) * grad_scale;
                if constexpr (Split) { if (live && c < m) dst[r * m + c] = s[q] == train_set ? g : 0.f; }
                else { if (live && c < m) dst[r * m + c] = g; }
                if (hit && c < m) py = o;
            }
            py = row16_reduce(py, [](float a, float b) { return a + b; });   // the others are exact zeros
            if (live && sub == 0) {
                if constexpr (Split) {
                    xent_add_by_slot(s[q], fabsf(logf(py)), ((idx == 0xFFFFFFFFu ? 0 : (int32_t)idx) == y[q]) ? 1.f : 0.f,
                                     loss_acc, corr_acc, loss_x, corr_x);
                } else {
                    loss_acc += fabsf(logf(py));
                    corr_acc += ((idx == 0xFFFFFFFFu ? 0 : (int32_t)idx) == y[q]) ? 1.f : 0.f;
                }
            }
        }
    }
    loss_acc = wave_sum_dpp(loss_acc);
    corr_acc = wave_sum_dpp(corr_acc);
    if constexpr (Split) {
#pragma unroll
        for (int j = 0; j < 3; j++) { loss_x[j] = wave_sum_dpp(loss_x[j]); corr_x[j] = wave_sum_dpp(corr_x[j]); }
    }
    xent_fold<Split>(loss_acc, corr_acc, loss_x, corr_x, s_sums, partials);
}

// ---- the unfused chain's split steps ------------------------------------------
// mat[i, :] = +0.0 where S[i] != set
__global__ __launch_bounds__(256) void select_rows_by_set_kernel(float *__restrict__ mat, const int32_t *__restrict__ S,
                                                                 int32_t set, size_t size, size_t m) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < size; i += stride)
        if (S[i / m] != set) mat[i] = 0.f;
}

// partial[4 b + k] = this workgroup's sum of |x[i]| over slot(S[i]) == k
__global__ __launch_bounds__(256) void abssum_by_set_partial_kernel(const float *__restrict__ x,
                                                                    const int32_t *__restrict__ S, size_t n,
                                                                    float *__restrict__ partial) {
    __shared__ float wsum[4][4];
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float a = fabsf(x[i]);
        const uint32_t slot = xent_slot(S[i]);
#pragma unroll
        for (int k = 0; k < 4; k++) acc[k] += slot == (uint32_t)k ? a : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) acc[k] = wave_sum(acc[k]);
    block_fold(acc, wsum, partial + 4 * (size_t)blockIdx.x);
}

// ---- fused Adam -------------------------------------------------------------
__global__ __launch_bounds__(256) void adam_fused_kernel(float *__restrict__ p, float *__restrict__ g,
                                                         float *__restrict__ m, float *__restrict__ v,
                                                         float step, float b1, float b2, float wd, float c2,
                                                         float eps, size_t size) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < size; i += stride) {
        const float pi = p[i];
        const float gi = fmaf(wd, pi, g[i]);                 // axpy(W, G_W, wd)     gcn.hpp:163
        const float mi = (1.f - b1) * gi + b1 * m[i];        // axpby                gcn.hpp:164
        const float vi = (1.f - b2) * gi * gi + b2 * v[i];   // aaxpby               gcn.hpp:166
        g[i] = gi; m[i] = mi; v[i] = vi;
        p[i] = pi - step * mi / (sqrtf(vi / c2) + eps);      // adam_final           gcn.hpp:168
    }
}

// one launch for EVERY parameter tensor of the model: block b works on 1024 elements of the tensor whose
// [first_block, first_block + blocks) range holds b (a model has ~8 tensors: linear search)
__device__ __forceinline__ void adam_one(float *p, float *g, float *m, float *v, size_t i, float step, float b1,
                                         float b2, float wd, float c2, float eps) {
    const float pi = p[i];
    const float gi = fmaf(wd, pi, g[i]);
    const float mi = (1.f - b1) * gi + b1 * m[i];
    const float vi = (1.f - b2) * gi * gi + b2 * v[i];
    g[i] = gi; m[i] = mi; v[i] = vi;
    p[i] = pi - step * mi / (sqrtf(vi / c2) + eps);
}

__global__ __launch_bounds__(256) void adam_multi_kernel(const mggcn_adam_tensor *__restrict__ table, uint32_t n_tensors,
                                                         float step, float b1, float b2, float c2, float eps) {
    uint32_t t = 0;
    while (t + 1 < n_tensors && table[t + 1].first_block <= blockIdx.x) t++;
    const mggcn_adam_tensor T = table[t];
    const size_t base = (size_t)(blockIdx.x - T.first_block) * 1024;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const size_t i = base + (size_t)k * 256 + threadIdx.x;
        if (i < T.size) adam_one(T.param, T.grad, T.m, T.v, i, step, b1, b2, T.weight_decay, c2, eps);
    }
}

// ---- dropout: the mask is never stored --------------------------------------
// Philox4x32-10 (Salmon et al., SC'11) on counter (c >> 2, row low, row high, stream) and key (seed low, seed high): word
// c & 3 of the output decides column c of global row `row`.  A pure function of (seed, stream, row, column): the backward
// pass calls the same kernel on the gradient and gets the same mask, a row shard gets the rows of the whole matrix's mask.
// The generator itself lives in philox.h, shared with the attention dropout of gat.hip.
__device__ __forceinline__ float dropout_one(float x, uint32_t word, uint32_t threshold, float scale) {
    return word >= threshold ? x * scale : 0.f;       // a select: +0.0 also where x is NaN or an infinity
}

// Both kernels walk (row, column group) without a division in the loop: a grid step is step_rows rows and step_cols
// units (both from the host: the grid's thread count over the units per row), with one carry.  The first unit of a
// thread is below 2^19 (stream_grid), so its division is a 32-bit one; a row of 2^32 units or more (q clamped) holds it
// whole.
struct dropout_walk {
    uint64_t row;        // local row
    uint64_t col;        // unit inside the row
    __device__ dropout_walk(size_t q) {
        const uint32_t i0 = blockIdx.x * blockDim.x + threadIdx.x;
        const uint32_t q32 = q > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)q;
        row = i0 / q32;
        col = i0 % q32;
    }
    __device__ void step(size_t q, uint64_t step_rows, uint64_t step_cols) {
        row += step_rows;
        col += step_cols;
        if (col >= q) { col -= q; row++; }
    }
};

// four columns per lane: one generator call serves the lane's float4 (q4 = m / 4 column groups per row)
__global__ __launch_bounds__(256) void dropout_vec4_kernel(const float4 *in, float4 *out, size_t size4, size_t q4,
                                                           uint64_t step_rows, uint64_t step_cols, uint64_t row0,
                                                           uint32_t threshold, float scale, uint32_t k0, uint32_t k1,
                                                           uint32_t dstream) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    dropout_walk at(q4);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < size4; i += stride) {
        float4 x = in[i];
        const uint64_t row = row0 + at.row;
        const philox4 r = philox4x32_10((uint32_t)at.col, (uint32_t)row, (uint32_t)(row >> 32), dstream, k0, k1);
        x.x = dropout_one(x.x, r.w[0], threshold, scale);
        x.y = dropout_one(x.y, r.w[1], threshold, scale);
        x.z = dropout_one(x.z, r.w[2], threshold, scale);
        x.w = dropout_one(x.w, r.w[3], threshold, scale);
        out[i] = x;
        at.step(q4, step_rows, step_cols);
    }
}

// any width, any alignment: a lane computes its column group's call and keeps word c & 3
__global__ __launch_bounds__(256) void dropout_kernel(const float *in, float *out, size_t size, size_t m, uint64_t step_rows,
                                                      uint64_t step_cols, uint64_t row0, uint32_t threshold, float scale,
                                                      uint32_t k0, uint32_t k1, uint32_t dstream) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    dropout_walk at(m);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < size; i += stride) {
        const uint64_t row = row0 + at.row;
        const philox4 r = philox4x32_10((uint32_t)(at.col >> 2), (uint32_t)row, (uint32_t)(row >> 32), dstream, k0, k1);
        const uint32_t lane = (uint32_t)at.col & 3u;
        const uint32_t word = lane == 0 ? r.w[0] : lane == 1 ? r.w[1] : lane == 2 ? r.w[2] : r.w[3];
        out[i] = dropout_one(in[i], word, threshold, scale);
        at.step(m, step_rows, step_cols);
    }
}

// ---- fused sigmoid + binary cross-entropy + gradient + micro-F1 counts -------
// The multi-label loss (mggcn_sigmoid_bce_from_f32): every element is a task of its own, so the pass has no row-wise
// reduction and no width limit.  One exp and one log1p serve the loss and the gradient: with e = exp(-|z|),
// softplus(+-z) = max(+-z, 0) + log1p(e) and sigmoid(z) = z >= 0 ? 1 / (1 + e) : e / (1 + e)  (exp(z) = e for z < 0).
struct bce_term { float loss, g, tp, fp, fn; };

__device__ __forceinline__ bce_term bce_one(float z, int32_t t, bool trains, float grad_scale) {
    const bool pos = t != 0;
    const float e = expf(-fabsf(z));
    const float zt = pos ? -z : z;                                      // t ? softplus(-z) : softplus(z): never inf - inf
    const float p = z >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
    const bool pred = z > 0.f;                                          // +-0 and NaN predict negative
    bce_term r;
    r.loss = fmaxf(zt, 0.f) + log1pf(e);
    r.g = trains ? (p - (pos ? 1.f : 0.f)) * grad_scale : 0.f;          // a select: +0.0 also where p is NaN
    r.tp = (pred && pos) ? 1.f : 0.f;
    r.fp = (pred && !pos) ? 1.f : 0.f;
    r.fn = (!pred && pos) ? 1.f : 0.f;
    return r;
}

// acc = [slot][loss, tp, fp, fn]; the slots other than the row's add +0.0, which keeps their bits (xent_add_by_slot)
template <bool Split>
__device__ __forceinline__ void bce_add_by_slot(uint32_t slot, float l, float tp, float fp, float fn, float (&acc)[Split ? 16 : 4]) {
    if constexpr (Split) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool mine = slot == (uint32_t)k;
            acc[4 * k + 0] += mine ? l : 0.f;
            acc[4 * k + 1] += mine ? tp : 0.f;
            acc[4 * k + 2] += mine ? fp : 0.f;
            acc[4 * k + 3] += mine ? fn : 0.f;
        }
    } else {
        acc[0] += l; acc[1] += tp; acc[2] += fp; acc[3] += fn;
    }
}

// V = 4: a unit is a float4 / int4 of one row (m % 4 == 0, 16-byte aligned operands); V = 1: a unit is an element.  Units
// are walked grid-stride with the row carried along (dropout_walk: no division in the loop).  Every thread reads a unit
// whole before it writes it, and no other thread touches it: dst may be src.  A thread's counts are small integers and a
// workgroup's are sums of those: exact in fp32 below 2^24.  Split = false is the S == NULL form: every row trains and
// lands in slot 0, with the additions of slot 0 of the split form in the same order.
template <int V, bool Split>
__global__ __launch_bounds__(256) void sigmoid_bce_kernel(const float *src, float *dst, const int32_t *__restrict__ T,
                                                          const int32_t *__restrict__ S, size_t units, size_t q,
                                                          uint64_t step_rows, uint64_t step_cols, int32_t train_set,
                                                          float grad_scale, float *__restrict__ partials) {
    constexpr int NA = Split ? 16 : 4;
    __shared__ float w[16][4];                                          // [value][wave]
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    float acc[NA], v[16];
#pragma unroll
    for (int j = 0; j < NA; j++) acc[j] = 0.f;
    dropout_walk at(q);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < units; i += stride) {
        int32_t s = 0;
        if constexpr (Split) s = S[at.row];
        const bool trains = !Split || s == train_set;
        const uint32_t slot = Split ? xent_slot(s) : 0u;
        if constexpr (V == 4) {
            const float4 z = reinterpret_cast<const float4 *>(src)[i];
            const int4 t = reinterpret_cast<const int4 *>(T)[i];
            const bce_term a = bce_one(z.x, t.x, trains, grad_scale), b = bce_one(z.y, t.y, trains, grad_scale),
                           c = bce_one(z.z, t.z, trains, grad_scale), d = bce_one(z.w, t.w, trains, grad_scale);
            reinterpret_cast<float4 *>(dst)[i] = make_float4(a.g, b.g, c.g, d.g);
            bce_add_by_slot<Split>(slot, (a.loss + b.loss) + (c.loss + d.loss), (a.tp + b.tp) + (c.tp + d.tp),
                                   (a.fp + b.fp) + (c.fp + d.fp), (a.fn + b.fn) + (c.fn + d.fn), acc);
        } else {
            const bce_term a = bce_one(src[i], T[i], trains, grad_scale);
            dst[i] = a.g;
            bce_add_by_slot<Split>(slot, a.loss, a.tp, a.fp, a.fn, acc);
        }
        at.step(q, step_rows, step_cols);
    }
#pragma unroll
    for (int j = 0; j < 16; j++) v[j] = j < NA ? wave_sum(acc[j]) : 0.f;    // the plain form's slots 1..3: +0.0
    block_fold(v, w, partials + 16 * (size_t)blockIdx.x);               // sixteen values per workgroup, summed by sums_final_kernel<16>
}

// ---- layer normalisation: one row per group of L lanes (the layout, the walk and the dispatch: row_group.h) ----
// y = act(xhat * gamma + beta), xhat = (x - mean) * rstd, rstd = 1 / sqrt(var + eps): mean and the biased variance in two
// passes over the registers (sum of (x - mean)^2, not E[x^2] - mean^2, which cancels for rows far from zero).
template <int V, int L, int K, int R>
__global__ __launch_bounds__(256) void layer_norm_forward_kernel(const float *x, float *y, float *xhat,
                                                                 float *__restrict__ rstd_out,
                                                                 const float *__restrict__ gamma,
                                                                 const float *__restrict__ beta, size_t n_rows, uint32_t m,
                                                                 float eps, float slope, int leaky) {
    constexpr int NV = K * V;
    const ln_walk<L> at;
    const float fm = (float)m;
    float ga[NV], be[NV];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const uint32_t c0 = (at.sub + (uint32_t)L * k) * V;
        ln_load<V>(&ga[k * V], gamma + c0, c0 < m, 0.f);
        ln_load<V>(&be[k * V], beta + c0, c0 < m, 0.f);
    }
    for (size_t base = 0; at.w0 + base < n_rows; base += at.gstride * R) {
        float a[R][NV];
#pragma unroll
        for (int q = 0; q < R; q++) {                                            // all loads first
            const size_t r = at.g0 + base + (size_t)q * at.gstride;
            const bool live = r < n_rows;
#pragma unroll
            for (int k = 0; k < K; k++) {
                const uint32_t c0 = (at.sub + (uint32_t)L * k) * V;
                ln_load<V>(&a[q][k * V], x + r * m + c0, live && c0 < m, 0.f);
            }
        }
#pragma unroll
        for (int q = 0; q < R; q++) {
            const size_t r = at.g0 + base + (size_t)q * at.gstride;
            const bool live = r < n_rows;
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < NV; i++) s += a[q][i];                           // columns past m hold +0.0
            const float mean = ln_group_sum<L>(s) / fm;
            float d2 = 0.f;
#pragma unroll
            for (int i = 0; i < NV; i++) {
                const uint32_t c = (at.sub + (uint32_t)L * (i / V)) * V + (i % V);
                const float d = c < m ? a[q][i] - mean : 0.f;
                a[q][i] = d;
                d2 = fmaf(d, d, d2);
            }
            const float rs = 1.f / sqrtf(ln_group_sum<L>(d2) / fm + eps);
#pragma unroll
            for (int k = 0; k < K; k++) {
                const uint32_t c0 = (at.sub + (uint32_t)L * k) * V;
                float xh[V], o[V];
#pragma unroll
                for (int v = 0; v < V; v++) {
                    xh[v] = a[q][k * V + v] * rs;
                    const float z = fmaf(xh[v], ga[k * V + v], be[k * V + v]);
                    o[v] = leaky ? lrelu(z, slope) : z;
                }
                if (live && c0 < m) {
                    ln_store<V>(xhat + r * m + c0, xh);
                    ln_store<V>(y + r * m + c0, o);
                }
            }
            if (live && at.sub == 0) rstd_out[r] = rs;
        }
    }
}

// dz = G . leaky_relu'(act) (or G), g = dz . gamma, G_in = rstd (g - mean(g) - xhat mean(g . xhat)); the column sums
// G_gamma = sum_r dz . xhat and G_beta = sum_r dz without a float atomic: a lane owns its columns for the whole grid-stride
// loop and sums its rows in registers, the workgroup's 256 / L groups meet in LDS and are added in group order, and one
// [2 x m] partial per workgroup goes to the scratch, which colsum_final_kernel (reduce.h) adds in workgroup order.
template <int V, int L, int K, int R>
__global__ __launch_bounds__(256) void layer_norm_backward_kernel(const float *G, const float *act, const float *xhat,
                                                                  const float *__restrict__ rstd,
                                                                  const float *__restrict__ gamma, float *G_in,
                                                                  float *__restrict__ partials, size_t n_rows, uint32_t m,
                                                                  float slope, int leaky) {
    constexpr int NV = K * V, NG = 256 / L, CP = L * NV;                         // CP: columns a group covers
    __shared__ float s_part[2 * NG * CP];                                        // [gamma | beta][group][column]
    const ln_walk<L> at;
    const float fm = (float)m;
    float ga[NV], dg[NV], db[NV];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const uint32_t c0 = (at.sub + (uint32_t)L * k) * V;
        ln_load<V>(&ga[k * V], gamma + c0, c0 < m, 0.f);
    }
#pragma unroll
    for (int i = 0; i < NV; i++) dg[i] = db[i] = 0.f;
    for (size_t base = 0; at.w0 + base < n_rows; base += at.gstride * R) {
        float g[R][NV], a[R][NV], xh[R][NV], rs[R];
#pragma unroll
        for (int q = 0; q < R; q++) {                                            // all loads first
            const size_t r = at.g0 + base + (size_t)q * at.gstride;
            const bool live = r < n_rows;
            rs[q] = live ? rstd[r] : 0.f;
#pragma unroll
            for (int k = 0; k < K; k++) {
                const uint32_t c0 = (at.sub + (uint32_t)L * k) * V;
                const bool ok = live && c0 < m;
                ln_load<V>(&g[q][k * V], G + r * m + c0, ok, 0.f);
                ln_load<V>(&xh[q][k * V], xhat + r * m + c0, ok, 0.f);
                if (leaky) {                                                     // uniform
                    ln_load<V>(&a[q][k * V], act + r * m + c0, ok, 1.f);
                } else {
#pragma unroll
                    for (int v = 0; v < V; v++) a[q][k * V + v] = 1.f;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < R; q++) {
            const size_t r = at.g0 + base + (size_t)q * at.gstride;
            const bool live = r < n_rows;
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int i = 0; i < NV; i++) {                                       // a dead row or column adds +0.0
                const float dz = a[q][i] > 0.f ? g[q][i] : slope * g[q][i];
                db[i] += dz;
                dg[i] = fmaf(dz, xh[q][i], dg[i]);
                const float gg = dz * ga[i];
                g[q][i] = gg;
                s1 += gg;
                s2 = fmaf(gg, xh[q][i], s2);
            }
            const float c1 = ln_group_sum<L>(s1) / fm, c2 = ln_group_sum<L>(s2) / fm;
#pragma unroll
            for (int k = 0; k < K; k++) {
                const uint32_t c0 = (at.sub + (uint32_t)L * k) * V;
                float o[V];
#pragma unroll
                for (int v = 0; v < V; v++) o[v] = rs[q] * fmaf(-xh[q][k * V + v], c2, g[q][k * V + v] - c1);
                if (live && c0 < m) ln_store<V>(G_in + r * m + c0, o);
            }
        }
    }
    const uint32_t grp = threadIdx.x / L;
#pragma unroll
    for (int i = 0; i < NV; i++) {
        const uint32_t c = (at.sub + (uint32_t)L * (i / V)) * V + (i % V);
        s_part[(0 * NG + grp) * CP + c] = dg[i];
        s_part[(1 * NG + grp) * CP + c] = db[i];
    }
    __syncthreads();
    for (uint32_t idx = threadIdx.x; idx < 2u * CP; idx += 256) {
        const uint32_t j = idx / CP, c = idx % CP;
        float s = s_part[(j * NG + 0) * CP + c];
#pragma unroll
        for (int w = 1; w < NG; w++) s += s_part[(j * NG + w) * CP + c];
        if (c < m) partials[((size_t)blockIdx.x * 2 + j) * m + c] = s;
    }
}

}  // namespace

// ============================ C ABI =========================================
MGGCN_API void mggcn_leaky_relu_forward_f32(mggcn_stream_t stream, const float *in, float *out,
                                            size_t size, float alpha) {
    launch_map1(as_stream(stream), in, out, size, LreluFwd{alpha});
}

MGGCN_API void mggcn_leaky_relu_backward_f32(mggcn_stream_t stream, const float *in, const float *G_in,
                                             float *G_out, size_t size, float alpha) {
    launch_map2(as_stream(stream), in, G_in, G_out, size, LreluBwd{alpha});
}

MGGCN_API void mggcn_broadcast_rows_f32(mggcn_stream_t stream, const float *row, float *mat, size_t size,
                                        size_t m, int discard) {
    if (!size) return;
    MGGCN_REQUIRE(m > 0, "row width must be positive");
    hipLaunchKernelGGL(broadcast_rows_kernel, dim3(stream_grid(size)), dim3(256), 0, as_stream(stream), row,
                       mat, size, m, discard);
    MGGCN_CHECK_LAUNCH();
}

MGGCN_API void mggcn_scale_rows_f32(mggcn_stream_t stream, float *mat, const float *scalar, size_t size,
                                    size_t m) {
    if (!size) return;
    MGGCN_REQUIRE(m > 0, "row width must be positive");
    hipLaunchKernelGGL(scale_rows_kernel, dim3(stream_grid(size)), dim3(256), 0, as_stream(stream), mat,
                       scalar, size, m);
    MGGCN_CHECK_LAUNCH();
}

MGGCN_API void mggcn_max_rows_f32(mggcn_stream_t stream, const float *mat, float *maxs, size_t size,
                                  size_t m) {
    if (!size) return;
    MGGCN_REQUIRE(m > 0 && size % m == 0, "size must be n_rows * m");
    const size_t n_rows = size / m;
    hipLaunchKernelGGL(max_rows_kernel, dim3(stream_grid(n_rows * 64)), dim3(256), 0, as_stream(stream), mat,
                       maxs, n_rows, m);
    MGGCN_CHECK_LAUNCH();
}

MGGCN_API void mggcn_max_row_indices_f32(mggcn_stream_t stream, const float *mat, int32_t *maxs,
                                         size_t size, size_t m) {
    if (!size) return;
    MGGCN_REQUIRE(m > 0 && size % m == 0, "size must be n_rows * m");
    const size_t n_rows = size / m;
    hipLaunchKernelGGL(max_row_indices_kernel, dim3(stream_grid(n_rows * 64)), dim3(256), 0,
                       as_stream(stream), mat, maxs, n_rows, m);
    MGGCN_CHECK_LAUNCH();
}

MGGCN_API void mggcn_index_log_rows_f32(mggcn_stream_t stream, const float *mat, const int32_t *indices,
                                        float *values, size_t size, size_t m) {
    if (!size) return;
    MGGCN_REQUIRE(m > 0 && size % m == 0, "size must be n_rows * m");
    const size_t n_rows = size / m;
    hipLaunchKernelGGL(index_log_rows_kernel, dim3(stream_grid(n_rows)), dim3(256), 0, as_stream(stream),
                       mat, indices, values, n_rows, m);
    MGGCN_CHECK_LAUNCH();
}

namespace {
// Halo pack: dst[k, :] = src[idx[k], :].  One wave64 per gathered row, float4 lanes where the
// pitches allow; a pure HBM stream (the rows a peer rank needs of this rank's shard).
__global__ __launch_bounds__(256) void gather_rows_kernel(const float *__restrict__ src, size_t ld_src,
                                                          const uint32_t *__restrict__ idx, size_t n_idx, uint32_t d,
                                                          float *__restrict__ dst, size_t ld_dst, bool vec) {
    const int lane = threadIdx.x & 63;
    const size_t waves = (size_t)gridDim.x * (blockDim.x >> 6);
    for (size_t k = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); k < n_idx; k += waves) {
        const float *s = src + (size_t)idx[k] * ld_src;
        float *o = dst + k * ld_dst;
        if (vec) {
            for (uint32_t c = lane * 4; c < d; c += 256)
                *reinterpret_cast<float4 *>(o + c) = *reinterpret_cast<const float4 *>(s + c);
        } else {
            for (uint32_t c = lane; c < d; c += 64) o[c] = s[c];
        }
    }
}
}  // namespace

MGGCN_API void mggcn_gather_rows_f32(mggcn_stream_t stream, const float *src, size_t ld_src, const uint32_t *indices,
                                     size_t n_indices, uint32_t d, float *dst, size_t ld_dst) {
    if (!n_indices || !d) return;
    MGGCN_REQUIRE(src && indices && dst && ld_src >= d && ld_dst >= d, "gather_rows: bad operand");
    const bool vec = d % 4 == 0 && ld_src % 4 == 0 && ld_dst % 4 == 0 && aligned16(src) && aligned16(dst);
    const size_t blocks = std::min<size_t>((n_indices + 3) / 4, (size_t)kNumCU * 16);
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), src, ld_src, indices,
                       n_indices, d, dst, ld_dst, vec);
    MGGCN_CHECK_LAUNCH();
}

MGGCN_API void mggcn_add_indexed_rows_f32(mggcn_stream_t stream, float *mat, const int32_t *indices,
                                          float alpha, size_t size, size_t m) {
    if (!size) return;
    MGGCN_REQUIRE(m > 0 && size % m == 0, "size must be n_rows * m");
    const size_t n_rows = size / m;
    hipLaunchKernelGGL(add_indexed_rows_kernel, dim3(stream_grid(n_rows)), dim3(256), 0, as_stream(stream),
                       mat, indices, alpha, n_rows, m);
    MGGCN_CHECK_LAUNCH();
}

MGGCN_API void mggcn_is_equal_i32(mggcn_stream_t stream, const int32_t *a, const int32_t *b, float *out,
                                  size_t size) {
    if (!size) return;
    hipLaunchKernelGGL(is_equal_kernel, dim3(stream_grid(size)), dim3(256), 0, as_stream(stream), a, b, out,
                       size);
    MGGCN_CHECK_LAUNCH();
}

MGGCN_API void mggcn_subtract_rows_exp_f32(mggcn_stream_t stream, const float *mat, const float *scalar,
                                           float *out, size_t size, size_t m) {
    if (!size) return;
    MGGCN_REQUIRE(m > 0, "row width must be positive");
    hipLaunchKernelGGL(subtract_rows_exp_kernel, dim3(stream_grid(size)), dim3(256), 0, as_stream(stream),
                       mat, scalar, out, size, m);
    MGGCN_CHECK_LAUNCH();
}

MGGCN_API void mggcn_axpby_f32(mggcn_stream_t stream, const float *A, float *B, float alpha, float beta,
                               size_t size) {
    launch_map2(as_stream(stream), A, B, B, size, Axpby{alpha, beta});
}

MGGCN_API void mggcn_aaxpby_f32(mggcn_stream_t stream, const float *A, float *B, float alpha, float beta,
                                size_t size) {
    launch_map2(as_stream(stream), A, B, B, size, Aaxpby{alpha, beta});
}

MGGCN_API void mggcn_adam_final_f32(mggcn_stream_t stream, float *param, const float *m, const float *v,
                                    float lr, float c1, float c2, float eps, size_t size) {
    if (!size) return;
    hipLaunchKernelGGL(adam_final_kernel, dim3(stream_grid(size)), dim3(256), 0, as_stream(stream), param, m,
                       v, lr / c1, c2, eps, size);
    MGGCN_CHECK_LAUNCH();
}

MGGCN_API void mggcn_axpy_f32(mggcn_stream_t stream, const float *A, float *B, float alpha, size_t size) {
    launch_map2(as_stream(stream), A, B, B, size, Axpy{alpha});
}

MGGCN_API void mggcn_scale_mat_f32(mggcn_stream_t stream, float *mat, float scalar, size_t size) {
    launch_map1(as_stream(stream), mat, mat, size, Scal{scalar});
}

MGGCN_API void mggcn_dropout_f32(mggcn_stream_t stream, const float *in, float *out, size_t size, size_t m, uint64_t row0,
                                 uint32_t threshold, float scale, uint64_t seed, uint32_t dropout_stream) {
    if (!size) return;
    MGGCN_REQUIRE(m > 0 && size % m == 0, "size must be n_rows * m");
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    if (m % 4 == 0 && aligned16(in) && aligned16(out)) {
        const size_t size4 = size / 4, q4 = m / 4;
        const unsigned grid = stream_grid(size4);
        const size_t threads = (size_t)grid * 256;
        hipLaunchKernelGGL(dropout_vec4_kernel, dim3(grid), dim3(256), 0, as_stream(stream),
                           reinterpret_cast<const float4 *>(in), reinterpret_cast<float4 *>(out), size4, q4,
                           (uint64_t)(threads / q4), (uint64_t)(threads % q4), row0, threshold, scale, k0, k1, dropout_stream);
    } else {
        const unsigned grid = stream_grid(size);
        const size_t threads = (size_t)grid * 256;
        hipLaunchKernelGGL(dropout_kernel, dim3(grid), dim3(256), 0, as_stream(stream), in, out, size, m,
                           (uint64_t)(threads / m), (uint64_t)(threads % m), row0, threshold, scale, k0, k1, dropout_stream);
    }
    MGGCN_CHECK_LAUNCH();
}

MGGCN_API void mggcn_layer_norm_forward_f32(mggcn_stream_t stream, const float *x, float *y, float *xhat, float *rstd,
                                            const float *gamma, const float *beta, size_t n_rows, size_t m, float eps,
                                            uint32_t flags) {
    MGGCN_REQUIRE(m > 0 && m <= MGGCN_LN_MAX_WIDTH, "layer norm supports 1 <= m <= 1024 columns");
    MGGCN_REQUIRE(xhat != nullptr && rstd != nullptr && gamma != nullptr && beta != nullptr, "layer norm: null operand");
    if (!n_rows) return;
    MGGCN_REQUIRE(x != nullptr && y != nullptr, "layer norm: null operand");
    const bool vec = m % 4 == 0 && aligned16(x) && aligned16(y) && aligned16(xhat) && aligned16(gamma) && aligned16(beta);
    const int leaky = (flags & MGGCN_LN_LEAKY_RELU) != 0;
#define MGGCN_LN_FWD(V, L, K, R)                                                                                         \
    hipLaunchKernelGGL((layer_norm_forward_kernel<V, L, K, R>), dim3(layer_norm_grid<L, R>(n_rows)), dim3(256), 0,          \
                       as_stream(stream), x, y, xhat, rstd, gamma, beta, n_rows, (uint32_t)m, eps, 0.01f, leaky)
    MGGCN_LN_DISPATCH(MGGCN_LN_FWD, vec, m);
#undef MGGCN_LN_FWD
    MGGCN_CHECK_LAUNCH();
}

MGGCN_API void mggcn_layer_norm_backward_f32(mggcn_stream_t stream, const float *G, const float *act, const float *xhat,
                                             const float *rstd, const float *gamma, float *G_in, float *G_gamma,
                                             float *G_beta, size_t n_rows, size_t m, uint32_t flags) {
    MGGCN_REQUIRE(m > 0 && m <= MGGCN_LN_MAX_WIDTH, "layer norm supports 1 <= m <= 1024 columns");
    MGGCN_REQUIRE(xhat != nullptr && rstd != nullptr && gamma != nullptr, "layer norm backward: null operand");
    MGGCN_REQUIRE(G_gamma != nullptr && G_beta != nullptr, "layer norm backward: null gradient");
    const int leaky = (flags & MGGCN_LN_LEAKY_RELU) != 0;
    const hipStream_t st = as_stream(stream);
    const unsigned final_grid = (unsigned)((2 * m + 63) / 64);
    if (!n_rows) {                                                    // the sums over no rows
        hipLaunchKernelGGL(colsum_final_kernel, dim3(final_grid), dim3(256), 0, st, nullptr, 0u, 2 * (uint32_t)m, G_gamma,
                           G_beta, (uint32_t)m);
        MGGCN_CHECK_LAUNCH();
        return;
    }
    MGGCN_REQUIRE(G != nullptr && G_in != nullptr && (!leaky || act != nullptr), "layer norm backward: null operand");
    const bool vec = m % 4 == 0 && aligned16(G) && aligned16(xhat) && aligned16(G_in) && aligned16(gamma) && (!leaky || aligned16(act));
    float *partials = stream_scratch(st, scratch_kind::colsums, (size_t)kLayerNormBlocks * 2 * m);
    unsigned grid = 0;
#define MGGCN_LN_BWD(V, L, K, R)                                                                                         \
    hipLaunchKernelGGL((layer_norm_backward_kernel<V, L, K, R>), dim3(grid = layer_norm_grid<L, R>(n_rows)), dim3(256), 0,  \
                       st, G, act, xhat, rstd, gamma, G_in, partials, n_rows, (uint32_t)m, 0.01f, leaky)
    MGGCN_LN_DISPATCH(MGGCN_LN_BWD, vec, m);
#undef MGGCN_LN_BWD
    MGGCN_CHECK_LAUNCH();
    hipLaunchKernelGGL(colsum_final_kernel, dim3(final_grid), dim3(256), 0, st, partials, grid, 2 * (uint32_t)m, G_gamma,
                       G_beta, (uint32_t)m);
    MGGCN_CHECK_LAUNCH();
}

MGGCN_API void mggcn_abssum_f32(mggcn_stream_t stream, const float *A, size_t size, float *result_device) {
    MGGCN_REQUIRE(result_device != nullptr, "null result pointer");
    float *scratch = sums_scratch<1, kAsumBlocks>(as_stream(stream));
    const unsigned blocks = std::min<unsigned>(kAsumBlocks, stream_grid(size ? size : 1));
    hipLaunchKernelGGL(abssum_partial_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), A, size, scratch);
    MGGCN_CHECK_LAUNCH();
    hipLaunchKernelGGL((sums_final_kernel<1, false>), dim3(1), dim3(256), 0, as_stream(stream), scratch, blocks,
                       result_device);
    MGGCN_CHECK_LAUNCH();
}

namespace {
// Both forms of the fused loss: the same grid, dispatch on KE / K / R and final tree; Split adds S and train_set to the
// kernel and four pairs instead of one to the partials.
template <bool Split>
void launch_xent(hipStream_t st, const float *logits, float *G, const int32_t *Y, const int32_t *S, size_t n_rows, size_t m,
                 int32_t train_set, float grad_scale, float *sums_device) {
    constexpr int NV = 2 * xent_slots(Split);
    const dim3 block(256);
    float *partials = sums_scratch<NV, kXentBlocks>(st);     // stream order keeps its users apart
    const dim3 grid(stream_grid(n_rows * (m <= 64 ? 16 : 64)));
    if (m <= 64) {                               // one row per 16-lane group
#define MGGCN_XENT16(KE)                                                                                          \
    hipLaunchKernelGGL((softmax_xent_rows16_kernel<KE, 4, Split>), grid, block, 0, st, logits, G, Y, n_rows, (uint32_t)m, \
                       grad_scale, partials, S, train_set)
        if (m <= 16) MGGCN_XENT16(1);
        else if (m <= 32) MGGCN_XENT16(2);
        else if (m <= 48) MGGCN_XENT16(3);
        else MGGCN_XENT16(4);
#undef MGGCN_XENT16
    } else {
        // (tried on the wave-per-row form: two workgroups per CU to thin out the two contended scalar atomics at the end
        //  of every workgroup -- 105 -> 145 us: the pass wants the occupancy)
#define MGGCN_XENT(K, R)                                                                                     \
    hipLaunchKernelGGL((softmax_xent_fused_kernel<K, R, Split>), grid, block, 0, st, logits, G, Y, n_rows, m, grad_scale, \
                       partials, S, train_set)
        if (m <= 128) MGGCN_XENT(2, 4);
        else if (m <= 256) MGGCN_XENT(4, 2);
        else if (m <= 512) MGGCN_XENT(8, 1);
        else MGGCN_XENT(16, 1);
#undef MGGCN_XENT
    }
    MGGCN_CHECK_LAUNCH();
    hipLaunchKernelGGL((sums_final_kernel<NV, true>), dim3(1), dim3(256), 0, st, partials, grid.x, sums_device);
    MGGCN_CHECK_LAUNCH();
}
}  // namespace

MGGCN_API void mggcn_softmax_xent_fused_from_f32(mggcn_stream_t stream, const float *logits, float *G, const int32_t *Y,
                                                 size_t n_rows, size_t m, float grad_scale, float *sums_device) {
    if (!n_rows) return;
    MGGCN_REQUIRE(m > 0 && m <= 64u * kXentMaxPerLane, "fused loss supports 1 <= m <= 1024 classes");
    MGGCN_REQUIRE(logits != nullptr && G != nullptr && Y != nullptr && sums_device != nullptr, "fused loss: null operand");
    launch_xent<false>(as_stream(stream), logits, G, Y, nullptr, n_rows, m, 0, grad_scale, sums_device);
}

MGGCN_API void mggcn_softmax_xent_split_from_f32(mggcn_stream_t stream, const float *logits, float *G, const int32_t *Y,
                                                 const int32_t *S, size_t n_rows, size_t m, int32_t train_set,
                                                 float grad_scale, float *sums_device) {
    if (!n_rows) return;
    MGGCN_REQUIRE(m > 0 && m <= 64u * kXentMaxPerLane, "fused loss supports 1 <= m <= 1024 classes");
    MGGCN_REQUIRE(train_set >= 0 && train_set <= 2, "train_set must be 0 (train), 1 (validation) or 2 (test)");
    MGGCN_REQUIRE(logits != nullptr && G != nullptr && Y != nullptr && S != nullptr && sums_device != nullptr,
                  "split-aware fused loss: null operand");
    launch_xent<true>(as_stream(stream), logits, G, Y, S, n_rows, m, train_set, grad_scale, sums_device);
}

namespace {
template <bool Split>
void launch_bce(hipStream_t st, const float *logits, float *G, const int32_t *T, const int32_t *S, size_t n_rows, size_t m,
                int32_t train_set, float grad_scale, float *sums_device) {
    float *partials = sums_scratch<16, kXentBlocks>(st);
    const bool vec = m % 4 == 0 && aligned16(logits) && aligned16(G) && aligned16(T);
    const size_t q = vec ? m / 4 : m, units = n_rows * q;
    const unsigned grid = stream_grid(units);
    const size_t threads = (size_t)grid * 256;
    if (vec)
        hipLaunchKernelGGL((sigmoid_bce_kernel<4, Split>), dim3(grid), dim3(256), 0, st, logits, G, T, S, units, q,
                           (uint64_t)(threads / q), (uint64_t)(threads % q), train_set, grad_scale, partials);
    else
        hipLaunchKernelGGL((sigmoid_bce_kernel<1, Split>), dim3(grid), dim3(256), 0, st, logits, G, T, S, units, q,
                           (uint64_t)(threads / q), (uint64_t)(threads % q), train_set, grad_scale, partials);
    MGGCN_CHECK_LAUNCH();
    hipLaunchKernelGGL((sums_final_kernel<16, true>), dim3(1), dim3(256), 0, st, partials, grid, sums_device);
    MGGCN_CHECK_LAUNCH();
}
}  // namespace

MGGCN_API void mggcn_sigmoid_bce_from_f32(mggcn_stream_t stream, const float *logits, float *G, const int32_t *T,
                                          const int32_t *S, size_t n_rows, size_t m, int32_t train_set, float grad_scale,
                                          float *sums_device) {
    if (!n_rows) return;
    MGGCN_REQUIRE(m >= 1, "sigmoid-BCE loss: the width must be positive");
    MGGCN_REQUIRE(train_set >= 0 && train_set <= 2, "train_set must be 0 (train), 1 (validation) or 2 (test)");
    MGGCN_REQUIRE(logits != nullptr && G != nullptr && T != nullptr && sums_device != nullptr, "sigmoid-BCE loss: null operand");
    if (S) launch_bce<true>(as_stream(stream), logits, G, T, S, n_rows, m, train_set, grad_scale, sums_device);
    else launch_bce<false>(as_stream(stream), logits, G, T, nullptr, n_rows, m, train_set, grad_scale, sums_device);
}

MGGCN_API void mggcn_select_rows_by_set_f32(mggcn_stream_t stream, float *mat, const int32_t *S, int32_t set, size_t size,
                                            size_t m) {
    if (!size) return;
    MGGCN_REQUIRE(m > 0 && size % m == 0, "size must be n_rows * m");
    MGGCN_REQUIRE(mat != nullptr && S != nullptr, "select_rows_by_set: null operand");
    hipLaunchKernelGGL(select_rows_by_set_kernel, dim3(stream_grid(size)), dim3(256), 0, as_stream(stream), mat, S, set,
                       size, m);
    MGGCN_CHECK_LAUNCH();
}

MGGCN_API void mggcn_abssum_by_set_f32(mggcn_stream_t stream, const float *x, const int32_t *S, size_t n,
                                       float *result_device) {
    MGGCN_REQUIRE(result_device != nullptr && (!n || (x != nullptr && S != nullptr)), "abssum_by_set: null operand");
    float *scratch = sums_scratch<4, kAsumBlocks>(as_stream(stream));
    const unsigned blocks = std::min<unsigned>(kAsumBlocks, stream_grid(n ? n : 1));
    hipLaunchKernelGGL(abssum_by_set_partial_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), x, S, n, scratch);
    MGGCN_CHECK_LAUNCH();
    hipLaunchKernelGGL((sums_final_kernel<4, false>), dim3(1), dim3(256), 0, as_stream(stream), scratch, blocks,
                       result_device);
    MGGCN_CHECK_LAUNCH();
}

MGGCN_API void mggcn_softmax_xent_fused_f32(mggcn_stream_t stream, float *H, const int32_t *Y,
                                            size_t n_rows, size_t m, float grad_scale, float *sums_device) {
    mggcn_softmax_xent_fused_from_f32(stream, H, H, Y, n_rows, m, grad_scale, sums_device);
}

MGGCN_API uint32_t mggcn_adam_multi_blocks(uint64_t size) { return (uint32_t)((size + 1023) / 1024); }

MGGCN_API void mggcn_adam_multi_f32(mggcn_stream_t stream, const mggcn_adam_tensor *table_device, uint32_t n_tensors,
                                    uint32_t total_blocks, float lr, float beta1, float beta2, float c1, float c2,
                                    float eps) {
    if (!n_tensors || !total_blocks) return;
    MGGCN_REQUIRE(table_device != nullptr, "mggcn_adam_multi_f32 needs the tensor table");
    hipLaunchKernelGGL(adam_multi_kernel, dim3(total_blocks), dim3(256), 0, as_stream(stream), table_device, n_tensors,
                       lr / c1, beta1, beta2, c2, eps);
    MGGCN_CHECK_LAUNCH();
}

MGGCN_API void mggcn_adam_fused_f32(mggcn_stream_t stream, float *param, float *grad, float *m, float *v,
                                    float lr, float beta1, float beta2, float weight_decay, float c1,
                                    float c2, float eps, size_t size) {
    if (!size) return;
    hipLaunchKernelGGL(adam_fused_kernel, dim3(stream_grid(size)), dim3(256), 0, as_stream(stream), param,
                       grad, m, v, lr / c1, beta1, beta2, weight_decay, c2, eps, size);
    MGGCN_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------
// fp32 -> bf16 for the bf16 aggregation (mggcn_spmm_csr_bf16): round to nearest even, NaN stays NaN, overflow -> inf.
// A plain cast: hipcc emits v_cvt_pk_bf16_f32 for it on gfx950 (integer rounding on the f32 bits would turn some NaNs
// into a zero or an infinity).  Vector form: four columns per thread (16 bytes in, 8 out) when the rows allow it.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t bf16_pair(float lo, float hi) {
    return (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)lo) | ((uint32_t)__builtin_bit_cast(uint16_t, (__bf16)hi) << 16);
}

__global__ __launch_bounds__(256) void convert_f32_bf16_vec4_kernel(const float *__restrict__ src, size_t ld_src,
                                                                    uint16_t *__restrict__ dst, size_t ld_dst,
                                                                    size_t n_rows, size_t q4) {
    const size_t total = n_rows * q4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / q4, c = (i % q4) * 4;
        const float4 v = *reinterpret_cast<const float4 *>(src + r * ld_src + c);
        *reinterpret_cast<uint2 *>(dst + r * ld_dst + c) = make_uint2(bf16_pair(v.x, v.y), bf16_pair(v.z, v.w));
    }
}

__global__ __launch_bounds__(256) void convert_f32_bf16_kernel(const float *__restrict__ src, size_t ld_src,
                                                               uint16_t *__restrict__ dst, size_t ld_dst, size_t n_rows,
                                                               size_t n_cols) {
    const size_t total = n_rows * n_cols;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / n_cols, c = i % n_cols;
        dst[r * ld_dst + c] = __builtin_bit_cast(uint16_t, (__bf16)src[r * ld_src + c]);
    }
}

MGGCN_API void mggcn_convert_f32_bf16(mggcn_stream_t stream, const float *src, size_t ld_src, uint16_t *dst,
                                      size_t ld_dst, size_t n_rows, size_t n_cols) {
    if (!n_rows || !n_cols) return;
    MGGCN_REQUIRE(src && dst, "null operand");
    MGGCN_REQUIRE(ld_src >= n_cols && ld_dst >= n_cols, "leading dimension smaller than the row");
    const bool vec = n_cols % 4 == 0 && ld_src % 4 == 0 && ld_dst % 4 == 0 && aligned16(src) &&
                     (reinterpret_cast<uintptr_t>(dst) & 7u) == 0;
    const size_t work = vec ? n_rows * (n_cols / 4) : n_rows * n_cols;
    const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>((work + 255) / 256, (size_t)kNumCU * 16));
    if (vec)
        hipLaunchKernelGGL(convert_f32_bf16_vec4_kernel, dim3(grid), dim3(256), 0, as_stream(stream), src, ld_src, dst,
                           ld_dst, n_rows, n_cols / 4);
    else
        hipLaunchKernelGGL(convert_f32_bf16_kernel, dim3(grid), dim3(256), 0, as_stream(stream), src, ld_src, dst, ld_dst,
                           n_rows, n_cols);
    MGGCN_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------
// Halo pack of a shard that is already bf16 (the row-partitioned model with agg_dtype = "bf16" rounds its shard once and
// sends that image): dst[k, 0:d] = src[idx[k], 0:d] on 2-byte bit patterns, a pure copy.
// A bf16 row is short -- 256 bytes at d = 128 are 16 lanes of 16 bytes -- so a wave64 carries 64 / L rows, L lanes per
// row (a power of two chosen on the host from the row's length in units of T): lane = sub * L + l copies units l, l + L,
// ... of row (wave * 64 / L + sub).  The L lanes of a row read and write consecutive units, so a row is one contiguous
// segment in both directions, and with ld_dst == d the 64 / L rows of a wave land back to back: a full 1 KiB store per
// instruction at d = 128.  T = uint4 (16 bytes) / uint32_t / uint16_t is picked on the host from d, the leading
// dimensions and the two base addresses.  Up to four units per lane are loaded before the first is stored: loads and
// stores retire through ONE in-order counter (vmcnt), so a load issued behind a store is known complete only once that
// store is -- load, store, load, store would pay a round trip per unit; this way the four loads are in flight together.
// ---------------------------------------------------------------------------------------------------------------------
namespace {
constexpr unsigned kGatherBf16Blocks = kNumCU * 8;      // 8 workgroups of 4 waves per CU: all resident at once

template <typename T>
__global__ __launch_bounds__(256) void gather_rows_u16_kernel(const uint16_t *__restrict__ src, size_t ld_src,
                                                               const uint32_t *__restrict__ idx, size_t n_idx,
                                                               uint32_t units, uint16_t *__restrict__ dst, size_t ld_dst,
                                                               uint32_t lanes_log2) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t L = 1u << lanes_log2, rows_per_wave = 64u >> lanes_log2;
    const uint32_t sub = lane >> lanes_log2, l = lane & (L - 1);
    const size_t wave = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const size_t stride = (size_t)gridDim.x * (blockDim.x >> 6) * rows_per_wave;
    for (size_t k = wave * rows_per_wave + sub; k < n_idx; k += stride) {
        const T *s = reinterpret_cast<const T *>(src + (size_t)idx[k] * ld_src);
        T *o = reinterpret_cast<T *>(dst + k * ld_dst);
        size_t c = l;
        for (; c + 3 * L < units; c += 4 * L) {
            const T v0 = s[c], v1 = s[c + L], v2 = s[c + 2 * L], v3 = s[c + 3 * L];
            o[c] = v0; o[c + L] = v1; o[c + 2 * L] = v2; o[c + 3 * L] = v3;
        }
        for (; c < units; c += L) o[c] = s[c];
    }
}

template <typename T>
void launch_gather_rows_bf16(hipStream_t st, const uint16_t *src, size_t ld_src, const uint32_t *indices, size_t n_indices,
                             uint32_t units, uint16_t *dst, size_t ld_dst) {
    uint32_t lanes_log2 = 0;                                // L = the power of two that covers a row, 64 at the most
    while (lanes_log2 < 6 && (1u << lanes_log2) < units) ++lanes_log2;
    const size_t rows_per_wave = 64u >> lanes_log2;
    const size_t waves = (n_indices + rows_per_wave - 1) / rows_per_wave;
    const unsigned blocks = (unsigned)std::min<size_t>((waves + 3) / 4, kGatherBf16Blocks);
    hipLaunchKernelGGL(gather_rows_u16_kernel<T>, dim3(blocks), dim3(256), 0, st, src, ld_src, indices, n_indices, units,
                       dst, ld_dst, lanes_log2);
    MGGCN_CHECK_LAUNCH();
}
}  // namespace

MGGCN_API void mggcn_gather_rows_bf16(mggcn_stream_t stream, const uint16_t *src, size_t ld_src, const uint32_t *indices,
                                      size_t n_indices, uint32_t d, uint16_t *dst, size_t ld_dst) {
    if (!n_indices || !d) return;
    MGGCN_REQUIRE(src && indices && dst && ld_src >= d && ld_dst >= d, "gather_rows_bf16: bad operand");
    const uintptr_t bases = reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst);
    const size_t pitches = d | ld_src | ld_dst;
    if (pitches % 8 == 0 && bases % 16 == 0)
        launch_gather_rows_bf16<uint4>(as_stream(stream), src, ld_src, indices, n_indices, d / 8, dst, ld_dst);
    else if (pitches % 2 == 0 && bases % 4 == 0)
        launch_gather_rows_bf16<uint32_t>(as_stream(stream), src, ld_src, indices, n_indices, d / 2, dst, ld_dst);
    else
        launch_gather_rows_bf16<uint16_t>(as_stream(stream), src, ld_src, indices, n_indices, d, dst, ld_dst);
}
