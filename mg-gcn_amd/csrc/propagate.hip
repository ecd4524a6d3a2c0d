// propagate.hip -- the row kernels of Correct and Smooth (smoothing.py; Huang et al. 2021, PyG's CorrectAndSmooth): a
// post-processing step over the logits of any trained model, two label-propagation loops whose products are the sweep
// SpMM's (mggcn_spmm_csr_f32, untouched) and whose everything else is here.
//
//   residual   P = softmax(logits) row-wise;  E0 = onehot(y) - P on the training rows, +0.0 elsewhere;  sum |E0|
//   step       out = clamp(fma(alpha, T, beta R), lo, hi), T = A X the product, R the loop's constant term; with
//              MGGCN_CS_FIX_TRAIN a training row is R's
//   correct    Z = fma(s, E, P), s = sigma / sum_c |E[i, c]| (MGGCN_CS_AUTOSCALE; 1 where that is not finite or above 1000) or
//              `scale`; with MGGCN_CS_SET_LABELS a training row is onehot(y): the smoothing loop's G0
//
// residual and correct keep a row in the registers of one lane group, the layout of the fused loss (elementwise.hip) with
// the walk of row_group.h: m <= 64 one row per 16-lane group, lane `sub` holding columns sub + 16 k, every reduction four
// DPP rotations inside the group; up to 1024 columns one wave per row, columns lane + 64 k.  The layout depends on m alone,
// so a row gives the same bits wherever it sits.  sum |E0| goes lane -> wave -> workgroup (block_fold) -> sums_final_kernel:
// no atomics, the same bits on every call.  The step is elementwise over the flat [n_rows x m] operands.
#include "common.h"
#include "reduce.h"
#include "row_group.h"
#include "scratch_internal.h"

namespace {

constexpr unsigned kCsBlocks = kNumCU * 4;              // grid cap of the row kernels: four workgroups of four waves per CU

template <int L>
__device__ __forceinline__ float cs_group_max(float v) {
    if constexpr (L == 16) return row16_reduce(v, [](float a, float b) { return fmaxf(a, b); });
    else return wave_max_dpp(v);
}

// Every lane of a group holds the row's label and set; columns past m hold -inf (the maximum ignores them) and give
// exp = +0.0.  The stores of a row come after all of its loads.
template <int L, int K>
__global__ __launch_bounds__(256) void cs_residual_kernel(const float *__restrict__ logits, const int32_t *__restrict__ Y,
                                                          const int32_t *__restrict__ S, size_t n_rows, uint32_t m,
                                                          int32_t train_set, float *__restrict__ P, float *__restrict__ E0,
                                                          float *__restrict__ partials) {
    __shared__ float s_sum[1][4];
    const ln_walk<L> at;
    float acc = 0.f;                                    // this lane's share of sum |E0|, rows in walk order
    for (size_t base = 0; at.w0 + base < n_rows; base += at.gstride) {      // wave-uniform trip count
        const size_t row = at.g0 + base;
        const bool live = row < n_rows;
        float x[K];
#pragma unroll
        for (int k = 0; k < K; k++) {
            const uint32_t c = at.sub + (uint32_t)L * k;
            x[k] = (live && c < m) ? logits[row * m + c] : -INFINITY;
        }
        const int32_t y = live ? Y[row] : -1;
        const bool train = live && S[row] == train_set;
        float mx = x[0];
#pragma unroll
        for (int k = 1; k < K; k++) mx = fmaxf(mx, x[k]);
        mx = cs_group_max<L>(mx);
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < K; k++) {
            x[k] = at.sub + (uint32_t)L * k < m ? expf(x[k] - mx) : 0.f;
            sum += x[k];
        }
        sum = ln_group_sum<L>(sum);
        float l1 = 0.f;
#pragma unroll
        for (int k = 0; k < K; k++) {
            const uint32_t c = at.sub + (uint32_t)L * k;
            const float p = x[k] / sum;
            const float e = train ? ((int32_t)c == y ? 1.f : 0.f) - p : 0.f;
            if (live && c < m) {
                P[row * m + c] = p;
                E0[row * m + c] = e;
                l1 += fabsf(e);
            }
        }
        acc += l1;
    }
    const float v[1] = {wave_sum_dpp(acc)};
    block_fold(v, s_sum, partials + blockIdx.x);
}

// out may be P: a lane reads exactly the elements it writes, and reads them first.
template <int L, int K>
__global__ __launch_bounds__(256) void cs_correct_kernel(const float *P, const float *__restrict__ E,
                                                         const int32_t *__restrict__ Y, const int32_t *__restrict__ S,
                                                         size_t n_rows, uint32_t m, int32_t train_set,
                                                         const float *__restrict__ sums, float inv_T, float scale, int autoscale,
                                                         int set_labels, float *out) {
    const ln_walk<L> at;
    const float sigma = autoscale ? sums[0] * inv_T : 0.f;
    for (size_t base = 0; at.w0 + base < n_rows; base += at.gstride) {      // wave-uniform trip count
        const size_t row = at.g0 + base;
        const bool live = row < n_rows;
        float p[K], e[K];
#pragma unroll
        for (int k = 0; k < K; k++) {
            const uint32_t c = at.sub + (uint32_t)L * k;
            const bool ok = live && c < m;
            p[k] = ok ? P[row * m + c] : 0.f;
            e[k] = ok ? E[row * m + c] : 0.f;
        }
        const bool hot = set_labels && live && S[row] == train_set;
        const int32_t y = hot ? Y[row] : -1;
        float s = scale;
        if (autoscale) {                                 // uniform
            float l1 = 0.f;
#pragma unroll
            for (int k = 0; k < K; k++) l1 += fabsf(e[k]);
            l1 = ln_group_sum<L>(l1);
            const float q = sigma / l1;                 // 0 / 0 = NaN and x / 0 = inf are "not finite"
            s = (fabsf(q) <= 1000.f) ? q : 1.f;         // false for NaN, inf and anything above 1000 (q is never negative)
        }
#pragma unroll
        for (int k = 0; k < K; k++) {
            const uint32_t c = at.sub + (uint32_t)L * k;
            const float z = hot ? ((int32_t)c == y ? 1.f : 0.f) : fmaf(s, e[k], p[k]);
            if (live && c < m) out[row * m + c] = z;
        }
    }
}

__device__ __forceinline__ float cs_post(float t, float r, float alpha, float beta, float lo, float hi) {
    float v = fmaf(alpha, t, beta * r);
    v = v < lo ? lo : v;
    return v > hi ? hi : v;
}

// out may be T: an element is read before it is written, by the thread that writes it.  V = 4: m % 4 == 0, so a float4
// never straddles two rows.
template <int V, bool Fix>
__global__ __launch_bounds__(256) void cs_step_kernel(const float *T, const float *__restrict__ R, const int32_t *__restrict__ S,
                                                      size_t units, size_t q, float alpha, float beta, float lo, float hi,
                                                      int32_t train_set, float *out) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < units; i += stride) {
        bool keep = false;
        if constexpr (Fix) keep = S[i / q] == train_set;
        if constexpr (V == 4) {
            const float4 t = reinterpret_cast<const float4 *>(T)[i], r = reinterpret_cast<const float4 *>(R)[i];
            reinterpret_cast<float4 *>(out)[i] =
                keep ? r : make_float4(cs_post(t.x, r.x, alpha, beta, lo, hi), cs_post(t.y, r.y, alpha, beta, lo, hi),
                                       cs_post(t.z, r.z, alpha, beta, lo, hi), cs_post(t.w, r.w, alpha, beta, lo, hi));
        } else {
            const float t = T[i], r = R[i];
            out[i] = keep ? r : cs_post(t, r, alpha, beta, lo, hi);
        }
    }
}

template <int L>
unsigned cs_grid(size_t n_rows) {
    const size_t per_block = 256 / L;
    return (unsigned)std::min<size_t>((n_rows + per_block - 1) / per_block, kCsBlocks);
}

// (L, K) from the width; F(L, K) launches
#define MGGCN_CS_DISPATCH(F, m)                  \
    do {                                         \
        if ((m) <= 16) F(16, 1);                 \
        else if ((m) <= 32) F(16, 2);            \
        else if ((m) <= 48) F(16, 3);            \
        else if ((m) <= 64) F(16, 4);            \
        else if ((m) <= 128) F(64, 2);           \
        else if ((m) <= 256) F(64, 4);           \
        else if ((m) <= 512) F(64, 8);           \
        else F(64, 16);                          \
    } while (0)

}  // namespace

// ============================ C ABI =========================================
MGGCN_API void mggcn_cs_residual_f32(mggcn_stream_t stream, const float *logits, const int32_t *Y, const int32_t *S,
                                     size_t n_rows, size_t m, int32_t train_set, float *P, float *E0, float *sums_device) {
    if (!n_rows) return;
    MGGCN_REQUIRE(m >= 1 && m <= MGGCN_CS_MAX_WIDTH, "correct and smooth supports 1 <= m <= 1024 columns");
    MGGCN_REQUIRE(logits != nullptr && Y != nullptr && S != nullptr && P != nullptr && E0 != nullptr && sums_device != nullptr,
                  "cs_residual: null operand");
    const hipStream_t st = as_stream(stream);
    static_assert(kCsBlocks <= kSumsGridMax, "more workgroups than the sums scratch holds partials");
    float *partials = sums_scratch<1, kCsBlocks>(st);
    unsigned grid = 0;
#define MGGCN_CS_RESIDUAL(L, K)                                                                                            \
    hipLaunchKernelGGL((cs_residual_kernel<L, K>), dim3(grid = cs_grid<L>(n_rows)), dim3(256), 0, st, logits, Y, S, n_rows, \
                       (uint32_t)m, train_set, P, E0, partials)
    MGGCN_CS_DISPATCH(MGGCN_CS_RESIDUAL, m);
#undef MGGCN_CS_RESIDUAL
    MGGCN_CHECK_LAUNCH();
    hipLaunchKernelGGL((sums_final_kernel<1, false>), dim3(1), dim3(256), 0, st, partials, grid, sums_device);
    MGGCN_CHECK_LAUNCH();
}

MGGCN_API void mggcn_cs_step_f32(mggcn_stream_t stream, const float *T, const float *R, const int32_t *S, size_t n_rows,
                                 size_t m, float alpha, float beta, float lo, float hi, int32_t train_set, uint32_t flags,
                                 float *out) {
    if (!n_rows) return;
    MGGCN_REQUIRE(m >= 1 && m <= MGGCN_CS_MAX_WIDTH, "correct and smooth supports 1 <= m <= 1024 columns");
    MGGCN_REQUIRE((flags & ~MGGCN_CS_FIX_TRAIN) == 0, "cs_step: unknown flag");
    MGGCN_REQUIRE(T != nullptr && R != nullptr && out != nullptr, "cs_step: null operand");
    const bool fix = (flags & MGGCN_CS_FIX_TRAIN) != 0;
    MGGCN_REQUIRE(!fix || S != nullptr, "cs_step: MGGCN_CS_FIX_TRAIN needs the sets");
    const hipStream_t st = as_stream(stream);
    const bool vec = m % 4 == 0 && aligned16(T) && aligned16(R) && aligned16(out);
    const size_t q = vec ? m / 4 : m, units = n_rows * q;
    const dim3 grid(stream_grid(units)), block(256);
#define MGGCN_CS_STEP(V, FIX)                                                                                          \
    hipLaunchKernelGGL((cs_step_kernel<V, FIX>), grid, block, 0, st, T, R, S, units, q, alpha, beta, lo, hi, train_set, out)
    if (vec) { if (fix) MGGCN_CS_STEP(4, true); else MGGCN_CS_STEP(4, false); }
    else { if (fix) MGGCN_CS_STEP(1, true); else MGGCN_CS_STEP(1, false); }
#undef MGGCN_CS_STEP
    MGGCN_CHECK_LAUNCH();
}

MGGCN_API void mggcn_cs_correct_f32(mggcn_stream_t stream, const float *P, const float *E, const int32_t *Y, const int32_t *S,
                                    size_t n_rows, size_t m, int32_t train_set, const float *sums_device, float inv_T,
                                    float scale, uint32_t flags, float *out) {
    if (!n_rows) return;
    MGGCN_REQUIRE(m >= 1 && m <= MGGCN_CS_MAX_WIDTH, "correct and smooth supports 1 <= m <= 1024 columns");
    MGGCN_REQUIRE((flags & ~(MGGCN_CS_AUTOSCALE | MGGCN_CS_SET_LABELS)) == 0, "cs_correct: unknown flag");
    MGGCN_REQUIRE(P != nullptr && E != nullptr && out != nullptr, "cs_correct: null operand");
    const int autoscale = (flags & MGGCN_CS_AUTOSCALE) != 0, set_labels = (flags & MGGCN_CS_SET_LABELS) != 0;
    MGGCN_REQUIRE(!autoscale || sums_device != nullptr, "cs_correct: MGGCN_CS_AUTOSCALE needs the residual's sum");
    MGGCN_REQUIRE(!set_labels || (Y != nullptr && S != nullptr), "cs_correct: MGGCN_CS_SET_LABELS needs the labels and the sets");
    const hipStream_t st = as_stream(stream);
#define MGGCN_CS_CORRECT(L, K)                                                                                        \
    hipLaunchKernelGGL((cs_correct_kernel<L, K>), dim3(cs_grid<L>(n_rows)), dim3(256), 0, st, P, E, Y, S, n_rows,      \
                       (uint32_t)m, train_set, sums_device, inv_T, scale, autoscale, set_labels, out)
    MGGCN_CS_DISPATCH(MGGCN_CS_CORRECT, m);
#undef MGGCN_CS_CORRECT
    MGGCN_CHECK_LAUNCH();
}
