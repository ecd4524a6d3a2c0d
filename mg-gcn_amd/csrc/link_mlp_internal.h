// link_mlp_internal.h -- what the entries of the MLP decoder of the link head share (link_mlp.hip on the fp32 matrix
// instruction, link_mlp_b16.hip on the bf16 one, link_rank.hip's ranking of both): the C layout of a 32 x 32 accumulator
// tile, the half-wave folds, the bf16 packing helpers, the grid caps that fix the order of the sums, the checks of the host
// entries and the (DB, HB) dispatch.  Internal linkage in each translation unit that includes it.  Not part of the ABI.
#pragma once

#include <type_traits>

#include "gat_internal.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr float kLinkMlpSlope = 0.01f;                  // the leaky ReLU of every gcn layer (elementwise.hip)
constexpr unsigned kLinkMlpWalkGrid = kNumCU * 2;       // workgroups of the walk: two fit a CU's LDS at 128 x 128
constexpr unsigned kLinkMlpPairsGrid = kNumCU;          // workgroups of the pairs kernel = rows of its partials
constexpr int kPad = 8;                                 // elements behind every row of the bf16 W1 image and tiles

// the four parameter gradients, and one row of the pairs kernel's partials: G_W1, G_b1, G_w2, G_b2
[[maybe_unused]] constexpr size_t link_mlp_grad_floats(uint32_t d, uint32_t hd) { return (size_t)d * hd + 2 * (size_t)hd + 1; }
// the bf16 W1 image: F [hd x (d + kPad)], then B [d x (hd + kPad)] (link_mlp_b16.hip)
[[maybe_unused]] constexpr size_t link_mlp_image_halves(uint32_t d, uint32_t hd) {
    return (size_t)hd * (d + kPad) + (size_t)d * (hd + kPad);
}

// Nothing is scheduled across it.  Left to itself the scheduler hoists the LDS reads of a whole unrolled product (up to 256
// A operands) in front of its first MFMA and spills the accumulators to make room for them.
#define MLP_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)

// the row of the C layout that register r of lane half h holds
__device__ __forceinline__ constexpr int c_row(int r, int h) { return 8 * (r >> 2) + 4 * h + (r & 3); }

// sum over the 32 lanes of a half wave, the same bits on all of them: a butterfly inside each row of 16, then the rows
__device__ __forceinline__ float half_sum(float v) {
    v = row16_reduce(v, [](float a, float b) { return a + b; });
    return v + __shfl_xor(v, 16);
}
// half_sum(w * a), the first step of the butterfly spelled out: the rounded product of lane l ^ 8 enters an fma with my own
// factors, so the lanes of a row do NOT end with the same bits.  This is the sum of a block in the pairs kernel's scores,
// and link_rank.hip's rank_score restates what lane 0 holds: the two change together or not at all.
__device__ __forceinline__ float half_dot(float w, float a) {
#pragma clang fp contract(off)
    auto ror = [](float x, auto ctrl) {
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), decltype(ctrl)::value, 0xF, 0xF, true));
    };
    float v = fmaf(w, a, ror(w * a, std::integral_constant<int, 0x128>{}));     // row_ror:8
    v = v + ror(v, std::integral_constant<int, 0x124>{});                        // row_ror:4
    v = v + ror(v, std::integral_constant<int, 0x122>{});                        // row_ror:2
    v = v + ror(v, std::integral_constant<int, 0x121>{});                        // row_ror:1
    return v + __shfl_xor(v, 16);
}
__device__ __forceinline__ uint32_t half_sum_u32(uint32_t v) {
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) v += (uint32_t)__shfl_xor((int)v, off);
    return v;
}

__device__ __forceinline__ void load4(float (&r)[4], const float *p, bool vec) {
    if (vec) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w;
    } else {
        r[0] = p[0]; r[1] = p[1]; r[2] = p[2]; r[3] = p[3];
    }
}

// ---- bf16 operands (link_mlp_b16.hip says what the order of a 32-block is)
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__host__ __device__ __forceinline__ constexpr uint32_t perm32(uint32_t i) { return (i & ~12u) | ((i & 4u) << 1) | ((i & 8u) >> 1); }

__device__ __forceinline__ uint32_t bf16_pair(float lo, float hi) {      // round to nearest even: v_cvt_pk_bf16_f32
    return (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)lo) | ((uint32_t)__builtin_bit_cast(uint16_t, (__bf16)hi) << 16);
}
__device__ __forceinline__ float widen_lo(uint32_t p) { return __uint_as_float(p << 16); }
__device__ __forceinline__ float widen_hi(uint32_t p) { return __uint_as_float(p & 0xFFFF0000u); }

[[maybe_unused]] bool overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a_bytes && b_bytes && x < y + b_bytes && y < x + a_bytes;
}
// of an fp32 matrix; an image of 2-byte elements passes elem = 2
[[maybe_unused]] size_t matrix_bytes(size_t rows, size_t ld, size_t d, size_t elem = sizeof(float)) {
    return rows ? ((rows - 1) * ld + d) * elem : 0;
}

[[maybe_unused]] void require_mlp_shape(uint32_t d, uint32_t hd) {
    MGGCN_REQUIRE(d >= 32 && d <= MGGCN_LINK_MLP_MAX_WIDTH && d % 32 == 0, "link mlp: d must be a multiple of 32 in [32, 128]");
    MGGCN_REQUIRE(hd >= 32 && hd <= MGGCN_LINK_MLP_MAX_WIDTH && hd % 32 == 0, "link mlp: hd must be a multiple of 32 in [32, 128]");
}

// The embeddings and W1 as an entry gets them.  elem == 4: H and W1 [d x hd] in fp32; elem == 2: Hb in bf16 and the W1 image.
struct mlp_inputs {
    const void *H;
    size_t ldh, elem;
    const void *W;
    bool image() const { return elem == 2; }
    size_t h_bytes(size_t rows, uint32_t d) const { return matrix_bytes(rows, ldh, d, elem); }
    size_t w_bytes(uint32_t d, uint32_t hd) const { return image() ? link_mlp_image_halves(d, hd) * 2 : (size_t)d * hd * 4; }
};

// what every entry asks of the two images: the walk reads 8 bytes of Hb at a time, every kernel 16 of the W1 image
[[maybe_unused]] void require_images(const mlp_inputs &in) {
    if (!in.image()) return;
    MGGCN_REQUIRE(rows16(static_cast<const uint16_t *>(in.H), in.ldh), "link mlp bf16: Hb needs an 8-byte aligned base and a leading dimension that is a multiple of 4");
    MGGCN_REQUIRE((reinterpret_cast<uintptr_t>(in.W) & 15u) == 0, "link mlp bf16: the W1 image must be 16-byte aligned");
}

// the walk's entries; false: there is nothing to launch.  (The bf16 entry looks at ldhb only when there are rows.)
[[maybe_unused]] bool require_walk(const mlp_inputs &in, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                   const uint32_t *indices, size_t nnz, uint32_t d, uint32_t hd, const float *b1, const float *w2,
                                   const float *b2, uint32_t R, const float *G, size_t ldg, const float *row_loss,
                                   const uint32_t *row_correct) {
    require_mlp_shape(d, hd);
    MGGCN_REQUIRE((in.image() || in.ldh >= d) && ldg >= d, "link mlp loss: leading dimension < d");
    MGGCN_REQUIRE(n_rows < (1u << 31) && n_cols < (1u << 31), "link mlp loss: n < 2^31");
    MGGCN_REQUIRE(nnz < ((size_t)1 << 31) && nnz * (R ? R : 1) < ((size_t)1 << 31), "link mlp loss: nnz * neg_ratio must be below 2^31");
    MGGCN_REQUIRE((row_loss == nullptr) == (row_correct == nullptr), "link mlp loss: row_loss and row_correct come together");
    if (!n_rows) return false;
    MGGCN_REQUIRE(indptr != nullptr && in.H != nullptr && G != nullptr, "link mlp loss: null operand");
    MGGCN_REQUIRE(in.W != nullptr && b1 != nullptr && w2 != nullptr && b2 != nullptr, "link mlp loss: null parameter");
    MGGCN_REQUIRE(nnz == 0 || (indices != nullptr && n_cols != 0), "link mlp loss: null operand");
    MGGCN_REQUIRE(in.ldh >= d, "link mlp loss: leading dimension < d");
    require_images(in);
    const size_t h_rows = n_rows > n_cols ? n_rows : n_cols;    // H is indexed by the row and by the entry
    const size_t g_bytes = matrix_bytes(n_rows, ldg, d), h_bytes = in.h_bytes(h_rows, d);
    MGGCN_REQUIRE(!overlap(G, g_bytes, in.H, h_bytes) && !overlap(G, g_bytes, in.W, in.w_bytes(d, hd)), "link mlp loss: G must not overlap an input");
    if (row_loss != nullptr)
        MGGCN_REQUIRE(!overlap(row_loss, (size_t)n_rows * 8, row_correct, (size_t)n_rows * 4) &&
                          !overlap(row_loss, (size_t)n_rows * 8, G, g_bytes) && !overlap(row_correct, (size_t)n_rows * 4, G, g_bytes) &&
                          !overlap(row_loss, (size_t)n_rows * 8, in.H, h_bytes) && !overlap(row_correct, (size_t)n_rows * 4, in.H, h_bytes),
                      "link mlp loss: the outputs must not overlap each other or H");
    return true;
}

// the pairs' entries; returns the length of the list, explicit (m) or the training list's M (1 + R).  partial_floats is
// mggcn_link_mlp_partial_floats(d, hd).
[[maybe_unused]] size_t require_pairs(const mlp_inputs &in, const uint32_t *src, const uint32_t *dst, size_t m, const uint32_t *head,
                                      const uint32_t *indices, size_t M, uint32_t R, uint32_t n_draw, size_t n_rows, uint32_t d,
                                      uint32_t hd, const float *b1, const float *w2, const float *b2, const float *out,
                                      const float *grads, const float *partials, size_t partial_floats) {
    require_mlp_shape(d, hd);
    MGGCN_REQUIRE(in.ldh >= d, "link mlp pairs: leading dimension < d");
    MGGCN_REQUIRE((src == nullptr) == (dst == nullptr), "link mlp pairs: src and dst come together");
    MGGCN_REQUIRE((grads == nullptr) == (partials == nullptr), "link mlp pairs: the gradients need their partials");
    MGGCN_REQUIRE(out != nullptr || grads != nullptr, "link mlp pairs: nothing to write");
    if (src == nullptr) {                           // the training list of P
        MGGCN_REQUIRE(M < ((size_t)1 << 31) && M * (R ? R : 1) < ((size_t)1 << 31), "link mlp pairs: M * neg_ratio must be below 2^31");
        MGGCN_REQUIRE(R == 0 || (n_draw >= 1 && n_draw < (1u << 31)), "link mlp pairs: 1 <= n < 2^31");
        m = M * (1 + (size_t)R);
        MGGCN_REQUIRE(m == 0 || (head != nullptr && indices != nullptr), "link mlp pairs: null operand");
    }
    MGGCN_REQUIRE(m < ((size_t)1 << 32), "link mlp pairs: the list must be shorter than 2^32");
    if (!m) return 0;
    MGGCN_REQUIRE(in.H != nullptr && n_rows != 0, "link mlp pairs: null operand");
    MGGCN_REQUIRE(in.W != nullptr && b1 != nullptr && w2 != nullptr && b2 != nullptr, "link mlp pairs: null parameter");
    require_images(in);
    const size_t h_bytes = in.h_bytes(n_rows, d), w_bytes = in.w_bytes(d, hd), width = link_mlp_grad_floats(d, hd);
    MGGCN_REQUIRE(out == nullptr || !overlap(out, m * 4, in.H, h_bytes), "link mlp pairs: out must not overlap H");
    MGGCN_REQUIRE(grads == nullptr || (!overlap(grads, width * 4, in.H, h_bytes) && !overlap(grads, width * 4, in.W, w_bytes) &&
                                       !overlap(partials, partial_floats * 4, in.H, h_bytes) &&
                                       !overlap(partials, partial_floats * 4, in.W, w_bytes) &&
                                       !overlap(partials, partial_floats * 4, grads, width * 4)),
                  "link mlp pairs: the gradients must not overlap an input or their partials");
    return m;
}

// the end of the pairs' entries: grads = the sum of the `grid` partials in workgroup order; an empty list (grid == 0) stores zeros
[[maybe_unused]] void pairs_final(hipStream_t st, const float *partials, unsigned grid, uint32_t d, uint32_t hd, float *grads) {
    const size_t width = link_mlp_grad_floats(d, hd);
    hipLaunchKernelGGL(colsum_final_kernel, dim3((unsigned)((width + 63) / 64)), dim3(256), 0, st, partials, grid, (uint32_t)width,
                       grads, grads, (uint32_t)width);
    MGGCN_CHECK_LAUNCH();
}

// f(std::integral_constant DB, HB)
template <class F>
void mlp_dispatch(uint32_t d, uint32_t hd, F f) {
    const auto by_hb = [&](auto db) {
        switch (hd / 32) {
        case 1: f(db, std::integral_constant<int, 1>{}); break;
        case 2: f(db, std::integral_constant<int, 2>{}); break;
        case 3: f(db, std::integral_constant<int, 3>{}); break;
        default: f(db, std::integral_constant<int, 4>{}); break;
        }
    };
    switch (d / 32) {
    case 1: by_hb(std::integral_constant<int, 1>{}); break;
    case 2: by_hb(std::integral_constant<int, 2>{}); break;
    case 3: by_hb(std::integral_constant<int, 3>{}); break;
    default: by_hb(std::integral_constant<int, 4>{}); break;
    }
}

}  // namespace
