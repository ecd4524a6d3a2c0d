// gated_skip.hip -- the skip connection of the attention layers (gat(skip="add" | "gate"); PyG's GATConv(residual=True) and
// TransformerConv(root_weight=True, beta=True)): what comes after the aggregation and before the norm, row by row.
//
//   add    y = o + r
//   gate   s = sum_c (w[0,c] o[c] + w[1,c] r[c] + w[2,c] (o[c] - r[c]));  g = sigmoid(s);  y = g r + (1 - g) o
//   then   y = leaky_relu(y, 0.01) with MGGCN_GS_LEAKY_RELU
//
// o is the attention output, r = H W_r + 1 b_r^T the skip linear's, w [3 x m] the gate's parameter, g one float per row.
// The structure is the layer norm pair's (row_group.h): a row in the registers of one lane group, float4 or element path,
// butterfly row sums, and the backward's three column sums G_w without atomics -- a lane owns its columns over the
// grid-stride loop, the groups of a workgroup are added in group order in LDS, one [3 x m] partial per workgroup goes to
// the stream's scratch and colsum_final_kernel adds the partials in workgroup order.  Every [n x m] operand has a leading
// dimension of its own.
#include "common.h"
#include "reduce.h"
#include "row_group.h"
#include "scratch_internal.h"

namespace {

__device__ __forceinline__ float gs_lrelu(float x, float slope) {
    const float y = slope * x;
    return x > y ? x : y;
}

// 1 / (1 + e^-s) on the branch that never overflows: e^-|s| is in (0, 1], so no finite s gives inf / inf, and the result
// is exactly 1 (s >= 17 or so: 1 + e^-s rounds to 1) or exactly 0 (s <= -104: e^s underflows to 0) where fp32 saturates
__device__ __forceinline__ float gs_sigmoid(float s) {
    const float e = expf(-fabsf(s));
    return s >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

template <int V, int L, int K, int R, bool Gate>
__global__ __launch_bounds__(256) void gated_skip_forward_kernel(const float *__restrict__ o, size_t ldo,
                                                                 const float *__restrict__ r, size_t ldr,
                                                                 const float *__restrict__ w, float *__restrict__ y,
                                                                 size_t ldy, float *__restrict__ gate, size_t n_rows,
                                                                 uint32_t m, float slope, int leaky) {
    constexpr int NV = K * V, NW = Gate ? NV : 1;
    const ln_walk<L> at;
    float w0[NW], w1[NW], w2[NW];
    if constexpr (Gate) {
#pragma unroll
        for (int k = 0; k < K; k++) {
            const uint32_t c0 = (at.sub + (uint32_t)L * k) * V;
            ln_load<V>(&w0[k * V], w + c0, c0 < m, 0.f);
            ln_load<V>(&w1[k * V], w + m + c0, c0 < m, 0.f);
            ln_load<V>(&w2[k * V], w + 2 * (size_t)m + c0, c0 < m, 0.f);
        }
    }
    for (size_t base = 0; at.w0 + base < n_rows; base += at.gstride * R) {
        float a[R][NV], b[R][NV];
#pragma unroll
        for (int q = 0; q < R; q++) {                                            // all loads first
            const size_t row = at.g0 + base + (size_t)q * at.gstride;
            const bool live = row < n_rows;
#pragma unroll
            for (int k = 0; k < K; k++) {
                const uint32_t c0 = (at.sub + (uint32_t)L * k) * V;
                ln_load<V>(&a[q][k * V], o + row * ldo + c0, live && c0 < m, 0.f);
                ln_load<V>(&b[q][k * V], r + row * ldr + c0, live && c0 < m, 0.f);
            }
        }
#pragma unroll
        for (int q = 0; q < R; q++) {
            const size_t row = at.g0 + base + (size_t)q * at.gstride;
            const bool live = row < n_rows;
            float g = 0.f;
            if constexpr (Gate) {
                float s = 0.f;
#pragma unroll
                for (int i = 0; i < NV; i++)                                     // columns past m hold +0.0 in o, r and w
                    s += fmaf(w0[i], a[q][i], fmaf(w1[i], b[q][i], w2[i] * (a[q][i] - b[q][i])));
                g = gs_sigmoid(ln_group_sum<L>(s));
            }
#pragma unroll
            for (int k = 0; k < K; k++) {
                const uint32_t c0 = (at.sub + (uint32_t)L * k) * V;
                float out[V];
#pragma unroll
                for (int v = 0; v < V; v++) {
                    const float ov = a[q][k * V + v], rv = b[q][k * V + v];
                    const float t = Gate ? fmaf(g, rv, (1.f - g) * ov) : ov + rv;
                    out[v] = leaky ? gs_lrelu(t, slope) : t;
                }
                if (live && c0 < m) ln_store<V>(y + row * ldy + c0, out);
            }
            if (Gate && live && at.sub == 0) gate[row] = g;
        }
    }
}

// dy = G . leaky_relu'(act) (or G).  add: G_o = G_r = dy.  gate: dg = sum_c dy (r - o), ds = dg g (1 - g),
// G_o = (1 - g) dy + ds (w0 + w2), G_r = g dy + ds (w1 - w2), and the column sums G_w[0] = sum_i ds_i o_i,
// G_w[1] = sum_i ds_i r_i, G_w[2] = sum_i ds_i (o_i - r_i).  A lane reads exactly the elements it writes, and reads them
// first: G_o may be G or act.  The three sums leave through one [groups x columns] LDS buffer, one after the other.
template <int V, int L, int K, int R, bool Gate>
__global__ __launch_bounds__(256) void gated_skip_backward_kernel(const float *G, size_t ldg, const float *act, size_t lda,
                                                                  const float *__restrict__ o, size_t ldo,
                                                                  const float *__restrict__ r, size_t ldr,
                                                                  const float *__restrict__ w,
                                                                  const float *__restrict__ gate, float *G_o, size_t ldgo,
                                                                  float *G_r, size_t ldgr, float *__restrict__ partials,
                                                                  size_t n_rows, uint32_t m, float slope, int leaky) {
    constexpr int NV = K * V, NW = Gate ? NV : 1, NG = 256 / L, CP = L * NV;      // CP: columns a group covers
    __shared__ float s_part[Gate ? NG * CP : 1];                                 // [group][column], one sum at a time
    const ln_walk<L> at;
    float wo[NW], wr[NW], acc[3][NW];
    if constexpr (Gate) {
#pragma unroll
        for (int k = 0; k < K; k++) {
            const uint32_t c0 = (at.sub + (uint32_t)L * k) * V;
            float t0[V], t1[V], t2[V];
            ln_load<V>(t0, w + c0, c0 < m, 0.f);
            ln_load<V>(t1, w + m + c0, c0 < m, 0.f);
            ln_load<V>(t2, w + 2 * (size_t)m + c0, c0 < m, 0.f);
#pragma unroll
            for (int v = 0; v < V; v++) {
                wo[k * V + v] = t0[v] + t2[v];
                wr[k * V + v] = t1[v] - t2[v];
            }
        }
#pragma unroll
        for (int i = 0; i < NV; i++) acc[0][i] = acc[1][i] = acc[2][i] = 0.f;
    }
    for (size_t base = 0; at.w0 + base < n_rows; base += at.gstride * R) {
        float g[R][NV], s[R][NV], a[R][NW], b[R][NW], gt[R];
#pragma unroll
        for (int q = 0; q < R; q++) {                                            // all loads first
            const size_t row = at.g0 + base + (size_t)q * at.gstride;
            const bool live = row < n_rows;
            gt[q] = Gate && live ? gate[row] : 0.f;
#pragma unroll
            for (int k = 0; k < K; k++) {
                const uint32_t c0 = (at.sub + (uint32_t)L * k) * V;
                const bool ok = live && c0 < m;
                ln_load<V>(&g[q][k * V], G + row * ldg + c0, ok, 0.f);
                if (leaky) {                                                     // uniform
                    ln_load<V>(&s[q][k * V], act + row * lda + c0, ok, 1.f);
                } else {
#pragma unroll
                    for (int v = 0; v < V; v++) s[q][k * V + v] = 1.f;
                }
                if constexpr (Gate) {
                    ln_load<V>(&a[q][k * V], o + row * ldo + c0, ok, 0.f);
                    ln_load<V>(&b[q][k * V], r + row * ldr + c0, ok, 0.f);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < R; q++) {
            const size_t row = at.g0 + base + (size_t)q * at.gstride;
            const bool live = row < n_rows;
            float ds = 0.f;
#pragma unroll
            for (int i = 0; i < NV; i++) g[q][i] = s[q][i] > 0.f ? g[q][i] : slope * g[q][i];
            if constexpr (Gate) {
                float dg = 0.f;
#pragma unroll
                for (int i = 0; i < NV; i++) dg = fmaf(g[q][i], b[q][i] - a[q][i], dg);      // a dead row or column adds +0.0
                ds = ln_group_sum<L>(dg) * (gt[q] * (1.f - gt[q]));
#pragma unroll
                for (int i = 0; i < NV; i++) {
                    acc[0][i] = fmaf(ds, a[q][i], acc[0][i]);
                    acc[1][i] = fmaf(ds, b[q][i], acc[1][i]);
                    acc[2][i] = fmaf(ds, a[q][i] - b[q][i], acc[2][i]);
                }
            }
#pragma unroll
            for (int k = 0; k < K; k++) {
                const uint32_t c0 = (at.sub + (uint32_t)L * k) * V;
                if (!(live && c0 < m)) continue;
                if constexpr (Gate) {
                    float to[V], tr[V];
#pragma unroll
                    for (int v = 0; v < V; v++) {
                        const int i = k * V + v;
                        to[v] = fmaf(ds, wo[i], (1.f - gt[q]) * g[q][i]);
                        tr[v] = fmaf(ds, wr[i], gt[q] * g[q][i]);
                    }
                    ln_store<V>(G_o + row * ldgo + c0, to);
                    ln_store<V>(G_r + row * ldgr + c0, tr);
                } else {
                    ln_store<V>(G_o + row * ldgo + c0, &g[q][k * V]);
                    if (G_r != G_o) ln_store<V>(G_r + row * ldgr + c0, &g[q][k * V]);        // uniform
                }
            }
        }
    }
    if constexpr (Gate) {
        const uint32_t grp = threadIdx.x / L;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            if (j) __syncthreads();                                              // the previous sum has been read
#pragma unroll
            for (int i = 0; i < NV; i++) {
                const uint32_t c = (at.sub + (uint32_t)L * (i / V)) * V + (i % V);
                s_part[grp * CP + c] = acc[j][i];
            }
            __syncthreads();
            for (uint32_t c = threadIdx.x; c < (uint32_t)CP; c += 256) {
                float t = s_part[c];
#pragma unroll
                for (int q = 1; q < NG; q++) t += s_part[q * CP + c];
                if (c < m) partials[((size_t)blockIdx.x * 3 + j) * m + c] = t;
            }
        }
    }
}

bool rows_aligned16(const float *p, size_t ld) { return p == nullptr || (aligned16(p) && ld % 4 == 0); }

}  // namespace

// ============================ C ABI =========================================
MGGCN_API void mggcn_gated_skip_forward_f32(mggcn_stream_t stream, const float *o, size_t ldo, const float *r, size_t ldr,
                                            const float *w, float *y, size_t ldy, float *gate, size_t n_rows, size_t m,
                                            uint32_t flags) {
    const bool gated = (flags & MGGCN_GS_GATE) != 0;
    MGGCN_REQUIRE(m > 0 && m <= MGGCN_GS_MAX_WIDTH, "gated skip supports 1 <= m <= 1024 columns");
    MGGCN_REQUIRE(ldo >= m && ldr >= m && ldy >= m, "gated skip: a leading dimension is below m");
    MGGCN_REQUIRE(!gated || (w != nullptr && gate != nullptr), "gated skip: MGGCN_GS_GATE needs w and gate");
    if (!n_rows) return;
    MGGCN_REQUIRE(o != nullptr && r != nullptr && y != nullptr, "gated skip: null operand");
    MGGCN_REQUIRE(y != o && y != r, "gated skip: y must not alias o or r (the backward pass reads both)");
    const bool vec = m % 4 == 0 && rows_aligned16(o, ldo) && rows_aligned16(r, ldr) && rows_aligned16(y, ldy) &&
                     (!gated || aligned16(w));
    const int leaky = (flags & MGGCN_GS_LEAKY_RELU) != 0;
#define MGGCN_GS_FWD(V, L, K, R)                                                                                          \
    do {                                                                                                                  \
        if (gated)                                                                                                        \
            hipLaunchKernelGGL((gated_skip_forward_kernel<V, L, K, R, true>), dim3(layer_norm_grid<L, R>(n_rows)),        \
                               dim3(256), 0, as_stream(stream), o, ldo, r, ldr, w, y, ldy, gate, n_rows, (uint32_t)m,     \
                               0.01f, leaky);                                                                             \
        else                                                                                                              \
            hipLaunchKernelGGL((gated_skip_forward_kernel<V, L, K, R, false>), dim3(layer_norm_grid<L, R>(n_rows)),       \
                               dim3(256), 0, as_stream(stream), o, ldo, r, ldr, nullptr, y, ldy, nullptr, n_rows,         \
                               (uint32_t)m, 0.01f, leaky);                                                                \
    } while (0)
    MGGCN_LN_DISPATCH(MGGCN_GS_FWD, vec, m);
#undef MGGCN_GS_FWD
    MGGCN_CHECK_LAUNCH();
}

MGGCN_API void mggcn_gated_skip_backward_f32(mggcn_stream_t stream, const float *G, size_t ldg, const float *act, size_t lda,
                                             const float *o, size_t ldo, const float *r, size_t ldr, const float *w,
                                             const float *gate, float *G_o, size_t ldgo, float *G_r, size_t ldgr, float *G_w,
                                             size_t n_rows, size_t m, uint32_t flags) {
    const bool gated = (flags & MGGCN_GS_GATE) != 0;
    const int leaky = (flags & MGGCN_GS_LEAKY_RELU) != 0;
    MGGCN_REQUIRE(m > 0 && m <= MGGCN_GS_MAX_WIDTH, "gated skip supports 1 <= m <= 1024 columns");
    MGGCN_REQUIRE(ldg >= m && ldgo >= m && ldgr >= m && (!leaky || lda >= m) && (!gated || (ldo >= m && ldr >= m)),
                  "gated skip backward: a leading dimension is below m");
    MGGCN_REQUIRE(!gated || (w != nullptr && gate != nullptr && G_w != nullptr),
                  "gated skip backward: MGGCN_GS_GATE needs w, gate and G_w");
    const hipStream_t st = as_stream(stream);
    const unsigned final_grid = (unsigned)((3 * m + 63) / 64);
    if (!n_rows) {                                                    // the sums over no rows
        if (gated) {
            hipLaunchKernelGGL(colsum_final_kernel, dim3(final_grid), dim3(256), 0, st, nullptr, 0u, 3 * (uint32_t)m, G_w,
                               G_w, 3 * (uint32_t)m);
            MGGCN_CHECK_LAUNCH();
        }
        return;
    }
    MGGCN_REQUIRE(G != nullptr && G_o != nullptr && G_r != nullptr && (!leaky || act != nullptr),
                  "gated skip backward: null operand");
    MGGCN_REQUIRE(!gated || (o != nullptr && r != nullptr), "gated skip backward: MGGCN_GS_GATE needs o and r");
    MGGCN_REQUIRE(!gated || (G_r != G_o && G_r != G && G_r != act && G_r != o && G_r != r && G_o != o && G_o != r),
                  "gated skip backward: with MGGCN_GS_GATE G_r is distinct from every other operand, G_o from o and r");
    const bool vec = m % 4 == 0 && rows_aligned16(G, ldg) && rows_aligned16(G_o, ldgo) && rows_aligned16(G_r, ldgr) &&
                     (!leaky || rows_aligned16(act, lda)) &&
                     (!gated || (rows_aligned16(o, ldo) && rows_aligned16(r, ldr) && aligned16(w)));
    float *partials = gated ? stream_scratch(st, scratch_kind::colsums, (size_t)kLayerNormBlocks * 3 * m) : nullptr;
    unsigned grid = 0;
#define MGGCN_GS_BWD(V, L, K, R)                                                                                          \
    do {                                                                                                                  \
        grid = layer_norm_grid<L, R>(n_rows);                                                                             \
        if (gated)                                                                                                        \
            hipLaunchKernelGGL((gated_skip_backward_kernel<V, L, K, R, true>), dim3(grid), dim3(256), 0, st, G, ldg, act, \
                               lda, o, ldo, r, ldr, w, gate, G_o, ldgo, G_r, ldgr, partials, n_rows, (uint32_t)m, 0.01f,  \
                               leaky);                                                                                    \
        else                                                                                                              \
            hipLaunchKernelGGL((gated_skip_backward_kernel<V, L, K, R, false>), dim3(grid), dim3(256), 0, st, G, ldg,     \
                               act, lda, nullptr, 0, nullptr, 0, nullptr, nullptr, G_o, ldgo, G_r, ldgr, nullptr, n_rows, \
                               (uint32_t)m, 0.01f, leaky);                                                                \
    } while (0)
    MGGCN_LN_DISPATCH(MGGCN_GS_BWD, vec, m);
#undef MGGCN_GS_BWD
    MGGCN_CHECK_LAUNCH();
    if (gated) {
        hipLaunchKernelGGL(colsum_final_kernel, dim3(final_grid), dim3(256), 0, st, partials, grid, 3 * (uint32_t)m, G_w, G_w,
                           3 * (uint32_t)m);
        MGGCN_CHECK_LAUNCH();
    }
}
