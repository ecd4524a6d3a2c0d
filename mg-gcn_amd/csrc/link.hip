// link.hip -- the link-prediction head (include/mggcn.h, "link prediction"): a dot-product decoder over pairs of rows of one
// embedding matrix H, the binary cross-entropy of its scores against uniformly drawn negatives, and the gradient of BOTH
// endpoints without an atomic.  No reference counterpart.
//
// The gradient of a vertex x sums over the pairs it heads and over the pairs it ends.  Each of the three sets of pairs is a
// CSR pattern whose row x lists the other endpoints, and one kernel walks all three, one after the other, adding into G:
//     (a) P         positives headed by x, and -- drawn inside the walk, entry position p being the walk's own index -- the
//                   R negatives (x, v') of each
//     (b) P^T       positives that end in x
//     (c) NT        negatives that end in x: the pairs (v', u) of the draw kernel, put in order of v' by the stable radix
//                   sort (radix_sort.hip), cut into rows by a binary search per vertex
// A launch writes G[x] = beta G[x] + (its sum): (a) with beta = 0, (b) and (c) with beta = 1, in that order, so G has the same
// bits on every call.
//
// The walk is the attention kernels' (gat_internal.h, the layout gat.hip describes) without their softmax: one wave per row,
// the row's own H[x] in registers for the whole walk, groups of LPR lanes that each own one entry at a time, a lane gathering
// four columns (float4 path) or one (element path) of H[y], the dot product a butterfly over the group's lanes, the pair's
// scalar g formed on every lane of the group from the same s, and the gathered row used a second time for acc += g H[y]:
// one gather per pair serves the score and the gradient.  The groups' accumulators meet in fold_groups' fixed order at the end
// of the row.  A row's work is a matrix-vector product against gathered rows: nothing for the matrix cores (the MLP decoder of
// link_mlp.hip, whose hidden layer makes a tile of pairs a real GEMM, is).
//
// Launch (a) also leaves three numbers per row -- the sum of softplus(-s) over its positives, of softplus(s) over its
// negatives, and the number of pairs on the right side of 0 -- which mggcn_link_sums_f32 adds through the tree of reduce.h
// (the count in integers).
#include "edge_draw.h"
#include "gat_internal.h"
#include "link_pair.h"

namespace {

// R == 0: no negatives are drawn (launches (b) and (c)); row_loss == nullptr: no row sums are written
template <int VEC, int NT, int U>
__global__ __launch_bounds__(256) void link_dot_loss_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr,
                                                            const uint32_t *__restrict__ indices,
                                                            const float *__restrict__ H, size_t ldh, uint32_t d, uint32_t lg,
                                                            bool positive, float weight, uint32_t R, float neg_weight,
                                                            uint32_t n_draw, uint32_t k0, uint32_t k1, uint32_t epoch,
                                                            float beta, float *__restrict__ G, size_t ldg,
                                                            float *__restrict__ row_loss, uint32_t *__restrict__ row_correct) {
    MGGCN_GAT_WAVE_ROW(n_rows);
    const uint32_t beg = indptr[row], end = indptr[row + 1];
    float h[NT][VEC], acc[NT][VEC];
    load_head_row<VEC, NT>(h, H + row * ldh, lpr, sub, d);
    zero_head_row<VEC, NT>(acc);
    float loss_pos = 0.f, loss_neg = 0.f;       // of my group: every lane of a group holds the same bits
    uint32_t hits = 0;

    // the entries my_c of lanes [0, cnt): U per group and step, all of one label and weight
    const auto walk = [&](uint32_t my_c, uint32_t cnt, bool pos, float w, float &loss) {
        for (uint32_t j = 0; j < cnt; j += n_grp * U) {
            float z[U][NT][VEC], p[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const uint32_t src = j + u * n_grp + grp;
                const uint32_t c = (uint32_t)__shfl((int)my_c, src & 63);
                ok[u] = src < cnt;
                load_head_row<VEC, NT>(z[u], H + (size_t)c * ldh, lpr, sub, d, ok[u]);
                p[u] = dot_head_row<VEC, NT>(h, z[u]);
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const pair_terms t = link_pair(group_sum(p[u], lpr), pos, w);
                axpy_head_row<VEC, NT>(acc, ok[u] ? t.g : 0.f, z[u]);       // z is zero where the entry does not exist
                loss += ok[u] ? t.loss : 0.f;
                hits += ok[u] ? t.hit : 0u;
            }
        }
    };

    entry_chunks<0> ch;
    ch.start(indices, beg, end, lane, no_scalars);
    for (uint32_t base = beg; base < end; base += 64) {
        ch.next(indices, base, end, lane, no_scalars);
        const uint32_t cnt = ch.cnt;
        walk(ch.my_c, cnt, positive, weight, positive ? loss_pos : loss_neg);
        if (R) {                                // the negatives of my entry, position base + lane: never stored
            link_negatives neg{base + lane, n_draw, k0, k1, epoch, {}};
            for (uint32_t r = 0; r < R; r++) walk(neg.next(r), cnt, false, neg_weight, loss_neg);
        }
    }

    float *__restrict__ g_row = G + row * ldg;
#pragma unroll
    for (int t = 0; t < NT; t++) {
#pragma unroll
        for (int v = 0; v < VEC; v++) acc[t][v] = fold_groups(acc[t][v], lpr);
        const uint32_t col = (t * lpr + sub) * VEC;
        if (grp == 0 && col < d) {
            if (beta != 0.f) {                  // beta == 0 never reads G
                float old[VEC];
                loadv<VEC>(old, g_row + col);
#pragma unroll
                for (int v = 0; v < VEC; v++) acc[t][v] = fmaf(beta, old[v], acc[t][v]);
            }
            storev<VEC>(g_row + col, acc[t]);
        }
    }
    if (row_loss != nullptr) {
        loss_pos = fold_groups(loss_pos, lpr);
        loss_neg = fold_groups(loss_neg, lpr);
        hits = fold_groups_u32(hits, lpr);
        if (lane == 0) {
            row_loss[2 * row] = loss_pos;
            row_loss[2 * row + 1] = loss_neg;
            row_correct[row] = hits;
        }
    }
}

// out[e] = H[src[e]] . H[dst[e]]: one lane group per pair, 64 / LPR pairs per wave
template <int VEC, int NT>
__global__ __launch_bounds__(256) void edge_dot_kernel(const uint32_t *__restrict__ src, const uint32_t *__restrict__ dst,
                                                       size_t m, const float *__restrict__ H, size_t ldh, uint32_t d,
                                                       uint32_t lg, float *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63, lpr = 1u << lg, n_grp = 64u >> lg, sub = lane & (lpr - 1), grp = lane >> lg;
    const size_t e = ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * n_grp + grp;
    const bool ok = e < m;                      // a group beyond the list loads nothing and stores nothing
    const uint32_t u = ok ? src[e] : 0u, v = ok ? dst[e] : 0u;
    float a[NT][VEC], b[NT][VEC];
    load_head_row<VEC, NT>(a, H + (size_t)u * ldh, lpr, sub, d, ok);
    load_head_row<VEC, NT>(b, H + (size_t)v * ldh, lpr, sub, d, ok);
    const float s = group_sum(dot_head_row<VEC, NT>(a, b), lpr);
    if (ok && sub == 0) out[e] = s;
}

// one wave per row of P, lanes over its entries: the R negatives of entry p at [p R, (p + 1) R)
__global__ __launch_bounds__(256) void link_neg_draw_kernel(uint32_t n_rows, const uint32_t *__restrict__ indptr, uint32_t n,
                                                            uint32_t R, uint32_t k0, uint32_t k1, uint32_t epoch,
                                                            uint32_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const uint32_t lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    const uint32_t beg = indptr[row], end = indptr[row + 1];
    for (size_t p = (size_t)beg + lane; p < end; p += 64) {
        link_negatives neg{(uint32_t)p, n, k0, k1, epoch, {}};
        for (uint32_t r = 0; r < R; r++) {
            keys[p * R + r] = neg.next(r);
            vals[p * R + r] = (uint32_t)row;
        }
    }
}

// nt_indptr[v] = #{sorted keys < v}, v = 0 .. n: the lower bound by bisection
__global__ __launch_bounds__(256) void link_bounds_kernel(const uint32_t *__restrict__ keys, uint32_t m, uint32_t n,
                                                          uint32_t *__restrict__ nt_indptr) {
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v > n) return;
    uint32_t lo = 0, hi = m;                    // keys[i] < v for i < lo, >= v for i >= hi
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    nt_indptr[v] = lo;
}

// the rows' three numbers, per workgroup: rows t, t + (grid 256), ... per thread, then the tree of reduce.h; the count in integers
__global__ __launch_bounds__(256) void link_sums_partial_kernel(const float *__restrict__ row_loss,
                                                                const uint32_t *__restrict__ row_correct, size_t n_rows,
                                                                float *__restrict__ partials, uint32_t *__restrict__ counts) {
    __shared__ float w[2][4];
    __shared__ uint32_t wc[4];
    float v[2] = {0.f, 0.f};
    uint32_t c = 0;
    for (size_t r = (size_t)blockIdx.x * 256 + threadIdx.x; r < n_rows; r += (size_t)gridDim.x * 256) {
        v[0] += row_loss[2 * r];
        v[1] += row_loss[2 * r + 1];
        c += row_correct[r];
    }
    v[0] = wave_sum(v[0]);
    v[1] = wave_sum(v[1]);
    c = fold_groups_u32(c, 1);
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = c;
    block_fold<2>(v, w, partials + 2 * blockIdx.x);         // holds the barrier
    if (threadIdx.x == 0) counts[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}
__global__ __launch_bounds__(256) void link_count_final_kernel(const uint32_t *__restrict__ counts, unsigned n_blocks,
                                                               uint32_t *__restrict__ out) {
    __shared__ uint32_t wc[4];
    uint32_t c = 0;
    for (unsigned i = threadIdx.x; i < n_blocks; i += 256) c += counts[i];
    c = fold_groups_u32(c, 1);
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) *out = wc[0] + wc[1] + wc[2] + wc[3];
}

bool overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a_bytes && b_bytes && x < y + b_bytes && y < x + a_bytes;
}
size_t matrix_bytes(size_t rows, size_t ld, size_t d) { return rows ? ((rows - 1) * ld + d) * sizeof(float) : 0; }

void require_link_width(uint32_t d) {
    MGGCN_REQUIRE(d >= 1 && d <= MGGCN_GAT_MAX_WIDTH, "link: the embedding width must be 1 <= d <= 1024");
}

}  // namespace

MGGCN_API void mggcn_link_neg_draw_u32(mggcn_stream_t stream, uint32_t n_rows, const uint32_t *indptr, size_t nnz, uint32_t n,
                                       uint32_t R, uint64_t seed, uint32_t epoch, uint32_t *keys, uint32_t *vals) {
    MGGCN_REQUIRE(R >= 1, "link draw: neg_ratio must be at least 1");
    MGGCN_REQUIRE(n >= 1 && n < (1u << 31), "link draw: 1 <= n < 2^31");
    MGGCN_REQUIRE(nnz < ((size_t)1 << 31) && nnz * R < ((size_t)1 << 31), "link draw: nnz * neg_ratio must be below 2^31");
    if (!n_rows || !nnz) return;
    MGGCN_REQUIRE(indptr != nullptr && keys != nullptr && vals != nullptr, "link draw: null operand");
    MGGCN_REQUIRE(!overlap(keys, nnz * R * 4, vals, nnz * R * 4), "link draw: keys and vals must not overlap");
    launch_rows(link_neg_draw_kernel, n_rows, stream, n_rows, indptr, n, R, (uint32_t)(seed & 0xFFFFFFFFull),
                (uint32_t)(seed >> 32), epoch, keys, vals);
}

MGGCN_API void mggcn_link_bounds_u32(mggcn_stream_t stream, const uint32_t *sorted_keys, size_t m, uint32_t n,
                                     uint32_t *nt_indptr) {
    MGGCN_REQUIRE(m < ((size_t)1 << 31), "link bounds: the list must be shorter than 2^31");
    MGGCN_REQUIRE(n < (1u << 31), "link bounds: n < 2^31");
    MGGCN_REQUIRE(nt_indptr != nullptr && (m == 0 || sorted_keys != nullptr), "link bounds: null operand");
    MGGCN_REQUIRE(!overlap(sorted_keys, m * 4, nt_indptr, ((size_t)n + 1) * 4), "link bounds: nt_indptr must not overlap the keys");
    hipLaunchKernelGGL(link_bounds_kernel, dim3((unsigned)(((size_t)n + 1 + 255) / 256)), dim3(256), 0, as_stream(stream),
                       sorted_keys, (uint32_t)m, n, nt_indptr);
    MGGCN_CHECK_LAUNCH();
}

MGGCN_API void mggcn_link_dot_loss_f32(mggcn_stream_t stream, uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr,
                                       const uint32_t *indices, size_t nnz, const float *H, size_t ldh, uint32_t d, int positive,
                                       float weight, uint32_t R, float neg_weight, uint64_t seed, uint32_t epoch, float beta,
                                       float *G, size_t ldg, float *row_loss, uint32_t *row_correct) {
    require_link_width(d);
    MGGCN_REQUIRE(ldh >= d && ldg >= d, "link loss: leading dimension < d");
    MGGCN_REQUIRE(n_rows < (1u << 31) && n_cols < (1u << 31), "link loss: n < 2^31");
    MGGCN_REQUIRE(nnz < ((size_t)1 << 31) && nnz * (R ? R : 1) < ((size_t)1 << 31), "link loss: nnz * neg_ratio must be below 2^31");
    MGGCN_REQUIRE((row_loss == nullptr) == (row_correct == nullptr), "link loss: row_loss and row_correct come together");
    if (!n_rows) return;
    MGGCN_REQUIRE(indptr != nullptr && H != nullptr && G != nullptr, "link loss: null operand");
    MGGCN_REQUIRE(nnz == 0 || (indices != nullptr && n_cols != 0), "link loss: null operand");
    const size_t h_rows = n_rows > n_cols ? n_rows : n_cols;    // H is indexed by the row and by the entry
    const size_t g_bytes = matrix_bytes(n_rows, ldg, d), h_bytes = matrix_bytes(h_rows, ldh, d);
    MGGCN_REQUIRE(!overlap(G, g_bytes, H, h_bytes), "link loss: G must not overlap H");
    if (row_loss != nullptr)
        MGGCN_REQUIRE(!overlap(row_loss, (size_t)n_rows * 8, row_correct, (size_t)n_rows * 4) &&
                          !overlap(row_loss, (size_t)n_rows * 8, G, g_bytes) && !overlap(row_correct, (size_t)n_rows * 4, G, g_bytes) &&
                          !overlap(row_loss, (size_t)n_rows * 8, H, h_bytes) && !overlap(row_correct, (size_t)n_rows * 4, H, h_bytes),
                      "link loss: the outputs must not overlap each other or H");
    const bool vec = d % 4 == 0 && rows16(H, ldh) && rows16(G, ldg);
    const head_geometry hg = head_geometry_for(d, vec);
    gat_dispatch(vec, hg.nt, [&](auto v) {
        launch_rows(link_dot_loss_kernel<v.VEC, v.NT, v.U>, n_rows, stream, n_rows, indptr, indices, H, ldh, d, hg.lg,
                    positive != 0, weight, nnz ? R : 0u, neg_weight, n_cols, (uint32_t)(seed & 0xFFFFFFFFull),
                    (uint32_t)(seed >> 32), epoch, beta, G, ldg, row_loss, row_correct);
    });
}

MGGCN_API void mggcn_link_sums_f32(mggcn_stream_t stream, const float *row_loss, const uint32_t *row_correct, size_t n_rows,
                                   float *loss_sums, uint32_t *correct_sum) {
    MGGCN_REQUIRE(loss_sums != nullptr && correct_sum != nullptr, "link sums: null operand");
    MGGCN_REQUIRE(n_rows == 0 || (row_loss != nullptr && row_correct != nullptr), "link sums: null operand");
    const hipStream_t st = as_stream(stream);
    const unsigned grid = n_rows ? stream_grid(n_rows) : 0;
    float *partials = sums_scratch<4, kSumsGridMax>(st);        // [grid][2] floats, then the counts behind every float pair
    uint32_t *counts = reinterpret_cast<uint32_t *>(partials + 2 * kSumsGridMax);
    if (grid) {
        hipLaunchKernelGGL(link_sums_partial_kernel, dim3(grid), dim3(256), 0, st, row_loss, row_correct, n_rows, partials, counts);
        MGGCN_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL((sums_final_kernel<2, false>), dim3(1), dim3(256), 0, st, partials, grid, loss_sums);
    MGGCN_CHECK_LAUNCH();
    hipLaunchKernelGGL(link_count_final_kernel, dim3(1), dim3(256), 0, st, counts, grid, correct_sum);
    MGGCN_CHECK_LAUNCH();
}

MGGCN_API void mggcn_edge_dot_f32(mggcn_stream_t stream, const uint32_t *src, const uint32_t *dst, size_t m, const float *H,
                                  size_t ldh, size_t n_rows, uint32_t d, float *out) {
    require_link_width(d);
    MGGCN_REQUIRE(ldh >= d, "edge dot: leading dimension < d");
    MGGCN_REQUIRE(m < ((size_t)1 << 31), "edge dot: the list must be shorter than 2^31");
    if (!m) return;
    MGGCN_REQUIRE(src != nullptr && dst != nullptr && H != nullptr && out != nullptr && n_rows != 0, "edge dot: null operand");
    MGGCN_REQUIRE(!overlap(out, m * 4, H, matrix_bytes(n_rows, ldh, d)) && !overlap(out, m * 4, src, m * 4) &&
                      !overlap(out, m * 4, dst, m * 4),
                  "edge dot: out must not overlap an input");
    const bool vec = d % 4 == 0 && rows16(H, ldh);
    const head_geometry hg = head_geometry_for(d, vec);
    const size_t per_block = 4 * (size_t)(64u >> hg.lg);
    gat_dispatch(vec, hg.nt, [&](auto v) {
        hipLaunchKernelGGL((edge_dot_kernel<v.VEC, v.NT>), dim3((unsigned)((m + per_block - 1) / per_block)), dim3(256), 0,
                           as_stream(stream), src, dst, m, H, ldh, d, hg.lg, out);
        MGGCN_CHECK_LAUNCH();
    });
}
