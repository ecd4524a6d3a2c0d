// test_dist.cpp -- the distributed (1D row partition) classes of the C++ host layer on the GPU.
//
//   test_dist [P]        P ranks in one process (default 1); with MGGCN_OVERSUBSCRIBE=1 the ranks wrap over
//                        the visible GPUs and the communication library runs its peer-copy transport
//
// The reference has no test of this path (its only distributed test covers the column partition,
// test/test_dist_matrix.cpp:12-51): parity unpinned by the reference.  Pinned here against the single-GPU
// `gcn` of the same layer at the same padded class count (src/main.cpp:135): dist_gcn<true,...> in every
// exchange schedule (allgather in K pieces / halo / the reference's rounds), overlap on and off (-S),
// fused and reference launch sequences.  P = 1 must reproduce the single-GPU gradients BIT FOR BIT (same
// kernels on the same operands); P > 1 regroups the sums: 1e-4 relative on the loss and every gradient of BOTH epochs
// (the second epoch restarts from the single-GPU parameters, see run_dist).  Every case runs twice -- one enqueue
// thread per GPU (host/enqueue.hpp, the default from two ranks on) and the reference's one-thread loops
// (MGGCN_ENQUEUE_THREADS=0) -- and the two must agree BIT FOR BIT: per GPU the same commands in the same order.
// test_late_rank: the per-pair ordering of the peer-copy transport and its deferred release (include/mggcn_comm.h).
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "check.hpp"
#include "gcn.hpp"

using x_t = unsigned;
using v_t = unsigned;
using r_t = float;

struct lcg {
    std::uint64_t s;
    std::uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (std::uint32_t)(s >> 33); }
    float unit() { return (float)(next() & 0xFFFFFF) / (float)0x1000000; }
};

static csr_matrix<x_t, v_t, r_t> make_graph(v_t n, std::uint64_t seed) {
    lcg g{seed};
    std::vector<x_t> ptr(n + 1, 0);
    std::vector<v_t> idx;
    std::vector<r_t> val;
    for (v_t r = 0; r < n; r++) {
        v_t deg = 6 + g.next() % 30;
        if (r % 389 == 5) deg = 700;                   // a few heavy rows (sliced by the SpMM plan)
        if (r % 97 == 11) deg = 1;                     // self-loop only
        idx.push_back(r);                              // self-loop first (prep.py:113)
        val.push_back(1.f);
        for (v_t k = 1; k < deg; k++) { idx.push_back(g.next() % n); val.push_back(1.f); }
        ptr[r + 1] = (x_t)idx.size();
    }
    return csr_matrix<x_t, v_t, r_t>(std::move(ptr), std::move(idx), std::move(val), n);
}

static double relerr(const std::vector<float> &got, const std::vector<float> &want) {
    double num = 0, den = 0;
    for (std::size_t i = 0; i < want.size(); i++) {
        num = std::max(num, std::fabs((double)got[i] - (double)want[i]));
        den = std::max(den, std::fabs((double)want[i]));
    }
    return num / (den + 1e-30);
}

struct epoch_result {
    float loss[2], acc[2];
    std::vector<std::vector<float>> G_W[2], G_b[2];           // gradients of epoch 0 and of epoch 1
    std::vector<std::vector<float>> W1, b1;                   // parameters after epoch 0's Adam step
    std::vector<std::vector<float>> W;                        // ... and after epoch 1's
};

static epoch_result run_single(csr_matrix<x_t, v_t, r_t> A, const std::vector<std::size_t> &sizes, dn_matrix<r_t> X,
                               dn_matrix<std::int32_t> Y, bool fused) {
    context ctx(0);
    gcn<x_t, v_t, r_t> G(A, sizes, false, fused);
    epoch_result r;
    for (int e = 0; e < 2; e++) {
        auto [loss, acc] = G.train_forward(ctx, X, Y);
        G.backward(ctx);
        ctx.sync();
        for (auto &l : G.layers()) { r.G_W[e].push_back(l.GW().to_host()); r.G_b[e].push_back(l.Gb().to_host()); }
        G.adam_update(ctx, 1e-2, 0.9, 0.999, 5e-4, 1e-8);
        ctx.sync();
        r.loss[e] = loss;
        r.acc[e] = acc;
        if (e == 0)
            for (auto &l : G.layers()) { r.W1.push_back(l.W().to_host()); r.b1.push_back(l.b().to_host()); }
    }
    for (auto &l : G.layers()) r.W.push_back(l.W().to_host());
    return r;
}

// Every epoch is held to the 1e-4 bar.  Epoch 0 starts from identical seed-99 parameters.  Adam's first step is
// lr * g / (|g| + eps): where |g| is rounding noise its SIGN -- a whole 0.01 step of that weight -- differs between two
// correct summation orders, so a free-running second epoch of a P > 1 model (regrouped sums) is not comparable at 1e-4.
// Therefore: after epoch 0's Adam step the replicas are (1) checked against the single-GPU parameters up to such sign
// flips (|dW| <= 2 lr), then (2) OVERWRITTEN with the single-GPU parameters, and epoch 1 -- the epoch that re-uses
// every buffer, event and exchange slot of the multi-stream schedule -- is compared at 1e-4: loss and every G_W / G_b.
static epoch_result run_dist(std::size_t P, csr_matrix<x_t, v_t, r_t> A0, const std::vector<std::size_t> &sizes, dn_matrix<r_t> X,
                             dn_matrix<std::int32_t> Y, bool fused, dist_mode mode, bool overlap, std::string *transport,
                             const epoch_result &single) {
    // the CLI's sequence, src/main.cpp:134-153
    csr_matrix<x_t, v_t, r_t> A(A0.indptr(), A0.indices(), A0.data(), A0.m());
    dist_context ctx(P, overlap);
    *transport = ctx.transport();
    std::vector<v_t> p(P + 1);
    for (std::size_t i = 1; i < p.size(); i++) p[i] = (v_t)(i * A.n() / P);
    A.normalize(true);
    auto A_T = A.transpose();
    dist_row_dn_matrix<std::int32_t> Yd(ctx, Y);
    dist_row_csr_matrix<x_t, v_t, r_t> Ad(ctx, A, p, p), A_Td(ctx, A_T, p, p);
    dist_gcn<true, x_t, v_t, r_t> G(ctx, Ad, A_Td, sizes, false, fused, mode);
    dist_row_dn_matrix<r_t> Xd(ctx, X);
    epoch_result r;
    for (int e = 0; e < 2; e++) {
        auto [loss, acc] = G.train_forward(ctx, Xd, Yd);
        G.backward(ctx);
        ctx.sync();
        for (auto &l : G.layers()) {
            for (std::size_t j = 1; j < P; j++) {          // replicas agree bit for bit after the all-reduce
                ctx[j].set();
                CHECK(l.GW()[j].to_host() == l.GW()[0].to_host());
                CHECK(l.Gb()[j].to_host() == l.Gb()[0].to_host());
            }
            ctx[0].set();
            r.G_W[e].push_back(l.GW()[0].to_host());
            r.G_b[e].push_back(l.Gb()[0].to_host());
        }
        G.adam_update(ctx, 1e-2, 0.9, 0.999, 5e-4, 1e-8);
        ctx.sync();
        r.loss[e] = loss;
        r.acc[e] = acc;
        std::size_t li = 0;
        for (auto &l : G.layers()) {
            for (std::size_t j = 1; j < P; j++) { ctx[j].set(); CHECK(l.W()[j].to_host() == l.W()[0].to_host()); }
            ctx[0].set();
            if (e == 0) {
                r.W1.push_back(l.W()[0].to_host());
                r.b1.push_back(l.b()[0].to_host());
                for (std::size_t j = 0; j < P; j++) {      // (2) every replica continues from the single-GPU parameters
                    ctx[j].set();
                    auto Wj = l.W()[j], bj = l.b()[j];     // shared handles of replica j's buffers
                    Wj.init(single.W1[li]);
                    bj.init(single.b1[li]);
                }
                ctx[0].set();
            } else {
                r.W.push_back(l.W()[0].to_host());
            }
            li++;
        }
        ctx.sync();
    }
    mggcn_set_device(0);
    return r;
}

static double max_abs_diff(const std::vector<float> &a, const std::vector<float> &b) {
    double m = a.size() == b.size() ? 0.0 : 1e30;
    for (std::size_t i = 0; i < a.size() && i < b.size(); i++) m = std::max(m, std::fabs((double)a[i] - (double)b[i]));
    return m;
}

static void compare(std::size_t P, const epoch_result &d, const epoch_result &s, double n) {
    const double tol = 1e-4;
    for (int e = 0; e < 2; e++) {
        CHECK(std::fabs(d.loss[e] - s.loss[e]) <= (P == 1 ? 1e-6 : tol) * std::fabs(s.loss[e]));
        CHECK(std::fabs(d.acc[e] - s.acc[e]) <= 3.0 / n);
        for (std::size_t l = 0; l < s.G_W[e].size(); l++) {
            if (P == 1) {                                  // same kernels on the same operands
                CHECK(d.G_W[e][l] == s.G_W[e][l]);
                CHECK(d.G_b[e][l] == s.G_b[e][l]);
            } else {
                CHECK(relerr(d.G_W[e][l], s.G_W[e][l]) <= tol);
                CHECK(relerr(d.G_b[e][l], s.G_b[e][l]) <= tol);
            }
        }
    }
    CHECK((d.loss[1] < d.loss[0]) == (s.loss[1] < s.loss[0]));      // training moves the way the single-GPU model moves (a width-1 bottleneck may go up)
    for (std::size_t l = 0; l < s.W1.size(); l++) {
        if (P == 1) {
            CHECK(d.W1[l] == s.W1[l]);
            CHECK(d.W[l] == s.W[l]);
        } else {
            // (1) the replicas' own Adam step: equal up to sign flips of rounding-noise gradients (2 lr = 0.02)
            CHECK(max_abs_diff(d.W1[l], s.W1[l]) <= 2.05e-2);
            CHECK(max_abs_diff(d.b1[l], s.b1[l]) <= 2.05e-2);
            // second Adam step from the same parameters and (nearly) the same moments
            CHECK(max_abs_diff(d.W[l], s.W[l]) <= 2.05e-2);
        }
    }
}

static bool same_bits(const epoch_result &a, const epoch_result &b) {
    bool ok = a.W1 == b.W1 && a.b1 == b.b1 && a.W == b.W;
    for (int e = 0; e < 2; e++) ok = ok && a.loss[e] == b.loss[e] && a.acc[e] == b.acc[e] && a.G_W[e] == b.G_W[e] && a.G_b[e] == b.G_b[e];
    return ok;
}

// One rank's comm stream is LATE (a queue of large GEMMs in front of the exchange).  Broadcast of rank 0's shard:
//   * a receiver that is on time gets its copy without waiting for the late rank (the round-3 transport bracketed every
//     exchange with an all-streams barrier: everybody finished when the slowest rank had pulled);
//   * the late rank still receives the ORIGINAL data although the root overwrites its shard right after the exchange:
//     the root's release (deferred to the stream that overwrites, MGGCN_COMM_DEFER_RELEASE) waits for that reader.
// Event timestamps on the ranks' own streams; meaningful on the p2p transport (the only one a one-GPU box can run at P > 1).
static void test_late_rank(std::size_t P) {
    dist_context ctx(P, true);
    const int cs = ctx.bcast_stream_id();
    const std::size_t rows = 64 * P, d = 256, late = P - 1, on_time = 1;
    std::vector<float> vals(rows * d);
    for (std::size_t i = 0; i < vals.size(); i++) vals[i] = (float)(i % 1009) + 0.5f;
    dn_matrix<r_t> host(rows, d);
    host.init(vals);
    dist_row_dn_matrix<r_t> B(ctx, host), R(ctx, rows, d);
    R.zero(ctx);
    ctx.sync();
    // the delay: ten 3072^3 products on the late rank's comm stream (several ms)
    // (MGGCN_TEST_DELAY_GEMM: a smaller product for the model runs of tests/native, where a "device" is a CPU loop)
    const std::uint32_t g = std::getenv("MGGCN_TEST_DELAY_GEMM") ? (std::uint32_t)std::atoi(std::getenv("MGGCN_TEST_DELAY_GEMM")) : 3072;
    ctx[late].set();
    dn_matrix<r_t> ga(g, g), gb(g, g), gc(g, g);
    ga.zero(ctx[late]); gb.zero(ctx[late]);
    ctx.sync();
    ctx.on(late, [c = ctx[late], ga, gb, gc, g, cs] {
        c.set();
        c.record("delay-0", cs);
        const auto ws = mggcn_gemm_workspace_bytes(0, 0, g, g, g);
        for (int k = 0; k < 10; k++)
            mggcn_gemm_f32(c.stream(cs), 0, 0, g, g, g, 1.f, ga.buffer(), g, gb.buffer(), g, 0.f, gc.buffer(), g, c.gemm_workspace(ws), ws);
        c.record("delay-1", cs);
    });
    ctx.record("t0", cs);
    B.bcast(ctx, 0, R, cs);
    ctx.record("t1", cs);
    ctx.register_timer("exchange", "t0", "t1");
    ctx.on(late, [c = ctx[late]] { c.register_timer("delay", "delay-0", "delay-1"); });
    // the overwrite below runs on the COMPUTE stream: ordered after the exchange on every transport (a collective frees its send
    // buffer in the order of the stream it was issued on -- found missing by the stream model of tests/native on the RCCL transport)
    ctx.wait("t1", 0);
    ctx.release_sends(0);                                  // the root's compute stream waits for every reader ...
    B.zero(ctx);                                           // ... and only then overwrites what it sent
    ctx.sync();
    const float delay = ctx[late].measure("delay"), t_on_time = ctx[on_time].measure("exchange");
    const std::vector<float> want(vals.begin(), vals.begin() + (rows / P) * d);
    for (std::size_t j = 0; j < P; j++) { ctx[j].set(); CHECK(R[j].to_host() == want); }
    // the timing claim needs the on-time rank's streams on hardware queues of their own.  Streams are multiplexed over a few
    // hardware queues per device and priority (GPU_MAX_HW_QUEUES, 4 by default) and two streams that share a queue run one
    // after the other: with P ranks x (compute, comm, P - 1 pulling streams) on ONE device the late rank's queue of GEMMs
    // holds up whoever shares its hardware queue.  Two queues per rank keep the ranks apart (measured with 4 and 8 queues at
    // P = 4, profiles/experiments/time_dist_tests_r04.log); the test leaves the runtime's setting alone.
    // (delay == 0: the stream model of tests/native has no clock -- the data claims above still hold there)
    const char *hwq = std::getenv("GPU_MAX_HW_QUEUES");
    const std::size_t queues = hwq && std::atoi(hwq) > 0 ? (std::size_t)std::atoi(hwq) : 4;
    const bool timed = ctx.transport() == "p2p" && 2 * P <= queues && delay > 0.f;
    if (timed) CHECK(t_on_time < 0.5f * delay);
    std::printf("%s: late rank: delay %.2f ms, on-time receiver's exchange %.3f ms%s, transport %s, threads %d, hw queues %zu\n",
                (!timed || t_on_time < 0.5f * delay) ? "TEST PASSED" : "TEST FAILED", delay, t_on_time, timed ? "" : " (not asserted)",
                ctx.transport().c_str(), (int)ctx.threaded(), queues);
    mggcn_set_device(0);
}

int main(int argc, char **argv) {
    // test_dist P [n graph_seed F C hidden...]: the defaults are the fixed case of the suite; tests/test_gpu_host_cpp.py also
    // walks a few random shapes (odd widths, one hidden layer, class counts that need padding to a multiple of P)
    const std::size_t P = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
    if (P == 1) setenv("MGGCN_DIST_SELF_GATHER", "1", 0);       // one rank: still put RCCL's all-gather through its paces
    const v_t n = argc > 2 ? (v_t)std::strtoull(argv[2], nullptr, 10) : 1536;      // 1536: divisible by 1, 2, 3, 4, 6, 8
    if (P == 0 || n % P != 0) { std::fprintf(stderr, "P must divide %u\n", n); return 2; }
    mggcn_set_device(0);
    const auto A = make_graph(n, argc > 3 ? (std::uint32_t)std::strtoull(argv[3], nullptr, 10) : 42u);
    const std::size_t F = argc > 4 ? std::strtoull(argv[4], nullptr, 10) : 24, C = argc > 5 ? std::strtoull(argv[5], nullptr, 10) : 6;
    std::vector<std::size_t> sizes{F};
    if (argc > 6) for (int i = 6; i < argc; i++) sizes.push_back(std::strtoull(argv[i], nullptr, 10));
    else { sizes.push_back(32); sizes.push_back(16); }                    // first layer out > in: SpMM first
    sizes.push_back((C + P - 1) / P * P);                                 // src/main.cpp:135
    lcg g{7};
    std::vector<float> xs(n * F);
    for (auto &x : xs) x = 2.f * g.unit() - 1.f;
    std::vector<std::int32_t> ys(n);
    for (auto &y : ys) y = (std::int32_t)(g.next() % C);
    dn_matrix<r_t> X(n, F);
    X.init(xs);
    dn_matrix<std::int32_t> Y(n, 1);
    Y.init(ys);

    for (const bool fused : {true, false}) {
        const auto single = run_single(csr_matrix<x_t, v_t, r_t>(A.indptr(), A.indices(), A.data(), A.m()), sizes, X, Y, fused);
        for (const auto mode : {dist_mode::allgather, dist_mode::halo, dist_mode::rounds})
            for (const bool overlap : {true, false}) {
                epoch_result by_threads[2];
                for (const int threads : {1, 0}) {         // one enqueue thread per GPU / the calling thread does it all
                    if (!threads && !(fused && overlap)) continue;   // (the one-thread form: fused sequence with overlap only -- suite time)
                    const int before = g_failures;
                    setenv("MGGCN_ENQUEUE_THREADS", threads ? "1" : "0", 1);
                    std::string transport;
                    const auto dist = run_dist(P, A, sizes, X, Y, fused, mode, overlap, &transport, single);
                    compare(P, dist, single, (double)n);
                    by_threads[threads] = dist;
                    if (!threads) CHECK(same_bits(by_threads[0], by_threads[1]));
                    const char *mn = mode == dist_mode::allgather ? "allgather" : mode == dist_mode::halo ? "halo" : "rounds";
                    std::printf("%s: dist_gcn P=%zu %s overlap=%d fused=%d threads=%d transport=%s  loss %.7f -> %.7f (single GPU %.7f -> %.7f)\n",
                                g_failures == before ? "TEST PASSED" : "TEST FAILED", P, mn, (int)overlap, (int)fused, threads, transport.c_str(),
                                dist.loss[0], dist.loss[1], single.loss[0], single.loss[1]);
                }
            }
    }
    unsetenv("MGGCN_ENQUEUE_THREADS");
    if (P >= 3)
        for (const int threads : {1, 0}) {
            setenv("MGGCN_ENQUEUE_THREADS", threads ? "1" : "0", 1);
            test_late_rank(P);
        }
    unsetenv("MGGCN_ENQUEUE_THREADS");
    // halo volume matrix of the partition (the figure test/data/prep.py:237-244 prints)
    if (P > 1) {
        dist_context ctx(P);
        CHECK((std::size_t)mggcn_comm_size(ctx.comm()) == P);
        {   // the exported displacement tables (include/mggcn_comm.h) on a ragged count matrix: prefix sums per sender / receiver
            std::vector<std::size_t> counts(P * P), sdis(P * P), rdis(P * P);
            for (std::size_t q = 0; q < P * P; q++) counts[q] = (q * 7 + 3) % 11;
            mggcn_comm_alltoallv_displacements((int)P, counts.data(), sdis.data(), rdis.data());
            for (std::size_t j = 0; j < P; j++) {
                std::size_t s = 0, r = 0;
                for (std::size_t k = 0; k < P; k++) {
                    CHECK(sdis[j * P + k] == s);
                    CHECK(rdis[j * P + k] == r);
                    s += counts[j * P + k];                 // what j sends to k
                    r += counts[k * P + j];                 // what j receives from k
                }
            }
        }
        std::vector<v_t> p(P + 1);
        for (std::size_t i = 1; i < p.size(); i++) p[i] = (v_t)(i * n / P);
        dist_row_csr_matrix<x_t, v_t, r_t> Ad(ctx, A, p, p);
        const auto V = Ad.halo_volume();
        std::size_t tot = 0;
        for (const auto &row : V) for (auto v : row) tot += v;
        CHECK(tot > 0 && tot <= (P - 1) * (std::size_t)n);
        CHECK(V[0][0] == 0);
        std::printf("%s: halo volume %zu rows of %zu (all-gather)\n", tot <= (P - 1) * (std::size_t)n ? "TEST PASSED" : "TEST FAILED", tot,
                    (P - 1) * (std::size_t)n);
    }
    return g_failures ? 1 : 0;
}
