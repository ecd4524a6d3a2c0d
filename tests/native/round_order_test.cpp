// round_order_test.cpp -- which sweep tasks share a launch round (plan_host.h: "tasks in non-increasing padded length; a
// launch round is a contiguous chunk of that order").  Stand-alone, plain build, no oracle:
//   g++ -std=c++17 -O2 -pthread -I mg-gcn_amd/csrc tests/native/round_order_test.cpp mg-gcn_amd/csrc/plan_host.cpp -o round_order_test
// (tests/test_plan_round_order_cpu.py does exactly that).
//
//   round_order_test                      the checks: every case with MGGCN_SPMM_SORT_ROUNDS = 1 and = 0 in one process
//   round_order_test --file F CUS W D     the figures: F = a CSR matrix as u32 n_rows, n_cols, nnz, indptr[n_rows + 1],
//                                         indices[nnz], f32 values[nnz]; cut into column slices of W columns (0 = one slice)
//                                         and built for a device of CUS compute units at d_hint D, with the knob at 0 and 1
//
// Checks, per case and form (wide: d_hint 0; narrow: d_hint 41):
//   1. sorted table: end - beg never grows from one task to the next
//   2. the sorted plan is a permutation of the unsorted one: every task has a twin with the same row count, the same row
//      table and the same entry sequence; split_rows and n_slots are equal
//   3. sum over the rounds of the longest task: sorted <= unsorted, and < in the case made of two classes of task
//   4. plans built with 1 and with 5 host threads are identical
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "plan_host.h"

using namespace mggcn_plan;

static int g_failures = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            if (g_failures < 40) std::fprintf(stderr, "FAILURE: %s at %s:%d\n", #cond, __FILE__, __LINE__); \
            g_failures++;                                                                \
        }                                                                                \
    } while (0)

struct lcg {
    std::uint64_t s;
    std::uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (std::uint32_t)(s >> 33); }
    float unit() { return (float)(next() & 0xFFFFFF) / (float)0x1000000; }
};

struct Csr {
    uint32_t n = 0, m = 0;
    std::vector<uint32_t> ip, ix;
    std::vector<float> v;
};

// heavy = false: every row has exactly `deg` non-zeros; true: short rows and a few long enough to be sliced
static Csr make_csr(uint32_t n, uint32_t m, uint32_t deg, bool heavy, uint64_t seed) {
    lcg g{seed};
    Csr A;
    A.n = n; A.m = m;
    A.ip.assign(n + 1, 0);
    for (uint32_t r = 0; r < n; r++) {
        uint32_t len = deg;
        if (heavy) {
            len = deg / 4 + g.next() % deg;
            if (r % 97 == 5) len = 30 * deg;
            if (r % 601 == 3) len = 100 * deg;
        }
        for (uint32_t k = 0; k < len; k++) { A.ix.push_back(g.next() % m); A.v.push_back(0.25f + g.unit()); }
        A.ip[r + 1] = (uint32_t)A.ix.size();
    }
    return A;
}

static bool build(const Csr &A, const uint32_t *ip, const uint32_t *ix, const float *vv, uint32_t d_hint, uint32_t num_cu, int sorted,
                  int threads, SweepHost &h) {
    setenv("MGGCN_SPMM_SORT_ROUNDS", sorted ? "1" : "0", 1);
    if (threads > 0) setenv("MGGCN_HOST_THREADS", std::to_string(threads).c_str(), 1);
    return sweep_build_host(A.n, A.m, ip, ix, vv, 128, true, d_hint, true, num_cu, h);
}

static uint64_t sum_round_max(const SweepHost &h) {
    uint64_t sum = 0;
    for (size_t t0 = 0; t0 < h.tasks.size(); t0 += h.round_tasks) {
        uint32_t longest = 0;
        for (size_t t = t0; t < std::min(h.tasks.size(), t0 + (size_t)h.round_tasks); t++) longest = std::max(longest, h.tasks[t].end - h.tasks[t].beg);
        sum += longest;
    }
    return sum;
}

// a task as bytes: rows in use, its row table, its entry sequence
static std::string task_key(const SweepHost &h, uint32_t t) {
    const SweepTask &tk = h.tasks[t];
    std::string key((const char *)&tk.n_rows, sizeof tk.n_rows);
    key.append((const char *)&h.task_rows[(size_t)t * kRW], kRW * sizeof(uint32_t));
    if (tk.end > tk.beg) key.append((const char *)&h.entries[tk.beg], (size_t)(tk.end - tk.beg) * sizeof(Entry));
    return key;
}

static bool same_plan(const SweepHost &a, const SweepHost &b) {
    auto bytes_equal = [](const auto &x, const auto &y) {
        return x.size() == y.size() && (x.empty() || std::memcmp(x.data(), y.data(), x.size() * sizeof(x[0])) == 0);
    };
    return a.n_tasks == b.n_tasks && a.round_tasks == b.round_tasks && a.n_slots == b.n_slots && a.run_pad == b.run_pad && a.lpe == b.lpe &&
           a.n_entries == b.n_entries && bytes_equal(a.tasks, b.tasks) && bytes_equal(a.entries, b.entries) &&
           bytes_equal(a.task_rows, b.task_rows) && bytes_equal(a.split_rows, b.split_rows);
}

static void check_case(const char *name, const Csr &A, uint32_t d_hint, uint32_t num_cu, bool two_classes, bool want_split_rows) {
    const int before = g_failures;
    SweepHost s, u, s5, u5;
    CHECK(build(A, A.ip.data(), A.ix.data(), A.v.data(), d_hint, num_cu, 1, 1, s));
    CHECK(build(A, A.ip.data(), A.ix.data(), A.v.data(), d_hint, num_cu, 0, 1, u));
    CHECK(build(A, A.ip.data(), A.ix.data(), A.v.data(), d_hint, num_cu, 1, 5, s5));
    CHECK(build(A, A.ip.data(), A.ix.data(), A.v.data(), d_hint, num_cu, 0, 5, u5));
    const uint32_t rounds = (s.n_tasks + s.round_tasks - 1) / s.round_tasks;
    CHECK(s.round_tasks == num_cu * 16u && rounds >= 3);                  // several full rounds, or there is nothing to order
    CHECK(want_split_rows ? !s.split_rows.empty() : s.split_rows.empty());
    // 1. non-increasing over the table
    for (uint32_t t = 0; t + 1 < s.n_tasks; t++) CHECK(s.tasks[t].end - s.tasks[t].beg >= s.tasks[t + 1].end - s.tasks[t + 1].beg);
    // 2. a permutation of the unsorted plan
    CHECK(s.n_tasks == u.n_tasks && s.round_tasks == u.round_tasks && s.n_entries == u.n_entries && s.n_slots == u.n_slots);
    CHECK(s.run_pad == u.run_pad && s.lpe == u.lpe && s.panel_rows == u.panel_rows);
    CHECK(s.split_rows.size() == u.split_rows.size() &&
          (s.split_rows.empty() || std::memcmp(s.split_rows.data(), u.split_rows.data(), s.split_rows.size() * sizeof(SweepSplitRow)) == 0));
    std::map<std::string, long> twins;
    for (uint32_t t = 0; t < u.n_tasks; t++) twins[task_key(u, t)]++;
    for (uint32_t t = 0; t < s.n_tasks; t++) {
        auto it = twins.find(task_key(s, t));
        CHECK(it != twins.end() && it->second > 0);
        if (it != twins.end()) it->second--;
    }
    for (const auto &kv : twins) CHECK(kv.second == 0);
    // 3. what the rounds wait for
    const uint64_t ms = sum_round_max(s), mu = sum_round_max(u);
    CHECK(ms <= mu);
    if (two_classes) CHECK(ms < mu);
    CHECK(s.round_excess <= u.round_excess && s.round_excess >= 0.0);
    // 4. thread count
    CHECK(same_plan(s, s5));
    CHECK(same_plan(u, u5));
    std::printf("%s: %s d_hint=%u tasks=%u rounds=%u run_pad=%u split_rows=%zu sum_round_max sorted=%llu unsorted=%llu round_excess sorted=%.4f unsorted=%.4f\n",
                g_failures == before ? "TEST PASSED" : "TEST FAILED", name, d_hint, s.n_tasks, rounds, s.run_pad, s.split_rows.size(),
                (unsigned long long)ms, (unsigned long long)mu, s.round_excess, u.round_excess);
}

// ---- the figures on a matrix from a file ---------------------------------------------------------------------------------
static void print_rounds(const char *label, const SweepHost &h, double seconds) {
    std::printf("%s tasks=%u round_tasks=%u run_pad=%u build_s=%.3f round_excess=%.4f sum_round_max=%llu\n", label, h.n_tasks, h.round_tasks,
                h.run_pad, seconds, h.round_excess, (unsigned long long)sum_round_max(h));
    for (size_t t0 = 0; t0 < h.tasks.size(); t0 += h.round_tasks) {
        std::vector<uint32_t> len;
        for (size_t t = t0; t < std::min(h.tasks.size(), t0 + (size_t)h.round_tasks); t++) len.push_back(h.tasks[t].end - h.tasks[t].beg);
        std::sort(len.begin(), len.end());
        double mean = 0;
        for (uint32_t l : len) mean += l;
        mean /= (double)len.size();
        std::printf("  round %zu: tasks=%zu mean=%.0f p50=%u p99=%u max=%u\n", t0 / h.round_tasks, len.size(), mean, len[len.size() / 2],
                    len[std::min(len.size() - 1, len.size() * 99 / 100)], len.back());
    }
}

static int figures(const char *path, uint32_t num_cu, uint32_t width, uint32_t d_hint) {
    std::FILE *f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 2; }
    uint32_t head[3];
    Csr A;
    bool ok = std::fread(head, 4, 3, f) == 3;
    if (ok) {
        A.n = head[0]; A.m = head[1];
        A.ip.resize((size_t)A.n + 1); A.ix.resize(head[2]); A.v.resize(head[2]);
        ok = std::fread(A.ip.data(), 4, A.ip.size(), f) == A.ip.size() && std::fread(A.ix.data(), 4, A.ix.size(), f) == A.ix.size() &&
             std::fread(A.v.data(), 4, A.v.size(), f) == A.v.size();
    }
    std::fclose(f);
    if (!ok || A.ip[A.n] != head[2] || !columns_in_range(A.n, A.m, A.ip.data(), A.ix.data())) { std::fprintf(stderr, "%s: not a CSR file\n", path); return 2; }
    const uint32_t S = width ? (A.m + width - 1) / width : 1u;
    SliceBuckets sl;
    if (S > 1) sl = slice_buckets(A.n, S, width, A.ip.data(), A.ix.data(), A.v.data());
    for (uint32_t k = 0; k < S; k++)
        for (int sorted = 0; sorted < 2; sorted++) {
            SweepHost h;
            const auto t0 = std::chrono::steady_clock::now();
            const bool built = S > 1 ? build(A, sl.ips[k].data(), sl.ixs[k].data(), sl.vvs[k].data(), d_hint, num_cu, sorted, 0, h)
                                     : build(A, A.ip.data(), A.ix.data(), A.v.data(), d_hint, num_cu, sorted, 0, h);
            const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (!built) { std::fprintf(stderr, "slice %u: no sweep plan\n", k); return 2; }
            char label[64];
            std::snprintf(label, sizeof label, "slice %u sort_rounds=%d", k, sorted);
            print_rounds(label, h, sec);
        }
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 6 && !std::strcmp(argv[1], "--file"))
        return figures(argv[2], (uint32_t)std::atoi(argv[3]), (uint32_t)std::atoi(argv[4]), (uint32_t)std::atoi(argv[5]));
    if (argc != 1) { std::fprintf(stderr, "usage: %s [--file F CUS SLICE_WIDTH D_HINT]\n", argv[0]); return 2; }
    setenv("MGGCN_HOST_THREADS_MIN_NNZ", "1", 1);             // every pass threaded at these sizes
    // A: the quantisation in miniature.  2 CUs = rounds of 32 tasks; 1 820 rows of exactly 64 non-zeros = 128 tasks in 4
    // rounds at 14.2 rows per task: tasks of 14 and of 15 rows
    const Csr A = make_csr(1820, 16384, 64, false, 20261);
    // B: the same size with rows short and long: the long ones are sliced and their slices are rows of their own
    const Csr B = make_csr(1820, 16384, 64, true, 20262);
    for (const uint32_t d_hint : {0u, 41u}) {
        check_case("even rows", A, d_hint, 2, true, false);
        check_case("heavy rows", B, d_hint, 2, false, true);
    }
    std::printf(g_failures ? "FAILED (%d)\n" : "ALL PASSED\n", g_failures);
    return g_failures ? 1 : 0;
}
