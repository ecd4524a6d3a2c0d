// row_values_test.cpp -- the row-value entry stream of a sweep plan (plan_host.h: SweepHost::row_values).  Stand-alone,
// plain build, no oracle:
//   g++ -std=c++17 -O2 -pthread -I mg-gcn_amd/csrc tests/native/row_values_test.cpp mg-gcn_amd/csrc/plan_host.cpp -o row_values_test
// (tests/test_plan_row_values_cpu.py does exactly that).
//
// Checks, per case (short rows / with sliced rows) and form (wide: d_hint 0; narrow: d_hint 41 and 16):
//   1. detection: one value per row -> row stream; one entry changed, a non-finite value, too many columns for the
//      padding column, or MGGCN_SPMM_ROW_VALUES=0 -> generic stream only
//   2. tasks (range, rows), row tables, split rows, rounds and round_excess are those of the generic build; the generic
//      stream itself is bit for bit the one built with the knob at 0
//   3. value table: task row r holds the value of its matrix row (every slice of a split row too), 0 for unused rows
//   4. padding contract: a real entry keeps its word; run padding = the generic word + n_cols, behind the run's real
//      entries, upper entry of its pair when the run is padded to 2; tail padding = SweepTask::pad entries at the end,
//      the first with the run flag, columns in range
//   5. expanding the row stream by the rule of the device's sweep_expand_kernel gives the generic stream bit for bit
//   6. plans built with 1 and with 5 host threads are identical
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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

// every row carries ONE value; an empty row, a one-entry row, odd and even lengths; heavy: rows long enough to be sliced
static Csr make_csr(uint32_t n, uint32_t m, bool heavy, uint64_t seed) {
    lcg g{seed};
    Csr A;
    A.n = n; A.m = m;
    A.ip.assign(n + 1, 0);
    for (uint32_t r = 0; r < n; r++) {
        uint32_t len = 3 + g.next() % 40;
        if (r == 0) len = 0;
        if (r == 1) len = 1;
        if (heavy && r % 13 == 5) len = 700 + g.next() % 900;
        const float val = 0.25f + g.unit();
        for (uint32_t k = 0; k < len; k++) { A.ix.push_back(g.next() % m); A.v.push_back(val); }
        A.ip[r + 1] = (uint32_t)A.ix.size();
    }
    return A;
}

static bool build(const Csr &A, const std::vector<float> &v, uint32_t d_hint, const char *knob, int threads, SweepHost &h) {
    if (knob) setenv("MGGCN_SPMM_ROW_VALUES", knob, 1); else unsetenv("MGGCN_SPMM_ROW_VALUES");
    setenv("MGGCN_HOST_THREADS", std::to_string(threads).c_str(), 1);
    setenv("MGGCN_HOST_THREADS_MIN_NNZ", "1", 1);
    setenv("MGGCN_SPMM_PANEL_ROWS", "1024", 1);
    setenv("MGGCN_SPMM_PANEL_ROWS_NARROW", "1024", 1);
    setenv("MGGCN_SPMM_SWEEP_SPLIT", "256", 1);
    return sweep_build_host(A.n, A.m, A.ip.data(), A.ix.data(), v.data(), 128, true, d_hint, true, 2, h);
}

template <typename T> static bool bytes_equal(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

static uint32_t bits(float f) { uint32_t w; std::memcpy(&w, &f, 4); return w; }

static void check_case(const char *name, const Csr &A, uint32_t d_hint) {
    const int before = g_failures;
    SweepHost row, gen, row5;
    CHECK(build(A, A.v, d_hint, nullptr, 1, row));
    CHECK(build(A, A.v, d_hint, "0", 1, gen));
    CHECK(build(A, A.v, d_hint, "1", 5, row5));
    // 1. detection
    CHECK(row.row_values && !gen.row_values && gen.entries32.empty() && gen.task_vals.empty());
    {
        SweepHost h;
        std::vector<float> v = A.v;
        v[v.size() / 2] += 0.5f;
        CHECK(build(A, v, d_hint, nullptr, 1, h) && !h.row_values && h.entries32.empty());
        for (const SweepTask &t : h.tasks) CHECK(t.pad == 0);
        v = A.v;
        for (uint32_t e = A.ip[A.n - 1]; e < A.ip[A.n]; e++) v[e] = std::numeric_limits<float>::infinity();   // a whole row
        CHECK(build(A, v, d_hint, nullptr, 1, h) && !h.row_values);
    }
    // 2. the plan around the stream
    CHECK(row.n_tasks == gen.n_tasks && row.round_tasks == gen.round_tasks && row.n_entries == gen.n_entries);
    CHECK(row.run_pad == gen.run_pad && row.lpe == gen.lpe && row.n_slots == gen.n_slots && row.panel_rows == gen.panel_rows);
    CHECK(row.round_excess == gen.round_excess);
    CHECK(bytes_equal(row.task_rows, gen.task_rows) && bytes_equal(row.split_rows, gen.split_rows));
    CHECK(bytes_equal(row.entries, gen.entries));
    CHECK(row.tasks.size() == gen.tasks.size());
    for (size_t t = 0; t < row.tasks.size() && t < gen.tasks.size(); t++) {
        CHECK(row.tasks[t].beg == gen.tasks[t].beg && row.tasks[t].end == gen.tasks[t].end && row.tasks[t].n_rows == gen.tasks[t].n_rows);
        CHECK(gen.tasks[t].pad == 0);
    }
    CHECK(row.entries32.size() == row.n_entries && row.task_vals.size() == (size_t)row.n_tasks * kRW);
    // slot -> matrix row
    std::vector<uint32_t> slot_row(row.n_slots, 0u);
    for (const SweepSplitRow &s : row.split_rows)
        for (uint32_t k = 0; k < s.n_slots; k++) slot_row[s.first_slot + k] = s.row;
    uint64_t n_run_pad = 0, n_tail = 0, n_sliced_vals = 0;
    for (uint32_t t = 0; t < row.n_tasks; t++) {
        const SweepTask &tk = row.tasks[t];
        // 3. value table
        for (uint32_t r = 0; r < (uint32_t)kRW; r++) {
            const float got = row.task_vals[(size_t)t * kRW + r];
            if (r >= tk.n_rows) { CHECK(bits(got) == 0u); continue; }
            const uint32_t dst = row.task_rows[(size_t)t * kRW + r];
            const uint32_t mr = (dst & kSlotFlag) ? slot_row[dst & ~kSlotFlag] : dst;
            n_sliced_vals += (dst & kSlotFlag) != 0;
            const float want = A.ip[mr] < A.ip[mr + 1] ? A.v[A.ip[mr]] : 0.f;
            CHECK(bits(got) == bits(want));
        }
        // 4. padding contract, 5. expansion
        CHECK(tk.pad <= tk.end - tk.beg && tk.pad % row.run_pad == 0);
        const uint32_t tail0 = tk.end - tk.pad;
        uint32_t run_start = tk.beg;
        bool seen_pad_in_run = false;
        for (uint32_t i = tk.beg; i < tk.end; i++) {
            const uint32_t x = row.entries32[i];
            const Entry g = row.entries[i];
            Entry back;
            if (i >= tail0) {
                n_tail++;
                CHECK(((x & kRunFlag) != 0) == (i == tail0));
                CHECK((x & kColMask) < A.m);
                back = Entry{x & ~kRunFlag, 0u};
            } else {
                if (x & kRunFlag) { run_start = i; seen_pad_in_run = false; }
                if ((x & kColMask) >= A.m) {
                    n_run_pad++;
                    seen_pad_in_run = true;
                    CHECK(!(x & kRunFlag));                                  // a run starts with a real entry
                    CHECK((x & kColMask) < 2u * A.m);
                    if (row.run_pad == 2) CHECK(((i - run_start) & 1u) == 1u);   // the upper entry of its pair
                    back = Entry{x - A.m, 0u};
                } else {
                    CHECK(!seen_pad_in_run);                                 // padding stays behind the real entries
                    back = Entry{x, bits(row.task_vals[(size_t)t * kRW + ((x >> kColBits) & (kRW - 1))])};
                }
            }
            CHECK(back.x == g.x && back.y == g.y);
        }
        if (tk.end > tk.beg) CHECK(row.entries32[tk.beg] & kRunFlag);
    }
    CHECK(n_run_pad > 0 && n_tail > 0);
    // 6. threads
    CHECK(bytes_equal(row.entries32, row5.entries32) && bytes_equal(row.task_vals, row5.task_vals) && bytes_equal(row.tasks, row5.tasks));
    std::printf("%s: %s d_hint=%u tasks=%u entries=%llu run_pad=%u run_padding=%llu tail=%llu split_rows=%zu sliced_row_values=%llu\n",
                g_failures == before ? "TEST PASSED" : "TEST FAILED", name, d_hint, row.n_tasks, (unsigned long long)row.n_entries,
                row.run_pad, (unsigned long long)n_run_pad, (unsigned long long)n_tail, row.split_rows.size(),
                (unsigned long long)n_sliced_vals);
}

int main() {
    const Csr even = make_csr(200, 5000, false, 7), heavy = make_csr(200, 5000, true, 11);
    for (uint32_t d_hint : {0u, 41u, 16u}) {
        check_case("short rows", even, d_hint);
        check_case("with sliced rows", heavy, d_hint);
    }
    {   // the padding column n_cols + c must fit the entry's column field: 27 bits wide, 24 in the narrow form
        Csr wide = make_csr(40, (1u << 23) + 1u, false, 3);
        SweepHost h;
        CHECK(build(wide, wide.v, 41, nullptr, 1, h) && !h.row_values);
        CHECK(build(wide, wide.v, 0, nullptr, 1, h) && h.row_values);
        std::printf("%s: column range\n", g_failures ? "TEST FAILED" : "TEST PASSED");
    }
    if (g_failures) { std::printf("%d FAILURES\n", g_failures); return 1; }
    std::printf("ALL PASSED\n");
    return 0;
}
