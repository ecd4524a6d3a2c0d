// plan_host.h -- the HOST passes of the SpMM plan builders, free of HIP.
//
// mggcn_spmm_plan_create_for (spmm.hip) = these passes + device allocation and upload.  They live in
// their own translation unit (plan_host.cpp) so that the same code can be compiled with plain g++
// under AddressSanitizer / UndefinedBehaviorSanitizer / ThreadSanitizer and driven on the CPU
// (tests/native/plan_host_test.cpp, `make -C tests/native sanitize`, tests/test_sanitizers.py): the passes are threaded
// (per-thread counters, per-row offsets, one task range per thread) and build the packed entry
// streams every sweep kernel trusts blindly.  Not part of the ABI.
//
// What the reference has in this place: nothing -- cusparseSpMM's workspace query
// (src/cuda_utils.hpp:94-102) hides whatever preprocessing cuSPARSE does.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace mggcn_plan {

// ---- row-split form (spmm.hip) ---------------------------------------------------------------
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;

struct SpmmItem {
    uint32_t row;   // output row
    uint32_t beg;   // first non-zero (absolute offset into indices/values)
    uint32_t end;   // one past the last
    uint32_t slot;  // kNoSlot: write C directly; else: partial-sum slot
};

struct SplitRow {
    uint32_t row;
    uint32_t first_slot;
    uint32_t n_slots;
    uint32_t pad;
};

struct RowSplitHost {
    std::vector<SpmmItem> items;          // longest first; ties in row order
    std::vector<SplitRow> split_rows;
    uint32_t n_slots = 0;
};
// heavy rows (longer than 1.5 x split) are cut into contiguous slices with partial-sum slots
RowSplitHost rowsplit_build(uint32_t n_rows, const uint32_t *indptr, uint32_t split);

// ---- sweep form (spmm_sweep.hip) -------------------------------------------------------------
constexpr int kRW = 16;                 // output rows per wave (4 row bits in the packed entry)
constexpr uint32_t kColBits = 27;       // columns < 134 M (papers100M: 111 M)
constexpr uint32_t kColMask = (1u << kColBits) - 1;
constexpr uint32_t kSlotFlag = 0x80000000u;    // task-row table: the row is a partial-sum slot
constexpr uint32_t kRunFlag = 0x80000000u;     // entry bit 31: first entry of a (panel,row) run; bits 30..27: row
constexpr int kWavesPerBlock = 4;
// internal launch flags (never part of the ABI's flags): bit 8 = rotate the wave priority, bits 12..15 = log2 of the
// rotation period in entries, bits 16..27 = compute units of the device (hardware wave slot of a block = block / CUs)
constexpr uint32_t kFlagPrioRotate = 0x100u;
constexpr uint32_t kPrioShiftPos = 12;
constexpr uint32_t kNumCuPos = 16, kNumCuMask = 0xFFFu;

struct SweepTask {
    uint32_t beg, end;   // entry range
    uint32_t n_rows;     // rows in use (<= kRW)
    uint32_t pad;        // row-value stream: entries of the tail run at the end of the range (below); 0 in the generic stream
};

struct SweepSplitRow {
    uint32_t row, first_slot, n_slots, pad;
};

struct Entry {           // layout of the device's uint2: {run:1 | row:4 | column:27, value bits}
    uint32_t x, y;
};

// everything sweep_plan_build decides and assembles before the first device call
struct SweepHost {
    uint32_t n_rows = 0, n_cols = 0, max_d = 0;
    uint32_t n_tasks = 0, round_tasks = 0, n_slots = 0;
    uint32_t run_pad = 2;          // every (panel,row) run is a multiple of this many entries
    uint32_t lpe = 0;              // narrow form: lanes per entry of the gather kernel (run_pad = 64 / lpe); 0 = wide form
    uint32_t panel_rows = 0;
    uint32_t num_cu = 0;
    uint64_t n_entries = 0;        // padded entry stream length
    // tuning knobs, read from the environment ONCE when the plan is built (never on the launch path)
    uint32_t prio_bits_wide = 0, prio_bits_narrow = 0;   // kFlagPrioRotate | shift << kPrioShiftPos | CUs << kNumCuPos
    uint32_t tasks_per_wave = 1;
    bool allow_quad = true, allow_vec4 = true, fast_pairs = true;
    double round_excess = 0.0;     // sum over the launch rounds of the longest task / sum of the rounds' mean task, minus 1
    // Task order (MGGCN_SPMM_SORT_ROUNDS, default 1): tasks in non-increasing padded length (end - beg), ties in the order
    // the LPT pass made them; a launch round is a contiguous chunk of round_tasks tasks of that order, so the tasks that
    // share a launch are as close in length as the plan allows.  With the knob at 0, and always in the experimental XCD
    // column layout (its task index encodes the slice), the table stays in LPT order.
    std::vector<SweepTask> tasks;
    std::vector<Entry> entries;                // generic stream (built in either case; a row-value plan does not upload it)
    std::vector<uint32_t> task_rows;           // n_tasks x kRW: output row or kSlotFlag | slot
    // Row-value stream (MGGCN_SPMM_ROW_VALUES, default 1 = where the matrix allows it).  When every stored value of a row
    // has the same bit pattern, for all rows of this plan (any unweighted graph's D^-1 A; split rows: every slice carries
    // its row's value), the stream drops the value word: entries32 holds the packed words {run | row | column} of the
    // generic stream in the same order and the same padded lengths, task_vals the value of each task row (0 for an empty
    // or unused row).  The kernels compute fmaf(v, b, acc) with v = the run's row value: the same operands in the same
    // order as the generic stream.  Padding, which the generic stream does with zero-valued copies:
    //   * run padding: column = n_cols + the column of the run's last entry.  It sorts last in its pair, and the row
    //     gathers put it where the buffer descriptor's bounds check sees it (the lane's own offset: the narrow kernel's
    //     whole offset, the pair kernel's upper-half offset -- the pair's lower entry is always a real one at run_pad 2),
    //     so the lane gets zeros without touching memory and adds v * 0.  Needs 2 n_cols <= 2^27 (2^24 in the narrow
    //     form, whose offsets are 24-bit products) and, at the call, (n_cols + 1) x row pitch <= 2^32 (narrow form: 2 n_cols x
    //     pitch, the whole product is the lane's).  With B finite the sum differs from the generic stream's at most in the
    //     sign of an exact zero (v * 0 against 0 * b).
    //   * tail padding up to the batch size: ONE run of its own at the end of the task (run flag set, columns = the last
    //     entry's, so the gathers are real and in range); SweepTask::pad counts its entries and the kernels drop its sum.
    // Everything else keeps the generic stream bit for bit: other matrices, non-finite values, the knob at 0, and any
    // call the row-value kernels do not serve (the one-row-per-load kernels, a narrow plan at a wide width), for
    // which the device expands this stream back into the generic one once (spmm_sweep.hip).
    bool row_values = false;
    std::vector<uint32_t> entries32;           // row_values: n_entries packed words
    std::vector<float> task_vals;              // row_values: n_tasks x kRW
    std::vector<SweepSplitRow> split_rows;
};

uint32_t sweep_lanes_per_entry(uint32_t d_hint);                    // 4 / 8 / 12 / 16 float4 lanes per gathered row
uint32_t sweep_panel_rows(uint32_t d_hint, bool hot_columns);       // rows of B per column panel
// false: the matrix is not worth sweeping (tiny, unless force) or does not fit the packed entry.  num_cu = compute
// units of the device the plan is for (a launch round = the resident set: num_cu x blocks per CU x 4 waves).
bool sweep_build_host(uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr, const uint32_t *indices, const float *values,
                      uint32_t max_d, bool force, uint32_t d_hint, bool hot_columns, uint32_t num_cu, SweepHost &out);
// what the rounds of a plan lose to their longest task: sum_rounds max(end - beg) / sum_rounds mean(end - beg) - 1 over
// chunks of round_tasks tasks (0 = every launch ends together)
double round_excess(const SweepHost &plan);
// every row's stored values share one finite bit pattern (threaded, read-only)
bool rows_have_one_value(uint32_t n_rows, const uint32_t *indptr, const float *values);

// ---- passes of mggcn_spmm_plan_create_for over the whole matrix ----------------------------------
// every column index < n_cols?  (one threaded read-only pass on behalf of the calling thread, which reports)
bool columns_in_range(uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr, const uint32_t *indices);

struct ColumnStats {
    double hot_share = 0.0;     // share of the non-zeros in the 1 % most popular columns
    double locality = 0.0;      // share of the non-zeros whose column lies in the same 1/32 of the index space as their row
    bool hot_columns = true;
};
ColumnStats column_stats(uint32_t n_rows, uint32_t n_cols, const uint32_t *indptr, const uint32_t *indices);

// fixed pseudo-random relabelling of the columns: pi[c] = new label of column c, src_row[pi[c]] = c
void column_permutation(uint32_t n_cols, std::vector<uint32_t> &pi, std::vector<uint32_t> &src_row);
// out[e] = pi[indices[e]], indexed like `indices` (the offset indptr[0] kept)
void permute_indices(uint32_t n_rows, const uint32_t *indptr, const uint32_t *indices, const std::vector<uint32_t> &pi,
                     std::vector<uint32_t> &out);

// the non-zeros bucketed by column slice of `width` columns: slice k = CSR (ips[k], ixs[k], vvs[k]) over all rows,
// row order and the order inside a row kept
struct SliceBuckets {
    std::vector<std::vector<uint32_t>> ips, ixs;
    std::vector<std::vector<float>> vvs;
};
SliceBuckets slice_buckets(uint32_t n_rows, uint32_t S, uint32_t width, const uint32_t *indptr, const uint32_t *indices,
                           const float *values);

// ---- shared knobs ------------------------------------------------------------------------------
uint32_t env_u32(const char *name, uint32_t dflt);
// threads of a host pass: MGGCN_HOST_THREADS, else the cores of the machine divided by the number of plan builders
// running side by side (set_concurrent_builders; csr_matrix::prebuild_plans runs up to four), capped at `cap`
unsigned host_threads(unsigned cap);
void set_concurrent_builders(unsigned n);
// compute units' worth of wave slots the launch rounds of plans built FROM NOW ON leave free (see sweep_build_host)
void set_reserved_cus(unsigned n);

}  // namespace mggcn_plan
