#!/usr/bin/env python3
"""Per-launch durations of the sweep kernels from two rocprofv3 --kernel-trace runs of bench.py, one with
MGGCN_SPMM_SORT_ROUNDS=0 and one with 1: the launches of ONE forward-matrix and ONE backward-matrix SpMM call of the last
epoch in each trace, and the mean over all epochs.  A call is a sequence of launches of one kernel (wide: two column slices
of four rounds; narrow: four rounds); the backward matrix has sliced rows, so a sweep_combine_kernel follows its slices.

  python3 profiles/experiments/round_order_launches.py <knob0 kernel_trace.csv> <knob1 kernel_trace.csv>   (markdown on stdout)
"""
import csv
import sys

KERNELS = {"spmm_sweep_pair_kernel<true>": ("d = 128 (pair kernel)", 4), "spmm_sweep_quad_lds_kernel<16>": ("d = 41 (narrow kernel)", 4)}


def slices(path):
    """[(kernel, backward?, [durations in us of the rounds of one slice])] in launch order"""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0] for r in rows]
    out, i = [], 0
    while i < len(rows):
        k = names[i]
        if k not in KERNELS:
            i += 1
            continue
        n = KERNELS[k][1]
        dur = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows[i:i + n]]
        assert names[i:i + n] == [k] * n, (i, names[i:i + n])
        backward = i + n < len(rows) and names[i + n] == "sweep_combine_kernel"
        out.append((k, backward, dur))
        i += n
    return out


def table(path):
    sl = slices(path)
    text = []
    for k, (label, _) in KERNELS.items():
        for backward in (False, True):
            mine = [d for kk, b, d in sl if kk == k and b == backward]
            per_call = 2 if "pair" in k else 1                       # slices per call
            last = mine[-per_call:]
            mean = [sum(d[r] for d in mine) / len(mine) for r in range(len(mine[0]))]
            text.append(f"| {label}, {'backward' if backward else 'forward'} matrix | " +
                        " / ".join(" ".join(f"{x:.0f}" for x in d) for d in last) + f" | {sum(map(sum, last)):.0f} | " +
                        " ".join(f"{x:.0f}" for x in mean) + f" | {sum(mean) * per_call:.0f} |")
    return text


def main():
    for knob, path in enumerate(sys.argv[1:3]):
        print(f"\n## Launch durations, MGGCN_SPMM_SORT_ROUNDS={knob} (us; rounds in launch order, slices separated by /)\n")
        print("| call | launches of the last call in the trace | sum | mean per round over all calls (slices pooled) | mean call |")
        print("|---|---|---|---|---|")
        print("\n".join(table(path)))


if __name__ == "__main__":
    main()
