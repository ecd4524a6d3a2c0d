#!/usr/bin/env python3
"""Which sweep tasks share a launch round, on the full-size Reddit stand-in -- CPU only, no device.

Builds tests/native/round_order_test.cpp against csrc/plan_host.cpp, writes the stand-in's adjacency (the backward-type
matrix: power-law rows) and its transpose (the forward-type matrix: even rows, hot columns) as CSR files and lets the
driver build their sweep plans for a 256-CU device with MGGCN_SPMM_SORT_ROUNDS = 0 and = 1: padded task lengths per
round, round_excess and the builder's seconds.  Wide form: two column slices of 131 072; narrow form: d_hint 41, one slice.

  python3 profiles/experiments/round_order.py [scale]      > profiles/experiments/round_order.log
"""
import importlib.util
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def load_datasets():
    spec = importlib.util.spec_from_file_location("mggcn_datasets", os.path.join(ROOT, "mg-gcn_amd", "datasets.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def transpose(indptr, indices, data, n):
    order = np.argsort(indices, kind="stable")
    t_indptr = np.zeros(n + 1, dtype=np.uint32)
    t_indptr[1:] = np.cumsum(np.bincount(indices, minlength=n))
    rows = np.repeat(np.arange(n, dtype=np.uint32), np.diff(indptr).astype(np.int64))
    return t_indptr, rows[order], data[order]


def write_csr(path, indptr, indices, data, n):
    with open(path, "wb") as f:
        np.array([n, n, len(indices)], dtype=np.uint32).tofile(f)
        np.asarray(indptr, dtype=np.uint32).tofile(f)
        np.asarray(indices, dtype=np.uint32).tofile(f)
        np.asarray(data, dtype=np.float32).tofile(f)


def main():
    scale = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "round_order_test")
        csrc = os.path.join(ROOT, "mg-gcn_amd", "csrc")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-I", csrc, os.path.join(ROOT, "tests", "native", "round_order_test.cpp"),
                               os.path.join(csrc, "plan_host.cpp"), "-o", exe])
        (indptr, indices, data), _, _ = load_datasets().synth_reddit_like(scale, seed=1)
        n = len(indptr) - 1
        mats = {"backward": (indptr, indices, data), "forward": transpose(indptr, indices, data, n)}
        for name, (ip, ix, dv) in mats.items():
            path = os.path.join(tmp, name + ".csr")
            write_csr(path, ip, ix, dv, n)
            for form, width, d_hint in (("wide", 131072, 0), ("narrow", 0, 41)):
                print(f"== {name} matrix, {form} form (slice width {width}, d_hint {d_hint}), 256 CUs", flush=True)
                subprocess.check_call([exe, "--file", path, "256", str(width), str(d_hint)])
            os.remove(path)


if __name__ == "__main__":
    main()
