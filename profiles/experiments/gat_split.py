"""What does cutting long rows buy the GAT kernels?  
The three plain calls beside their _split twins (ops.gat_*_split over ops.gat_split_plan) in one process, each walking F and
then F^T of the Reddit-shaped stand-in (synth_reddit_like(1.0, seed=1); longest row 607 / 21 657 entries, the same entry
count), at the two layer shapes of the epoch [608, 128, 128, 128, 41] -- 128 columns with 4 heads, 41 columns with 1 head --
for split in 512, 1024, 2048, 4096, with each plan's bytes and host build time; then the 4-head epoch with and without
row_split.  The protocol of gat.py: device events after a warm-up, medians of SAMPLES samples, the sides taking turns.  The
merge has no entry point of its own and is inside the split call's time.  A manual script, not a test; not to be run under
a profiler.
Usage: python profiles/experiments/gat_split.py"""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import __graft_entry__ as g

pkg = g.load_package()
ctx = pkg.context(0)
lib, ops, dn = ctx.lib, pkg.ops, pkg.dn_matrix
SAMPLES = 7
SPLITS = (512, 1024, 2048, 4096)


def sample(fn):
    ctx.record("exp-begin", 0)
    fn()
    ctx.record("exp-end", 0)
    ctx.sync()
    return float(lib.mggcn_event_elapsed_ms(ctx.events["exp-begin"], ctx.events["exp-end"]))


def alternate(sides):
    for fn in sides.values():                        # warm-up: code objects, caches
        sample(fn)
    got = {name: [] for name in sides}
    for _ in range(SAMPLES):
        for name, fn in sides.items():
            got[name].append(sample(fn))
    return {name: statistics.median(v) for name, v in got.items()}


(ip, ix, dv), X, Y = pkg.datasets.synth_reddit_like(1.0, seed=1)
n = ip.shape[0] - 1
A = pkg.csr_matrix(ip, ix, dv.copy(), n)
mats = {"F": A.transpose(), "F^T": A}
for name, M in mats.items():
    print(f"[graph] {name}: n {n}, nnz {M.nnz()}, longest row {np.diff(M.indptr.astype(np.int64)).max()}", flush=True)

for D, K in ((128, 4), (41, 1)):
    rng = np.random.default_rng(D)
    Z, G = (dn.from_numpy(rng.standard_normal((n, D), dtype=np.float32)) for _ in range(2))
    att = dn.from_numpy((0.1 * rng.standard_normal((2, D))).astype(np.float32))
    out, G_Z = dn(n, D), dn(n, D)
    s_dst, s_src, lse, Dm, ds_dst, ds_src = (dn(n, K) for _ in range(6))
    ops.gat_scores(ctx, Z, att, s_dst, s_src, K)
    for name, M in mats.items():
        calls = {
            "forward": lambda *p: getattr(ops, "gat_forward" + ("_split" if p else ""))(ctx, M, Z, s_dst, s_src, out, lse, K, *p),
            "backward_dst": lambda *p: getattr(ops, "gat_backward_dst" + ("_split" if p else ""))(
                ctx, M, Z, s_dst, s_src, lse, G, out, Dm, ds_dst, K, *p),
            "backward_src": lambda *p: getattr(ops, "gat_backward_src" + ("_split" if p else ""))(
                ctx, M, Z, s_dst, s_src, lse, Dm, G, att, ds_dst, ds_src, G_Z, K, *p),
        }
        for split in SPLITS:
            t0 = time.perf_counter()
            plan = ops.gat_split_plan(ctx, M, split, K, D)
            build = time.perf_counter() - t0
            print(f"[{name} {D}/{K}] split {split}: {plan.num_items()} items, {plan.num_split_rows()} split rows, "
                  f"{plan.num_slots()} slots, {plan.nbytes() / 2**20:.2f} MiB, built in {build * 1e3:.1f} ms", flush=True)
            for call, fn in calls.items():           # forward first: the two backward calls read its lse and out
                res = alternate({"plain": fn, "split": lambda: fn(plan)})
                print(f"[{name} {D}/{K}] split {split} {call:12s} plain {res['plain']:8.3f} ms  split {res['split']:8.3f} ms  "
                      f"split / plain = {res['split'] / res['plain']:.3f}", flush=True)
    del Z, G, out, G_Z

sizes = [608, 128, 128, 128, 41]
Xd, Yd = dn.from_numpy(X), dn.from_numpy(Y.reshape(-1, 1).astype(np.int32))
for split in (None, 1024, None, 1024):
    model = pkg.gat(pkg.csr_matrix(ip, ix, dv.copy(), n), sizes, heads=4, row_split=split)
    times = []
    for _ in range(2 + SAMPLES):
        ctx.sync()
        t0 = time.perf_counter()
        model.train_step(ctx, Xd, Yd, 1e-2, 0.9, 0.999, 5e-4, 1e-8)
        ctx.sync()
        times.append((time.perf_counter() - t0) * 1e3)
    print(f"[epoch {sizes} heads 4] row_split {split}: {statistics.median(times[2:]):.1f} ms "
          f"(min {min(times[2:]):.1f}, max {max(times[2:]):.1f})", flush=True)
    del model
