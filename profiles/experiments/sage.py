"""What GraphSAGE costs, on the Reddit-shaped stand-in (synth_reddit_like(1.0, seed=1)), on the protocol of
profiles/experiments/correct_smooth.py:
  * per call at d = 128 and d = 41, in one run: mggcn_agg_max_forward_f32 (with and without arg) and
    mggcn_agg_max_backward_f32 next to mggcn_spmm_csr_f32 (the mean aggregator: gcn's forward matrix and its backward matrix)
    and to mggcn_gat_forward_f32 / mggcn_gat_backward_src_f32 with one head, over the same patterns;
  * the epoch [608, 128, 128, 128, 41] of sage(aggr="mean") and sage(aggr="max") next to gcn's (gcn.py is what it was
    before sage existed), train_step by the host's wall clock around call + synchronisation.
Device events after a warm-up, medians of SAMPLES samples, the sides of a comparison taking turns.  A manual script, not a
test; not to be run under a profiler.
Usage: python profiles/experiments/sage.py"""
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
SIZES = [608, 128, 128, 128, 41]
ADAM = (1e-2, 0.9, 0.999, 5e-4, 1e-8)


def sample(fn):
    ctx.record("exp-begin", 0)
    fn()
    ctx.record("exp-end", 0)
    ctx.sync()
    return float(lib.mggcn_event_elapsed_ms(ctx.events["exp-begin"], ctx.events["exp-end"]))


def alternate(sides, samples=SAMPLES):
    for fn in sides.values():                        # warm-up: code objects, caches, scratch, plans
        sample(fn)
    got = {name: [] for name in sides}
    for _ in range(samples):
        for name, fn in sides.items():
            got[name].append(sample(fn))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in got.items()}


def show(tag, res):
    for name, (med, lo, hi) in res.items():
        print(f"[{tag}] {name:40s} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)


(ip, ix, dv), Xh, Yh = pkg.datasets.synth_reddit_like(1.0, seed=1)
n = ip.shape[0] - 1
A = pkg.csr_matrix(ip, ix, dv.copy(), n)
A.normalize(True)
F = A.transpose()                                     # what every forward walks: row i lists the sources of destination i
F_T = F.transpose()                                   # the row-sorted pattern of A: what every backward walks
lens, t_lens = np.diff(F.indptr.astype(np.int64)), np.diff(F_T.indptr.astype(np.int64))
print(f"[graph] n {n}, nnz {A.nnz()}; rows of F: median {int(np.median(lens))}, max {int(lens.max())}; rows of F^T: median "
      f"{int(np.median(t_lens))}, max {int(t_lens.max())}", flush=True)

rng = np.random.default_rng(3)
for d in (128, 41):
    B = dn.from_numpy(rng.standard_normal((n, d), dtype=np.float32))
    G = dn.from_numpy(rng.standard_normal((n, d), dtype=np.float32))
    out, G_B = dn(n, d), dn(n, d)
    arg = dn(n, d, dtype=np.int32)
    att = dn.from_numpy(0.1 * rng.standard_normal((2, d), dtype=np.float32))
    s_dst, s_src, lse, D, ds_dst, ds_src = (dn(n, 1) for _ in range(6))
    plan, plan_T = ops.spmm_plan_for(ctx, F, max(d, 128), d), ops.spmm_plan_for(ctx, F_T, max(d, 128), d)
    ops.gat_scores(ctx, B, att, s_dst, s_src, 1)
    ops.gat_forward(ctx, F, B, s_dst, s_src, out, lse, 1)
    ops.gat_backward_dst(ctx, F, B, s_dst, s_src, lse, G, out, D, ds_dst, 1)
    ops.agg_max_forward(ctx, F, B, out, arg)
    show(f"d = {d}", alternate({
        "agg_max_forward (out and arg)": lambda: ops.agg_max_forward(ctx, F, B, out, arg),
        "agg_max_forward (arg = NULL)": lambda: ops.agg_max_forward(ctx, F, B, out),
        "spmm_csr, forward matrix": lambda: ops.matmul(ctx, F, B, out, plan, 1.0, 0.0),
        "gat_forward, one head": lambda: ops.gat_forward(ctx, F, B, s_dst, s_src, out, lse, 1),
        "agg_max_backward": lambda: ops.agg_max_backward(ctx, F_T, arg, G, G_B),
        "agg_max_backward, accumulate": lambda: ops.agg_max_backward(ctx, F_T, arg, G, G_B, accumulate=True),
        "spmm_csr, backward matrix": lambda: ops.matmul(ctx, F_T, G, G_B, plan_T, 1.0, 0.0),
        "gat_backward_src, one head": lambda: ops.gat_backward_src(ctx, F_T, B, s_dst, s_src, lse, D, G, att, ds_dst, ds_src,
                                                                    G_B, 1),
    }))
    gathered = A.nnz() * d * 4
    print(f"[d = {d}] bytes gathered per call: forward {gathered / 1e9:.2f} GB (B rows), backward {2 * gathered / 1e9:.2f} GB "
          f"(arg and G rows)", flush=True)
    del B, G, out, G_B, arg

# ---- the epoch ---------------------------------------------------------------------------------------------------------------------
X, Y = dn.from_numpy(Xh), dn.from_numpy(Yh.reshape(-1, 1).astype(np.int32))


def epochs(name, model):
    for _ in range(2):
        model.train_step(ctx, X, Y, *ADAM)
    wall = []
    for _ in range(SAMPLES):
        ctx.sync()
        t0 = time.perf_counter()
        loss, acc = model.train_step(ctx, X, Y, *ADAM)
        wall.append(1e3 * (time.perf_counter() - t0))
    print(f"[epoch {SIZES}] {name:24s} {statistics.median(wall):9.3f} ms (min {min(wall):.3f}, max {max(wall):.3f}); "
          f"loss {loss:.4f}", flush=True)


for name, make in (("gcn", lambda M: pkg.gcn(M, SIZES)), ("sage(aggr='mean')", lambda M: pkg.sage(M, SIZES, aggr="mean")),
                   ("sage(aggr='max')", lambda M: pkg.sage(M, SIZES, aggr="max"))):
    model = make(pkg.csr_matrix(ip, ix, dv.copy(), n))
    epochs(name, model)
    if name != "gcn":
        held = sum(t.n() * t.m() * 4 for layer in model.layers() for t in (layer.M, layer.Y, layer.G_out, layer.agg.arg
                                                                            if hasattr(layer.agg, "arg") else None) if t is not None)
        print(f"[memory] {name}: M, Y, G_out and arg of all layers {held / 2 ** 20:.0f} MiB", flush=True)
    del model
