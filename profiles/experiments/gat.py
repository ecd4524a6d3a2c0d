"""What graph attention costs, on the Reddit-shaped stand-in (synth_reddit_like(1.0, seed=1)):
  * per call at d = 128, heads 4: mggcn_gat_forward_f32 and the two backward gathers (mggcn_gat_backward_dst_f32 over F,
    mggcn_gat_backward_src_f32 over F^T), each beside mggcn_spmm_csr_f32 with plan = NULL on the same matrix at the same
    width -- the same one-wave-per-row gather, so the ratio prices the softmax and the per-edge dot products;
  * one epoch of gat([608, 128, 128, 128, 41], heads=4) beside one epoch of gcn on the same sizes in the same process.
Device events after a warm-up, medians of SAMPLES samples, the sides of a comparison taking turns.  A manual script, not a
test; not to be run under a profiler.
Usage: python profiles/experiments/gat.py [--no-epoch]"""
import io
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import __graft_entry__ as g

pkg = g.load_package()
ctx = pkg.context(0)
lib, ops, dn = ctx.lib, pkg.ops, pkg.dn_matrix
SAMPLES, K, D = 7, 4, 128


def sample(fn):
    ctx.record("exp-begin", 0)
    fn()
    ctx.record("exp-end", 0)
    ctx.sync()
    return float(lib.mggcn_event_elapsed_ms(ctx.events["exp-begin"], ctx.events["exp-end"]))


def alternate(sides):
    for fn in sides.values():                        # warm-up: code objects, caches, scratch
        sample(fn)
    got = {name: [] for name in sides}
    for _ in range(SAMPLES):
        for name, fn in sides.items():
            got[name].append(sample(fn))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in got.items()}


(ip, ix, dv), Xh, Yh = pkg.datasets.synth_reddit_like(1.0, seed=1)
n = ip.shape[0] - 1
A = pkg.csr_matrix(ip, ix, dv.copy(), n)
F = A.transpose()
deg = np.diff(F.indptr.astype(np.int64))
print(f"[graph] n {n}, nnz {F.nnz()}, longest row of F {deg.max()}, of F^T {np.diff(A.indptr.astype(np.int64)).max()}", flush=True)

rng = np.random.default_rng(0)
Z, G = (dn.from_numpy(rng.standard_normal((n, D), dtype=np.float32)) for _ in range(2))
att = dn.from_numpy((0.1 * rng.standard_normal((2, D))).astype(np.float32))
out, G_Z, C = dn(n, D), dn(n, D), dn(n, D)
s_dst, s_src, lse, Dm, ds_dst, ds_src = (dn(n, K) for _ in range(6))
G_att = dn(2, D)
ops.gat_scores(ctx, Z, att, s_dst, s_src, K)
ops.gat_forward(ctx, F, Z, s_dst, s_src, out, lse, K)
ops.gat_backward_dst(ctx, F, Z, s_dst, s_src, lse, G, out, Dm, ds_dst, K)
ctx.sync()
out_t, lse_t, D_t, ds_t = dn(n, D), dn(n, K), dn(n, K), dn(n, K)      # outputs of the runs on the other matrix
res = alternate({
    "gat_forward (F)": lambda: ops.gat_forward(ctx, F, Z, s_dst, s_src, out, lse, K),
    "spmm plan=NULL (F)": lambda: ops.matmul(ctx, F, Z, C, None, 1.0, 0.0),
    "gat_backward_dst (F)": lambda: ops.gat_backward_dst(ctx, F, Z, s_dst, s_src, lse, G, out, Dm, ds_dst, K),
    "gat_backward_src (F^T)": lambda: ops.gat_backward_src(ctx, A, Z, s_dst, s_src, lse, Dm, G, att, ds_dst, ds_src, G_Z, K),
    "spmm plan=NULL (F^T)": lambda: ops.matmul(ctx, A, G, C, None, 1.0, 0.0),
    # the same kernels on the other matrix: F's longest row has a few hundred entries, F^T's ~21 k, the entry count is the
    # same -- the difference is what the heavy rows cost (a consistent forward / backward over A's pattern: F is ITS transpose)
    "gat_forward (F^T)": lambda: ops.gat_forward(ctx, A, Z, s_dst, s_src, out_t, lse_t, K),
    "gat_backward_dst (F^T)": lambda: ops.gat_backward_dst(ctx, A, Z, s_dst, s_src, lse_t, G, out_t, D_t, ds_t, K),
    "gat_backward_src (F)": lambda: ops.gat_backward_src(ctx, F, Z, s_dst, s_src, lse_t, D_t, G, att, ds_t, ds_src, G_Z, K),
    "gat_scores": lambda: ops.gat_scores(ctx, Z, att, s_dst, s_src, K),
    "gat_scores_backward": lambda: ops.gat_scores_backward(ctx, ds_dst, Z, ds_src, Z, G_att, K),
})
for name, (med, lo, hi) in res.items():
    print(f"[{n} x {D}, heads {K}] {name:24s} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
for a, b in (("gat_forward (F)", "spmm plan=NULL (F)"), ("gat_backward_dst (F)", "spmm plan=NULL (F)"),
             ("gat_backward_src (F^T)", "spmm plan=NULL (F^T)")):
    print(f"[ratio] {a} / {b} = {res[a][0] / res[b][0]:.2f}", flush=True)
del Z, G, out, out_t, G_Z, C

if "--no-epoch" not in sys.argv:
    sizes = [Xh.shape[1], 128, 128, 128, 1 + int(Yh.max())]
    models = {"gcn": pkg.gcn(pkg.csr_matrix(ip, ix, dv.copy(), n), sizes), "gat": pkg.gat(A, sizes, heads=K)}
    Xd, Yd = dn.from_numpy(Xh), dn.from_numpy(Yh)
    res = alternate({name: (lambda M_=M_: M_.train_step(ctx, Xd, Yd, 1e-2, 0.9, 0.999, 5e-4, 1e-8)) for name, M_ in models.items()})
    for name, (med, lo, hi) in res.items():
        print(f"[epoch {sizes}] {name:4s} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
    text = io.StringIO()
    ctx.dump_timers(text, "")
    print("\n".join(ln for ln in text.getvalue().splitlines() if "gat-" in ln), flush=True)
