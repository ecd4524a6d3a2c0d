"""What attention dropout costs, on the Reddit-shaped stand-in (synth_reddit_like(1.0, seed=1)), with the
protocol of profiles/experiments/gat.py:
  * per call at d = 128, heads 4: mggcn_gat_forward_drop_f32, mggcn_gat_backward_dst_drop_f32 (over F) and
    mggcn_gat_backward_src_drop_f32 (over F^T) at p = 0.6, each beside its plain twin in the same process -- the plain
    entry points launch the DROP = false kernels, which are the kernels as they were before the flag;
  * one epoch of gat([608, 128, 128, 128, 41], heads=4) with (dropout, attn_dropout) = (0.6, 0.6), (0, 0.6), (0.6, 0) and
    (0, 0), the models taking turns, and the per-layer timers of one epoch with and without attention dropout.
Device events after a warm-up, medians of SAMPLES samples, the sides of a comparison taking turns.  A manual script, not a
test; not to be run under a profiler.
Usage: python profiles/experiments/gat_dropout.py [--no-epoch]"""
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
SAMPLES, K, D, P = 7, 4, 128, 0.6


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
print(f"[graph] n {n}, nnz {F.nnz()}", flush=True)

rng = np.random.default_rng(0)
Z, G = (dn.from_numpy(rng.standard_normal((n, D), dtype=np.float32)) for _ in range(2))
att = dn.from_numpy((0.1 * rng.standard_normal((2, D))).astype(np.float32))
out, G_Z = dn(n, D), dn(n, D)
s_dst, s_src, lse, Dm, ds_dst, ds_src = (dn(n, K) for _ in range(6))
drop = (*ops.dropout_params(P), 0x5EED, 3, 0, 0)
ops.gat_scores(ctx, Z, att, s_dst, s_src, K)
ops.gat_forward(ctx, F, Z, s_dst, s_src, out, lse, K)
ops.gat_backward_dst(ctx, F, Z, s_dst, s_src, lse, G, out, Dm, ds_dst, K)
ctx.sync()
res = alternate({
    "gat_forward": lambda: ops.gat_forward(ctx, F, Z, s_dst, s_src, out, lse, K),
    "gat_forward_drop": lambda: ops.gat_forward(ctx, F, Z, s_dst, s_src, out, lse, K, drop=drop),
    "gat_backward_dst": lambda: ops.gat_backward_dst(ctx, F, Z, s_dst, s_src, lse, G, out, Dm, ds_dst, K),
    "gat_backward_dst_drop": lambda: ops.gat_backward_dst(ctx, F, Z, s_dst, s_src, lse, G, out, Dm, ds_dst, K, drop=drop),
    "gat_backward_src": lambda: ops.gat_backward_src(ctx, A, Z, s_dst, s_src, lse, Dm, G, att, ds_dst, ds_src, G_Z, K),
    "gat_backward_src_drop": lambda: ops.gat_backward_src(ctx, A, Z, s_dst, s_src, lse, Dm, G, att, ds_dst, ds_src, G_Z, K, drop=drop),
})
for name, (med, lo, hi) in res.items():
    print(f"[{n} x {D}, heads {K}, p {P}] {name:24s} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
for a in ("gat_forward", "gat_backward_dst", "gat_backward_src"):
    extra = res[a + "_drop"][0] - res[a][0]
    print(f"[ratio] {a}_drop / {a} = {res[a + '_drop'][0] / res[a][0]:.3f}  (+{extra:.3f} ms = "
          f"{1e9 * extra / (F.nnz() * K):.2f} ps per (entry, head))", flush=True)
del Z, G, out, G_Z

if "--no-epoch" not in sys.argv:
    sizes = [Xh.shape[1], 128, 128, 128, 1 + int(Yh.max())]
    models = {f"gat({pd}, {pa})": pkg.gat(A, sizes, heads=K, dropout=pd, attn_dropout=pa)
              for pd, pa in ((0.0, 0.0), (P, P), (0.0, P), (P, 0.0))}
    Xd, Yd = dn.from_numpy(Xh), dn.from_numpy(Yh)
    res = alternate({name: (lambda M_=M_: M_.train_step(ctx, Xd, Yd, 1e-2, 0.9, 0.999, 5e-4, 1e-8)) for name, M_ in models.items()})
    for name, (med, lo, hi) in res.items():
        print(f"[epoch {sizes}] {name:14s} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
    for name in ("gat(0.0, 0.0)", f"gat(0.0, {P})"):      # where the epoch's difference sits: the model's own timers, one epoch each
        models[name].train_step(ctx, Xd, Yd, 1e-2, 0.9, 0.999, 5e-4, 1e-8)
        text = io.StringIO()
        ctx.dump_timers(text, "")
        print(f"[timers {name}] " + "  ".join(ln for ln in text.getvalue().splitlines() if "gat-" in ln and "scores" not in ln), flush=True)
