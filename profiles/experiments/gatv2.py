"""What GATv2 costs next to GAT, on the Reddit-shaped stand-in (synth_reddit_like(1.0, seed=1)), on the
protocol of profiles/experiments/gat.py:
  * per call at d = 128 with 4 heads (float4 path, LPR = 8) and at d = 41 with 1 head (element path, LPR = 64): the three
    sparse GATv2 calls and att_grad next to the GAT calls of the same tree -- gatv2_forward and gatv2_backward_dst against
    gat_backward_dst (the v1 kernel with the same gather plus a dot product), gatv2_backward_src against gat_backward_src;
  * one epoch of gat([608, 128, 128, 128, 41], heads=4) of both variants in the same process.
Device events after a warm-up, medians of SAMPLES samples, the sides of a comparison taking turns.  A manual script, not a
test; not to be run under a profiler.
Usage: python profiles/experiments/gatv2.py [--no-epoch]"""
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
SAMPLES = 7


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
print(f"[graph] n {n}, nnz {F.nnz()}, longest row of F {np.diff(F.indptr.astype(np.int64)).max()}, "
      f"of F^T {np.diff(A.indptr.astype(np.int64)).max()}", flush=True)

for D, K in ((128, 4), (41, 1)):
    rng = np.random.default_rng(0)
    Z2 = dn.from_numpy(rng.standard_normal((n, 2 * D), dtype=np.float32))         # the model's layout: [Zs | Zd]
    Z, G = (dn.from_numpy(rng.standard_normal((n, D), dtype=np.float32)) for _ in range(2))
    att1 = dn.from_numpy((0.1 * rng.standard_normal((2, D))).astype(np.float32))
    att2 = dn.from_numpy((0.1 * rng.standard_normal((1, D))).astype(np.float32))
    out, G_Z, out2, P, G_Z2 = dn(n, D), dn(n, D), dn(n, D), dn(n, D), dn(n, 2 * D)
    s_dst, s_src, lse, Dm, ds_dst, ds_src, lse2, Dm2 = (dn(n, K) for _ in range(8))
    G_att1, G_att2 = dn(2, D), dn(1, D)
    ops.gat_scores(ctx, Z, att1, s_dst, s_src, K)
    ops.gat_forward(ctx, F, Z, s_dst, s_src, out, lse, K)
    ops.gat_backward_dst(ctx, F, Z, s_dst, s_src, lse, G, out, Dm, ds_dst, K)
    ops.gatv2_forward(ctx, F, Z2, Z2, att2, out2, lse2, K)
    ops.gatv2_backward_dst(ctx, F, Z2, Z2, att2, lse2, G, out2, Dm2, G_Z2, P, K)
    ctx.sync()
    res = alternate({
        "gat_forward (F)": lambda: ops.gat_forward(ctx, F, Z, s_dst, s_src, out, lse, K),
        "gatv2_forward (F)": lambda: ops.gatv2_forward(ctx, F, Z2, Z2, att2, out2, lse2, K),
        "gat_backward_dst (F)": lambda: ops.gat_backward_dst(ctx, F, Z, s_dst, s_src, lse, G, out, Dm, ds_dst, K),
        "gatv2_backward_dst (F)": lambda: ops.gatv2_backward_dst(ctx, F, Z2, Z2, att2, lse2, G, out2, Dm2, G_Z2, P, K),
        "gat_backward_src (F^T)": lambda: ops.gat_backward_src(ctx, A, Z, s_dst, s_src, lse, Dm, G, att1, ds_dst, ds_src, G_Z, K),
        "gatv2_backward_src (F^T)": lambda: ops.gatv2_backward_src(ctx, A, Z2, Z2, att2, lse2, Dm2, G, G_Z2, K),
        "gat_scores": lambda: ops.gat_scores(ctx, Z, att1, s_dst, s_src, K),
        "gat_scores_backward": lambda: ops.gat_scores_backward(ctx, ds_dst, Z, ds_src, Z, G_att1, K),
        "gatv2_att_grad": lambda: ops.gatv2_att_grad(ctx, P, G_att2),
    })
    for name, (med, lo, hi) in res.items():
        print(f"[{n} x {D}, heads {K}] {name:26s} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
    for a, b in (("gatv2_forward (F)", "gat_backward_dst (F)"), ("gatv2_forward (F)", "gat_forward (F)"),
                 ("gatv2_backward_dst (F)", "gat_backward_dst (F)"), ("gatv2_backward_src (F^T)", "gat_backward_src (F^T)")):
        print(f"[ratio, d = {D}] {a} / {b} = {res[a][0] / res[b][0]:.2f}", flush=True)
    del Z2, Z, G, out, G_Z, out2, P, G_Z2

if "--no-epoch" not in sys.argv:
    sizes = [Xh.shape[1], 128, 128, 128, 1 + int(Yh.max())]
    models = {"gat v1": pkg.gat(A, sizes, heads=4), "gat v2": pkg.gat(A, sizes, heads=4, variant="v2")}
    Xd, Yd = dn.from_numpy(Xh), dn.from_numpy(Yh)
    res = alternate({name: (lambda M_=M_: M_.train_step(ctx, Xd, Yd, 1e-2, 0.9, 0.999, 5e-4, 1e-8)) for name, M_ in models.items()})
    for name, (med, lo, hi) in res.items():
        print(f"[epoch {sizes}] {name:6s} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
    text = io.StringIO()
    ctx.dump_timers(text, "")
    print("\n".join(ln for ln in text.getvalue().splitlines() if "gat" in ln), flush=True)
