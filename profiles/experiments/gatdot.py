"""What dot-product attention costs next to GATv2, on the Reddit-shaped stand-in
(synth_reddit_like(1.0, seed=1)), on the protocol of profiles/experiments/gatv2.py:
  * per call at d = 128 with 4 heads (float4 path, LPR = 8) and at d = 41 with 1 head (element path, LPR = 64): the three
    sparse gatdot calls next to the three sparse GATv2 calls of the same tree, each on the model's layout (the thirds of one
    [n x 3 d] buffer, the halves of one [n x 2 d] buffer).  The forward gathers two head-rows per entry where GATv2's gathers
    one, backward_dst two against one, backward_src two as GATv2's does;
  * one epoch of gat([608, 128, 128, 128, 41], heads=4) of both variants in the same process.
Device events after a warm-up, medians of SAMPLES samples, the sides of a comparison taking turns.  A manual script, not a
test; not to be run under a profiler.
Usage: python profiles/experiments/gatdot.py [--no-epoch]"""
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
    Z2 = dn.from_numpy(rng.standard_normal((n, 2 * D), dtype=np.float32))         # GATv2's layout: [Zs | Zd]
    Z3 = dn.from_numpy(rng.standard_normal((n, 3 * D), dtype=np.float32))         # the dot model's: [Zq | Zk | Zv]
    G = dn.from_numpy(rng.standard_normal((n, D), dtype=np.float32))
    att2 = dn.from_numpy((0.1 * rng.standard_normal((1, D))).astype(np.float32))
    out2, P, G_Z2, out3, G_Z3 = dn(n, D), dn(n, D), dn(n, 2 * D), dn(n, D), dn(n, 3 * D)
    lse2, Dm2, lse3, Dm3 = (dn(n, K) for _ in range(4))
    ops.gatv2_forward(ctx, F, Z2, Z2, att2, out2, lse2, K)
    ops.gatv2_backward_dst(ctx, F, Z2, Z2, att2, lse2, G, out2, Dm2, G_Z2, P, K)
    ops.gatdot_forward(ctx, F, Z3, Z3, Z3, out3, lse3, K)
    ops.gatdot_backward_dst(ctx, F, Z3, Z3, Z3, lse3, G, out3, Dm3, G_Z3, K)
    ctx.sync()
    res = alternate({
        "gatv2_forward (F)": lambda: ops.gatv2_forward(ctx, F, Z2, Z2, att2, out2, lse2, K),
        "gatdot_forward (F)": lambda: ops.gatdot_forward(ctx, F, Z3, Z3, Z3, out3, lse3, K),
        "gatv2_backward_dst (F)": lambda: ops.gatv2_backward_dst(ctx, F, Z2, Z2, att2, lse2, G, out2, Dm2, G_Z2, P, K),
        "gatdot_backward_dst (F)": lambda: ops.gatdot_backward_dst(ctx, F, Z3, Z3, Z3, lse3, G, out3, Dm3, G_Z3, K),
        "gatv2_backward_src (F^T)": lambda: ops.gatv2_backward_src(ctx, A, Z2, Z2, att2, lse2, Dm2, G, G_Z2, K),
        "gatdot_backward_src (F^T)": lambda: ops.gatdot_backward_src(ctx, A, Z3, Z3, Z3, lse3, Dm3, G, G_Z3, G_Z3, K),
    })
    for name, (med, lo, hi) in res.items():
        print(f"[{n} x {D}, heads {K}] {name:26s} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
    for call in ("forward (F)", "backward_dst (F)", "backward_src (F^T)"):
        print(f"[ratio, d = {D}] gatdot_{call} / gatv2_{call} = {res['gatdot_' + call][0] / res['gatv2_' + call][0]:.2f}", flush=True)
    del Z2, Z3, G, out2, P, G_Z2, out3, G_Z3

if "--no-epoch" not in sys.argv:
    sizes = [Xh.shape[1], 128, 128, 128, 1 + int(Yh.max())]
    models = {"gat v2": pkg.gat(A, sizes, heads=4, variant="v2"), "gat dot": pkg.gat(A, sizes, heads=4, variant="dot")}
    Xd, Yd = dn.from_numpy(Xh), dn.from_numpy(Yh)
    res = alternate({name: (lambda M_=M_: M_.train_step(ctx, Xd, Yd, 1e-2, 0.9, 0.999, 5e-4, 1e-8)) for name, M_ in models.items()})
    for name, (med, lo, hi) in res.items():
        print(f"[epoch {sizes}] {name:7s} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
    text = io.StringIO()
    ctx.dump_timers(text, "")
    print("\n".join(ln for ln in text.getvalue().splitlines() if "gat" in ln or "matmul" in ln), flush=True)
