"""What the export of the attention coefficients costs, on the Reddit-shaped stand-in
(synth_reddit_like(1.0, seed=1)), on the protocol of profiles/experiments/gat.py: per call at d = 128 with 4 heads and at
d = 41 with 1 head, gat_alpha and gatv2_alpha next to gat_forward and gatv2_forward of the same process, and the time the
bytes alone would take at 6.3 TB/s (the HBM rate DESIGN.md prices streamed bytes at): nnz (4 + 4 K) B of index reads and alpha
writes, plus for v2 the gather of Zs, nnz K dh 4 B.  Device events after a warm-up, medians of SAMPLES samples, the sides
taking turns.  A manual script, not a test; not to be run under a profiler.
Usage: python profiles/experiments/gat_alpha.py"""
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
HBM = 6.3e12


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
    return {name: (statistics.median(v), min(v), max(v)) for name, v in got.items()}


(ip, ix, dv), _, _ = pkg.datasets.synth_reddit_like(1.0, seed=1)
n = ip.shape[0] - 1
F = pkg.csr_matrix(ip, ix, dv.copy(), n).transpose()
nnz = F.nnz()
print(f"[graph] n {n}, nnz {nnz}, longest row of F {np.diff(F.indptr.astype(np.int64)).max()}", flush=True)

for D, K in ((128, 4), (41, 1)):
    rng = np.random.default_rng(0)
    Z2 = dn.from_numpy(rng.standard_normal((n, 2 * D), dtype=np.float32))         # the model's layout: [Zs | Zd]
    Z = dn.from_numpy(rng.standard_normal((n, D), dtype=np.float32))
    att1 = dn.from_numpy((0.1 * rng.standard_normal((2, D))).astype(np.float32))
    att2 = dn.from_numpy((0.1 * rng.standard_normal((1, D))).astype(np.float32))
    out, out2 = dn(n, D), dn(n, D)
    s_dst, s_src, lse, lse2 = (dn(n, K) for _ in range(4))
    alpha = dn(nnz, K)                                                            # 1.84 GB at K = 4
    ops.gat_scores(ctx, Z, att1, s_dst, s_src, K)
    ops.gat_forward(ctx, F, Z, s_dst, s_src, out, lse, K)
    ops.gatv2_forward(ctx, F, Z2, Z2, att2, out2, lse2, K)
    ctx.sync()
    res = alternate({
        "gat_forward": lambda: ops.gat_forward(ctx, F, Z, s_dst, s_src, out, lse, K),
        "gat_alpha": lambda: ops.gat_alpha(ctx, F, s_dst, s_src, lse, alpha, K),
        "gatv2_forward": lambda: ops.gatv2_forward(ctx, F, Z2, Z2, att2, out2, lse2, K),
        "gatv2_alpha": lambda: ops.gatv2_alpha(ctx, F, Z2, Z2, att2, lse2, alpha, K),
    })
    own = nnz * (4 + 4 * K)
    bytes_ = {"gat_alpha": own, "gatv2_alpha": own + nnz * D * 4}
    for name, (med, lo, hi) in res.items():
        tail = ""
        if name in bytes_:
            ms = bytes_[name] / HBM * 1e3
            tail = f"  bytes alone {bytes_[name] / 1e9:.2f} GB = {ms:.3f} ms at 6.3 TB/s ({med / ms:.1f} x)"
        print(f"[{n} x {D}, heads {K}] {name:14s} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f}){tail}", flush=True)
    for a, b in (("gat_alpha", "gat_forward"), ("gatv2_alpha", "gatv2_forward")):
        print(f"[ratio, d = {D}] {a} / {b} = {res[a][0] / res[b][0]:.2f}", flush=True)
    del Z2, Z, out, out2, alpha
