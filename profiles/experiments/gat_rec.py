"""Is the packed destination record faster than three scalar gathers?  
mggcn_gat_backward_src_f32 (s_dst, lse, D as three [n x heads] arrays: the kernel as it was) beside
mggcn_gat_backward_src_rec_f32 (one 16-byte record per (destination, heads)) in one process, over F^T of the Reddit-shaped
stand-in (synth_reddit_like(1.0, seed=1)), at the two layer shapes of the epoch [608, 128, 128, 128, 41]: 128 columns with 4
heads and 41 columns with 1 head.  The protocol of gat.py: device events after a warm-up, medians of SAMPLES samples, the
sides taking turns; the pack itself is timed too, and both sides' outputs are compared as bits.  A manual script, not a
test; not to be run under a profiler.
Usage: python profiles/experiments/gat_rec.py"""
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
    for fn in sides.values():                        # warm-up: code objects, caches
        sample(fn)
    got = {name: [] for name in sides}
    for _ in range(SAMPLES):
        for name, fn in sides.items():
            got[name].append(sample(fn))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in got.items()}


import torch

(ip, ix, dv), _, _ = pkg.datasets.synth_reddit_like(1.0, seed=1)
n = ip.shape[0] - 1
A = pkg.csr_matrix(ip, ix, dv.copy(), n)             # F^T: what backward_src walks
F = A.transpose()
print(f"[graph] n {n}, nnz {A.nnz()}, longest row of F^T {np.diff(A.indptr.astype(np.int64)).max()}", flush=True)

for D, K in ((128, 4), (41, 1)):
    rng = np.random.default_rng(D)
    Z, G = (dn.from_numpy(rng.standard_normal((n, D), dtype=np.float32)) for _ in range(2))
    att = dn.from_numpy((0.1 * rng.standard_normal((2, D))).astype(np.float32))
    out = dn(n, D)
    s_dst, s_src, lse, Dm, ds_dst = (dn(n, K) for _ in range(5))
    ops.gat_scores(ctx, Z, att, s_dst, s_src, K)
    ops.gat_forward(ctx, F, Z, s_dst, s_src, out, lse, K)
    ops.gat_backward_dst(ctx, F, Z, s_dst, s_src, lse, G, out, Dm, ds_dst, K)
    rec = torch.empty(n * K * 4, dtype=torch.float32, device=ctx.device)
    ops.gat_pack_dst(ctx, s_dst, lse, Dm, rec)
    ctx.sync()
    outs = {name: (dn(n, K), dn(n, D)) for name in ("plain", "record")}
    sides = {
        "plain": lambda: ops.gat_backward_src(ctx, A, Z, s_dst, s_src, lse, Dm, G, att, ds_dst, *outs["plain"], K),
        "record": lambda: ops.gat_backward_src_rec(ctx, A, Z, rec, s_src, G, att, ds_dst, *outs["record"], K),
    }
    for turn, order in enumerate((("plain", "record"), ("record", "plain"))):       # either side first
        res = alternate({name: sides[name] for name in order})
        for name in ("plain", "record"):
            med, lo, hi = res[name]
            print(f"[{n} x {D}, heads {K}] turn {turn} backward_src {name:6s} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
        print(f"[{n} x {D}, heads {K}] turn {turn} record / plain = {res['record'][0] / res['plain'][0]:.4f}", flush=True)
    med, lo, hi = alternate({"pack": lambda: ops.gat_pack_dst(ctx, s_dst, lse, Dm, rec)})["pack"]
    print(f"[{n} x {D}, heads {K}] pack_dst {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
    same = all(torch.equal(a.t.view(torch.int32), b.t.view(torch.int32)) for a, b in zip(outs["plain"], outs["record"]))
    print(f"[{n} x {D}, heads {K}] ds_src and G_Z bit-equal: {same}", flush=True)
    assert same
    del Z, G, out, outs, rec
