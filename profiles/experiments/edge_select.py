"""What the exact fan-out costs, on the Reddit-shaped stand-in (synth_reddit_like(1.0, seed=1)), with the
protocol of profiles/experiments/edge_sample.py:
  * the select: mggcn_edge_sample_select_u32 over F (rows are destinations) at k = 10 and k = 25 for every R the library is
    built for, next to mggcn_edge_sample_count_u32 over F from the same run (both draw every word of F once); the streaming
    path on the same matrix (force_stream), and on F^T used as if it were a forward matrix (a hub row of ~21 000 entries),
    there also with the hub's row cut out so that its share of the launch is on record;
  * the whole draw and the epoch of [608, 128, 128, 128, 41], exact against expected in the same run: gat v1 (4 heads),
    sage(aggr="max") and gcn(edge_rescale="row") at fanout 10, gat v1 at fanout 25, with the kept fraction of each.
Device events after a warm-up, medians of SAMPLES samples.  A manual script, not a test; not to be run under a profiler.
Usage: python profiles/experiments/edge_select.py [--no-epochs]"""
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
es = sys.modules[pkg.__name__ + ".edge_sample"]
SAMPLES = 7
ADAM = (1e-2, 0.9, 0.999, 5e-4, 1e-8)
FULL = 0xFFFFFFFF


def sample(fn):
    ctx.record("exp-begin", 0)
    fn()
    ctx.record("exp-end", 0)
    ctx.sync()
    return float(lib.mggcn_event_elapsed_ms(ctx.events["exp-begin"], ctx.events["exp-end"]))


def timed(fn):
    sample(fn)                                                   # warm-up: code objects, caches
    v = [sample(fn) for _ in range(SAMPLES)]
    return statistics.median(v), min(v), max(v)


t0 = time.time()
(ip, ix, dv), Xh, Yh = pkg.datasets.synth_reddit_like(1.0, seed=1)
n = ip.shape[0] - 1
A = pkg.csr_matrix(ip, ix, dv.copy(), n)
F = A.transpose()
deg, deg_t = np.diff(F.indptr.astype(np.int64)), np.diff(A.indptr.astype(np.int64))
print(f"[graph] n {n}, nnz {F.nnz()}; rows of F: mean {deg.mean():.0f}, longest {deg.max()}; rows of F^T: longest {deg_t.max()} "
      f"(row {int(deg_t.argmax())}); built in {time.time() - t0:.1f} s on the host", flush=True)

# ---- the select -------------------------------------------------------------------------------------------------------------
import torch
thr = torch.empty(n, dtype=torch.int32, device=ctx.device)
counts = torch.empty(n, dtype=torch.int32, device=ctx.device)
fp, fx, _ = F.device(ctx.device)
tp, tx, _ = A.device(ctx.device)
hub = int(deg_t.argmax())
for k in (10, 25):
    thr_k = torch.from_numpy(es.thresholds(F.indptr, k, 1.0).view(np.int32)).to(ctx.device)
    count, lo, hi = timed(lambda: ops.edge_sample_count(ctx, n, fp, fx, thr_k, 0, counts, seed=7, epoch=0))
    print(f"[select k={k}] F   count (expected fan-out)      {count:8.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
    want = None
    for R in ops.EDGE_SELECT_RS:
        med, lo, hi = timed(lambda: ops.edge_sample_select(ctx, n, fp, fx, k, FULL, thr, seed=7, epoch=0, regs=R))
        got = thr.cpu().numpy()
        want = got if want is None else want
        assert (got == want).all()
        path = "registers" if deg.max() <= 64 * R else f"registers / streaming ({int((deg > 64 * R).sum())} rows stream)"
        print(f"[select k={k}] F   select R={R:2d} {path:22s} {med:8.3f} ms (min {lo:.3f}, max {hi:.3f}) = {med / count:.2f} of count",
              flush=True)
    med, lo, hi = timed(lambda: ops.edge_sample_select(ctx, n, fp, fx, k, FULL, thr, seed=7, epoch=0, force_stream=True))
    assert (thr.cpu().numpy() == want).all()
    print(f"[select k={k}] F   select force_stream           {med:8.3f} ms (min {lo:.3f}, max {hi:.3f}) = {med / count:.2f} of count", flush=True)
    med, lo, hi = timed(lambda: ops.edge_sample_select(ctx, n, tp, tx, k, FULL, thr, seed=7, epoch=0))
    print(f"[select k={k}] F^T as a forward matrix            {med:8.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
    one, lo, hi = timed(lambda: ops.edge_sample_select(ctx, 1, tp[hub:], tx, k, FULL, thr, row0=hub, seed=7, epoch=0))
    print(f"[select k={k}] F^T, the hub's row alone ({deg_t[hub]} entries) {one:8.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
    def all_but_the_hub():
        ops.edge_sample_select(ctx, hub, tp, tx, k, FULL, thr, seed=7, epoch=0)
        ops.edge_sample_select(ctx, n - hub - 1, tp[hub + 1:], tx, k, FULL, thr[hub + 1:], row0=hub + 1, seed=7, epoch=0)
    rest, lo, hi = timed(all_but_the_hub)
    print(f"[select k={k}] F^T, every row but the hub's (two calls)  {rest:8.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
del thr, counts
if "--no-epochs" in sys.argv:
    sys.exit(0)

# ---- the draw and the epoch: exact against expected ---------------------------------------------------------------------------
sizes = [Xh.shape[1], 128, 128, 128, 1 + int(Yh.max())]
Xd, Yd = dn.from_numpy(Xh), dn.from_numpy(Yh)
MODELS = [('gat(variant="v1")', lambda: pkg.gat(A, sizes, heads=4), (10, 25)),
          ('sage(aggr="max")', lambda: pkg.sage(A, sizes, aggr="max"), (10,)),
          ('gcn(edge_rescale="row")', lambda: pkg.gcn(A, sizes, edge_rescale="row"), (10,))]
for name, make, fanouts in MODELS:
    M = make()
    step = lambda: M.train_step(ctx, Xd, Yd, *ADAM)
    for fanout in fanouts:
        for exact in (False, True, False):                       # the second "expected" shows the drift of the run
            M.set_sampling(fanout=fanout, seed=7, exact=exact)
            med, lo, hi = timed(step)
            kept = M.sampler.pair[0].nnz()
            timers = [t for t in ("sample-select", "sample-count", "sample-scan", "sample-compact", "sample-plan") if t in ctx.timers
                      and (exact or t != "sample-select")]
            draw = {t: ctx.measure(t) for t in timers}
            print(f"[epoch {sizes}] {name:24s} fanout {fanout:2d} {'exact   ' if exact else 'expected'} {med:9.3f} ms (min {lo:.3f}, "
                  f"max {hi:.3f}); kept {kept} ({100.0 * kept / F.nnz():.2f} %); draw {sum(draw.values()):.3f} ms: "
                  + ", ".join(f"{t[7:]} {v:.3f}" for t, v in draw.items()), flush=True)
    del M
