"""What per-epoch edge sampling costs and buys, on the Reddit-shaped stand-in (synth_reddit_like(1.0, seed=1)),
with the protocol of profiles/experiments/gat.py:
  * the draw: mggcn_edge_sample_count_u32 / _scan_u32 / _compact_u32 per matrix (F = A.transpose(), rows are destinations;
    F^T = A, the threshold gathered per entry) and edge_sampler.draw as a whole, for fanout 10, fanout 25 and keep 0.5, with
    the kept entries next to each;
  * the epoch of gat([608, 128, 128, 128, 41], heads=4) as v1, v2 and dot and of sage(aggr="max") on the same sizes, one model
    per kind, under: off, fanout 10, fanout 25, keep 0.5 and off again (the second "off" shows the drift of the run), every
    setting after a warm-up epoch of its own (which also pays the upload of the thresholds), with the kept entries of the
    last epoch next to each.
The comparison of the DEFAULT model against the parent commit is profiles/experiments/gat_efeat.py --default-epoch LABEL and
bench.py --gpus 1 --steps 10 --warmup 3, each run from a built checkout of either commit, taking turns.
Device events after a warm-up, medians of SAMPLES samples.  A manual script, not a test; not to be run under a profiler.
Usage: python profiles/experiments/edge_sample.py [--kinds v1,v2,dot,sage]"""
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
SETTINGS = [("fanout 10", dict(fanout=10, keep=1.0)), ("fanout 25", dict(fanout=25, keep=1.0)), ("keep 0.5", dict(fanout=None, keep=0.5))]
KINDS = sys.argv[sys.argv.index("--kinds") + 1].split(",") if "--kinds" in sys.argv else ["v1", "v2", "dot", "sage"]
ADAM = (1e-2, 0.9, 0.999, 5e-4, 1e-8)


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
print(f"[graph] n {n}, nnz {F.nnz()} ({F.nnz() / n:.0f} per destination), built in {time.time() - t0:.1f} s on the host", flush=True)

# ---- the draw ---------------------------------------------------------------------------------------------------------------
for label, kw in SETTINGS:
    sampler = es.edge_sampler(F, A, **kw)
    pair = sampler.draw(ctx, 7, 0)                               # allocates, uploads the thresholds
    kept = pair[0].nnz()
    assert kept == pair[1].nnz()
    q = sampler.thr_host.astype(np.float64) / 2.0 ** 32
    deg = np.diff(F.indptr.astype(np.int64))
    print(f"[draw {label}] kept {kept} of {F.nnz()} ({100.0 * kept / F.nnz():.1f} %), expected without self-loops "
          f"{float((q * deg).sum()):.0f}", flush=True)
    thr = sampler._thr
    for t, (M, (counts, indptr, indices)) in enumerate(zip((F, A), sampler._bufs)):
        mp, mx, _ = M.device(ctx.device)
        side = "F^T" if t else "F  "
        for name, fn in (("count", lambda: ops.edge_sample_count(ctx, n, mp, mx, thr, t, counts, seed=7, epoch=0)),
                         ("scan", lambda: ops.edge_sample_scan(ctx, counts, n, indptr)),
                         ("compact", lambda: ops.edge_sample_compact(ctx, n, mp, mx, thr, t, indptr, indices, seed=7, epoch=0))):
            med, lo, hi = timed(fn)
            print(f"[draw {label}] {side} {name:8s} {med:8.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
    med, lo, hi = timed(lambda: sampler.draw(ctx, 7, 0))
    read = 2 * 2 * 4 * F.nnz() + 4 * F.nnz()                    # both passes read both index arrays; F^T's gathers a threshold per entry
    print(f"[draw {label}] whole draw   {med:8.3f} ms (min {lo:.3f}, max {hi:.3f}); reads {read / 1e9:.2f} GB of indices and "
          f"thresholds, writes {2 * 4 * kept / 1e9:.2f} GB: {(read + 2 * 4 * kept) / med / 1e6:.0f} GB/s", flush=True)
    del sampler, pair, thr

# ---- the epochs -------------------------------------------------------------------------------------------------------------
sizes = [Xh.shape[1], 128, 128, 128, 1 + int(Yh.max())]
Xd, Yd = dn.from_numpy(Xh), dn.from_numpy(Yh)
for kind in KINDS:
    t0 = time.time()
    if kind == "sage":
        M, name = pkg.sage(A, sizes, aggr="max"), 'sage(aggr="max")'
    else:
        M, name = pkg.gat(A, sizes, heads=4, variant=kind), f'gat(variant="{kind}")'
    print(f"[model {name}] built in {time.time() - t0:.1f} s on the host", flush=True)
    step = lambda: M.train_step(ctx, Xd, Yd, *ADAM)
    base = None
    for label, kw in [("off", dict())] + SETTINGS + [("off again", dict())]:
        M.set_sampling(seed=7, **kw)
        med, lo, hi = timed(step)
        kept = M.sampler.pair[0].nnz() if M.sampler is not None else F.nnz()
        base = med if base is None else base
        draw = sum(ctx.measure(t) for t in ("sample-count", "sample-scan", "sample-compact")) if M.sampler is not None else 0.0
        print(f"[epoch {sizes}] {name:18s} {label:10s} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f}) = {med / base:.3f} of off; "
              f"kept {kept} ({100.0 * kept / F.nnz():.1f} %); the draw's three timers {draw:.3f} ms", flush=True)
    del M
