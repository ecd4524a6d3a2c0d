"""What edge sampling with values costs and buys, on the Reddit-shaped stand-in (synth_reddit_like(1.0,
seed=1)), with the protocol of profiles/experiments/edge_sample.py:
  * the draw with values: rowscale / count, scan, compact_val and the device plan build per matrix (F = A.transpose(), rows
    are destinations; F^T = A) and edge_sampler.draw as a whole, for fanout 10, fanout 25 and keep 0.5, with the kept entries
    and the plan's item / slot / split-row totals next to each;
  * ops.spmm_dev (row-split on the device-built plan) against the sweep SpMM on the same matrix at FULL keep (fanout 10**6:
    every entry kept, every factor 1), at 128 and 41 columns, forward and transposed;
  * the epoch [608, 128, 128, 128, 41] of gcn and sage(aggr="mean"): off, then fanout 10, fanout 25 and keep 0.5, for both
    rescale modes, and off again (the drift of the run), every setting after a warm-up epoch of its own.
Device events after a warm-up, medians of SAMPLES samples.  A manual script, not a test; not to be run under a profiler.
Usage: python profiles/experiments/edge_sample_spmm.py [--kinds gcn,sage]"""
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
KINDS = sys.argv[sys.argv.index("--kinds") + 1].split(",") if "--kinds" in sys.argv else ["gcn", "sage"]
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
A.normalize(True)
F = A.transpose()
print(f"[graph] n {n}, nnz {F.nnz()} ({F.nnz() / n:.0f} per destination), built in {time.time() - t0:.1f} s on the host", flush=True)

# ---- the draw with values ----------------------------------------------------------------------------------------------------
for label, kw in SETTINGS:
    sampler = es.edge_sampler(F, A, rescale="row", max_d=128, **kw)
    t0 = time.time()
    pair = sampler.draw(ctx, 7, 0)                               # allocates, uploads the thresholds, sizes the two plans
    ctx.sync()
    kept = pair[0].nnz()
    assert kept == pair[1].nnz()
    print(f"[draw {label}] kept {kept} of {F.nnz()} ({100.0 * kept / F.nnz():.1f} %); first draw incl. allocation and the host "
          f"capacity pass {time.time() - t0:.2f} s; plans {sum(p.nbytes() for p in sampler.plans) / 1e6:.0f} MB", flush=True)
    thr, scale = sampler._thr, sampler._scale
    for t, (M, (counts, indptr, indices, values)) in enumerate(zip((F, A), sampler._bufs)):
        mp, mx, mv = M.device(ctx.device)
        side = "F^T" if t else "F  "
        plan = sampler.plans[t]
        first = (("rowscale", lambda: ops.edge_sample_rowscale(ctx, n, mp, mx, mv, thr, counts, scale, seed=7, epoch=0)) if t == 0
                 else ("count", lambda: ops.edge_sample_count(ctx, n, mp, mx, thr, t, counts, seed=7, epoch=0)))
        for name, fn in (first, ("scan", lambda: ops.edge_sample_scan(ctx, counts, n, indptr)),
                         ("compact_val", lambda: ops.edge_sample_compact_val(ctx, n, mp, mx, mv, thr, t, scale, True, indptr, indices,
                                                                             values, seed=7, epoch=0)),
                         ("plan build", lambda: ops.spmm_dev_plan_build(ctx, plan, indptr))):
            med, lo, hi = timed(fn)
            print(f"[draw {label}] {side} {name:11s} {med:8.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
        totals = plan.read()[2]
        print(f"[draw {label}] {side} plan: items {int(totals[0])} of {plan.cap_items}, slots {int(totals[1])} of {plan.cap_slots}, "
              f"split rows {int(totals[2])} of {plan.cap_split}", flush=True)
    med, lo, hi = timed(lambda: sampler.draw(ctx, 7, 0))
    print(f"[draw {label}] whole draw     {med:8.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
    del sampler, pair, thr, scale, plan

# ---- spmm_dev against the sweep SpMM at full keep --------------------------------------------------------------------------------
sampler = es.edge_sampler(F, A, fanout=10 ** 6, rescale="row", max_d=128)
pair = sampler.draw(ctx, 7, 0)
rng = np.random.default_rng(0)
for d in (128, 41):
    B, C, C2 = dn.from_numpy(rng.standard_normal((n, d)).astype(np.float32)), dn(n, d), dn(n, d)
    for side, M, S in (("F  ", F, pair[0]), ("F^T", A, pair[1])):
        buf = ops.get_matmul_buffer(ctx, M, B, C, max_d=128)
        sweep = timed(lambda: ops.matmul(ctx, M, B, C, buf, 1.0, 0.0))
        dev = timed(lambda: ops.spmm_dev(ctx, S, B, C2, S.plan, 1.0, 0.0))
        err = float(np.abs(C.numpy() - C2.numpy()).max() / np.abs(C.numpy()).max())
        print(f"[spmm full keep] {side} d {d:3d}: sweep {sweep[0]:7.3f} ms (min {sweep[1]:.3f}, max {sweep[2]:.3f}), spmm_dev "
              f"{dev[0]:7.3f} ms (min {dev[1]:.3f}, max {dev[2]:.3f}) = {dev[0] / sweep[0]:.2f} x; max difference {err:.1e} of the "
              f"largest entry; the host plan is the {'sweep' if buf.num_sweep_tasks() else 'row-split'} form", flush=True)
del sampler, pair

# ---- the epochs -------------------------------------------------------------------------------------------------------------
sizes = [Xh.shape[1], 128, 128, 128, 1 + int(Yh.max())]
Xd, Yd = dn.from_numpy(Xh), dn.from_numpy(Yh)
TIMERS = ("sample-count", "sample-scan", "sample-compact", "sample-plan")
for kind in KINDS:
    t0 = time.time()
    A2 = pkg.csr_matrix(ip, ix, dv.copy(), n)
    M, name = (pkg.gcn(A2, sizes), "gcn") if kind == "gcn" else (pkg.sage(A2, sizes, aggr="mean"), 'sage(aggr="mean")')
    print(f"[model {name}] built in {time.time() - t0:.1f} s on the host", flush=True)
    step = lambda: M.train_step(ctx, Xd, Yd, *ADAM)
    base = None
    runs = [("off", None, dict())] + [(f"{label} {mode}", mode, kw) for mode in ("row", "inverse") for label, kw in SETTINGS]
    for label, mode, kw in runs + [("off again", None, dict())]:
        M.set_sampling(seed=7, rescale=mode, **kw)
        med, lo, hi = timed(step)
        kept = M.sampler.pair[0].nnz() if M.sampler is not None else F.nnz()
        base = med if base is None else base
        draw = sum(ctx.measure(t) for t in TIMERS) if M.sampler is not None else 0.0
        print(f"[epoch {sizes}] {name:18s} {label:18s} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f}) = {med / base:.3f} of off; "
              f"kept {kept} ({100.0 * kept / F.nnz():.1f} %); the draw's four timers {draw:.3f} ms", flush=True)
    del M, A2
