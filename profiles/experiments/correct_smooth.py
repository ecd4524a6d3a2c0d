"""What Correct and Smooth costs, on the Reddit-shaped stand-in (synth_reddit_like(1.0, seed=1)) with its
values sym_normalize'd, C = 41, L1 = L2 = 50, alpha = 0.8, on the protocol of profiles/experiments/label_input.py:
  * the whole call cs(ctx, logits, Y, S) -- residual, 50 + 50 iterations, the scale kernel -- by device events and by the
    host's wall clock around call + synchronisation;
  * its own timers: cs-residual, cs-correct, cs-scale, cs-smooth, and cs-spmm / cs-step of the last iteration;
  * per call: the three row kernels; the step against what existing ops can assemble of it (scale_mat + axpy: two passes,
    axpby: one; neither clamps -- there is no clamp among them);
  * the loop with and without its steps (50 products alone against 50 products + 50 steps): the share of the steps;
  * one product at d = 41 by this matrix against the same call by the matrix the gcn's logits layer multiplies by (the
    README's d = 41 figure: column-normalised, transposed), in the same run.
Device events after a warm-up, medians of SAMPLES samples, the sides of a comparison taking turns.  A manual script, not a
test; not to be run under a profiler.
Usage: python profiles/experiments/correct_smooth.py"""
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
L, ALPHA = 50, 0.8


def sample(fn):
    ctx.record("exp-begin", 0)
    fn()
    ctx.record("exp-end", 0)
    ctx.sync()
    return float(lib.mggcn_event_elapsed_ms(ctx.events["exp-begin"], ctx.events["exp-end"]))


def alternate(sides):
    for fn in sides.values():                        # warm-up: code objects, caches, scratch, plans
        sample(fn)
    got = {name: [] for name in sides}
    for _ in range(SAMPLES):
        for name, fn in sides.items():
            got[name].append(sample(fn))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in got.items()}


def show(tag, res):
    for name, (med, lo, hi) in res.items():
        print(f"[{tag}] {name:34s} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
    return {name: med for name, (med, _, _) in res.items()}


(ip, ix, dv), _, Yh = pkg.datasets.synth_reddit_like(1.0, seed=1)
n = ip.shape[0] - 1
C = 1 + int(Yh.max())
A = pkg.csr_matrix(ip, ix, pkg.datasets.sym_normalize(ip, ix, dv), n)
rng = np.random.default_rng(2)
S = rng.choice(3, size=n, p=(0.66, 0.10, 0.24)).astype(np.int32)                   # Reddit's split, roughly
Y = Yh.reshape(-1).astype(np.int32)
onehot = np.zeros((n, C), dtype=np.float32)
onehot[np.arange(n), Y] = 2.0
logits = dn.from_numpy(onehot + 1.5 * rng.standard_normal((n, C), dtype=np.float32))
del onehot
print(f"[graph] n {n}, nnz {A.nnz()}, classes {C}, training rows {int((S == 0).sum())}; L1 = L2 = {L}, alpha = {ALPHA}", flush=True)

cs = pkg.correct_and_smooth(A, C, L, ALPHA, L, ALPHA)
Yd, Sd = dn.from_numpy(Y.reshape(-1, 1)), dn.from_numpy(S.reshape(-1, 1))
whole = show("whole", alternate({"cs(ctx, logits, Y, S)": lambda: cs(ctx, logits, Yd, Sd)}))
wall = []
for _ in range(SAMPLES):
    ctx.sync()
    t0 = time.perf_counter()
    cs(ctx, logits, Yd, Sd)
    ctx.sync()
    wall.append(1e3 * (time.perf_counter() - t0))
print(f"[whole] host wall clock, call + sync        {statistics.median(wall):9.3f} ms (min {min(wall):.3f}, max {max(wall):.3f})", flush=True)
timers = {}
for _ in range(SAMPLES):
    cs(ctx, logits, Yd, Sd)
    ctx.sync()
    for name in ("cs-residual", "cs-correct", "cs-scale", "cs-smooth", "cs-spmm", "cs-step"):
        timers.setdefault(name, []).append(ctx.measure(name))
for name, v in timers.items():
    print(f"[timers] {name:12s} {statistics.median(v):9.3f} ms (min {min(v):.3f}, max {max(v):.3f})", flush=True)

# ---- per call ---------------------------------------------------------------------------------------------------------------------
inv_T = float(np.float32(1.0 / int((S == 0).sum())))
beta = 1.0 - ALPHA
T, R, T2 = cs.X1, cs.E0, cs.X2
flags = ops.CS_AUTOSCALE | ops.CS_SET_LABELS
calls = show(f"{n} x {C}", alternate({
    "cs_residual": lambda: ops.cs_residual(ctx, logits, Yd, Sd, 0, cs.P, cs.E0, cs.sums),
    "cs_correct (autoscale + labels)": lambda: ops.cs_correct(ctx, cs.P, cs.X1, Yd, Sd, 0, cs.sums, inv_T, 1.0, flags, out=cs.G0),
    "cs_step clamp(-1, 1)": lambda: ops.cs_step(ctx, T, R, None, ALPHA, beta, -1.0, 1.0),
    "cs_step fix, no clamp": lambda: ops.cs_step(ctx, T, R, Sd, ALPHA, beta, -float("inf"), float("inf"), 0, ops.CS_FIX_TRAIN),
    "scale_mat + axpy (no clamp)": lambda: (ops.scale_mat(ctx, T2, ALPHA), ops.axpy(ctx, R, T2, beta)),
    "axpby (no clamp)": lambda: ops.axpby(ctx, R, T2, beta, ALPHA),
}))

# ---- the loop with and without its steps ---------------------------------------------------------------------------------
plan = ops.spmm_plan_for(ctx, A, C, C)


def products(with_step):
    X = cs.E0
    for i in range(L):
        out = (cs.X1, cs.X2)[i % 2]
        ops.matmul(ctx, A, X, out, plan, 1.0, 0.0)
        if with_step:
            ops.cs_step(ctx, out, cs.E0, None, ALPHA, beta, -1.0, 1.0)
        X = out


ops.cs_residual(ctx, logits, Yd, Sd, 0, cs.P, cs.E0, cs.sums)
loop = show(f"loop of {L}", alternate({"products + steps": lambda: products(True), "products alone": lambda: products(False)}))
both, alone = loop["products + steps"], loop["products alone"]
print(f"[loop of {L}] the steps' share {100.0 * (both - alone) / both:.1f} % of the loop; per iteration "
      f"{both / L:.4f} ms = product {alone / L:.4f} + step {(both - alone) / L:.4f}", flush=True)

# ---- one product at d = 41: this matrix against the gcn's ----------------------------------------------------------------
M = pkg.csr_matrix(ip, ix, dv.copy(), n)
M.normalize(True)
M_T = M.transpose()                                   # what the gcn's forward multiplies by (gcn.hpp:946-955)
plan_T = ops.spmm_plan_for(ctx, M_T, C, C)
B, Cm = cs.P, cs.X2
show(f"SpMM d = {C}", alternate({
    "sym_normalize'd A (this loop's)": lambda: ops.matmul(ctx, A, B, Cm, plan, 1.0, 0.0),
    "gcn's forward matrix (README's)": lambda: ops.matmul(ctx, M_T, B, Cm, plan_T, 1.0, 0.0),
}))
print(f"[plans] this loop's: {plan.num_launches(C)} launches per call; the gcn's: {plan_T.num_launches(C)}", flush=True)
