"""What masked label inputs cost, on the Reddit-shaped stand-in (synth_reddit_like(1.0, seed=1)), on the
protocol of profiles/experiments/gat_skip.py:
  * per call, at the width of layer 0's Z of every variant (128 / 256 / 384 columns): mggcn_label_input_forward_f32 and
    mggcn_label_input_backward_f32 over the training rows (two thirds of the vertices, 41 classes), at rate 0.5 and with
    feed_all;
  * the host's count of one epoch's fed rows (label_mask.fed_count over the training rows), wall clock;
  * one epoch of gat([608, 128, 128, 128, 41], heads=4) of every variant, default against label_input=0.5, in the same
    process: device events, and for the label-input model the host's wall clock of train_step too -- the count of the next
    epoch runs between the last launch and the synchronisation, and hides when the wall clock stays at the device time.
Device events after a warm-up, medians of SAMPLES samples, the sides of a comparison taking turns.  A manual script, not a
test; not to be run under a profiler.
Usage: python profiles/experiments/label_input.py [--no-epoch | --default-only]
--default-only times the default models alone (run it on two checkouts to compare a change against its parent)."""
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
DEFAULT_ONLY = "--default-only" in sys.argv


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
C = 1 + int(Yh.max())
S = np.random.default_rng(2).choice(3, size=n, p=(0.66, 0.10, 0.24)).astype(np.int32)      # Reddit's split, roughly
T = int((S == 0).sum())
print(f"[graph] n {n}, nnz {A.nnz()}, classes {C}, training rows {T}", flush=True)

if not DEFAULT_ONLY:
    from importlib import import_module
    gat, lm = import_module(pkg.__name__ + ".gat"), import_module(pkg.__name__ + ".label_mask")
    rows, cls, ptr = gat.label_lists(S, Yh, 0, C)
    rd, cd, pd = (dn.from_numpy(a.reshape(-1, 1)) for a in (rows, cls, ptr))
    thr = lm.threshold(0.5)
    rng = np.random.default_rng(0)
    for width in (128, 256, 384):
        Z, G = dn.from_numpy(rng.standard_normal((n, width), dtype=np.float32)), dn.from_numpy(rng.standard_normal((n, width), dtype=np.float32))
        E, G_E, S_e = dn.from_numpy(rng.standard_normal((C, width), dtype=np.float32)), dn(C, width), dn.from_numpy(S.reshape(-1, 1))
        res = alternate({
            "forward  rate 0.5": lambda: ops.label_input_forward(ctx, rd, cd, E, Z, thr, False, 1, 0, 0, 0, 3, S_e),
            "forward  feed_all": lambda: ops.label_input_forward(ctx, rd, cd, E, Z, 0, True, 0, 0, 0, 0, 3, None),
            "backward rate 0.5": lambda: ops.label_input_backward(ctx, rd, cd, pd, G, G_E, thr, False, 1, 0, 0),
            "backward feed_all": lambda: ops.label_input_backward(ctx, rd, cd, pd, G, G_E, 0, True, 0, 0, 0),
        })
        for name, (med, lo, hi) in res.items():
            print(f"[{T} of {n} x {width}] label_input {name:18s} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
        del Z, G, E, G_E
    glob = np.sort(rows).astype(np.uint64)
    lm.fed_count(glob, thr, 1, 0)
    t = []
    for e in range(SAMPLES):
        t0 = time.perf_counter()
        lm.fed_count(glob, thr, 1, e)
        t.append(1e3 * (time.perf_counter() - t0))
    print(f"[host] label_mask.fed_count over {T} rows {statistics.median(t):9.3f} ms (min {min(t):.3f}, max {max(t):.3f})", flush=True)

if "--no-epoch" not in sys.argv:
    sizes = [Xh.shape[1], 128, 128, 128, C]
    Xd, Yd = dn.from_numpy(Xh), dn.from_numpy(Yh)
    step = lambda M: M.train_step(ctx, Xd, Yd, 1e-2, 0.9, 0.999, 5e-4, 1e-8)
    for variant in ("v1", "v2", "dot"):
        models = {f"{variant} default": pkg.gat(A, sizes, heads=4, variant=variant)}
        models[f"{variant} default"].set_splits(S)
        if not DEFAULT_ONLY:
            M = pkg.gat(A, sizes, heads=4, variant=variant, label_input=0.5)
            M.set_splits(S)
            M.set_label_input(Yd, seed=1)
            models[f"{variant} label 0.5"] = M
        res = alternate({name: (lambda M_=M_: step(M_)) for name, M_ in models.items()})
        for name, (med, lo, hi) in res.items():
            print(f"[epoch {sizes}] {name:16s} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
        if not DEFAULT_ONLY:
            wall = []
            for _ in range(SAMPLES):
                ctx.sync()
                t0 = time.perf_counter()
                step(M)
                wall.append(1e3 * (time.perf_counter() - t0))
            print(f"[epoch {sizes}] {variant} label 0.5 host wall clock {statistics.median(wall):9.3f} ms "
                  f"(min {min(wall):.3f}, max {max(wall):.3f})", flush=True)
        del models
