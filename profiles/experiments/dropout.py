"""What dropout costs: mggcn_dropout_f32 in place on [232 968 x 128] against mggcn_leaky_relu_forward_f32 on
the same buffer (the same bytes: the ratio is the price of the generator), on [232 968 x 41] (the element path), and one
Reddit-shaped epoch at p = 0.5 against p = 0.  Device events, medians of 20 samples, the two sides of a comparison
alternating inside one process; a kernel sample is INNER calls back to back.  A manual script, not a test.
Usage: python profiles/experiments/dropout.py [--no-epoch]"""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import __graft_entry__ as g

pkg = g.load_package()
ctx = pkg.context(0)
lib = ctx.lib
N, SAMPLES, INNER = 232_968, 20, 10


def sample(fn, calls):
    """device milliseconds per call of ``calls`` back-to-back calls of fn"""
    ctx.record("exp-begin", 0)
    for _ in range(calls):
        fn()
    ctx.record("exp-end", 0)
    ctx.sync()
    return float(lib.mggcn_event_elapsed_ms(ctx.events["exp-begin"], ctx.events["exp-end"])) / calls


def alternate(sides, calls):
    """{name: (median, min, max)} in ms of SAMPLES samples per side, the sides taking turns"""
    for fn in sides.values():                        # warm-up: code objects, caches
        sample(fn, calls)
    got = {name: [] for name in sides}
    for _ in range(SAMPLES):
        for name, fn in sides.items():
            got[name].append(sample(fn, calls))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in got.items()}


threshold, _ = pkg.ops.dropout_params(0.5)
for m in (128, 41):
    X = pkg.dn_matrix.from_numpy(np.random.default_rng(m).standard_normal((N, m), dtype=np.float32))
    mbytes = 2 * 4 * N * m / 1e6                     # read + write
    # scale 1 (the kernel never sees p): the buffer keeps its magnitudes over thousands of in-place calls
    res = alternate({"dropout": lambda: pkg.ops.dropout_raw(ctx, X, X, threshold, 1.0, 7, 3),
                     "leaky_relu": lambda: pkg.ops.leaky_relu_forward(ctx, X, X)}, INNER)
    for name, (med, lo, hi) in res.items():
        print(f"[{N} x {m}] {name:10s} {med * 1e3:8.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})  "
              f"{mbytes / med / 1e3:6.2f} TB/s of {mbytes:.0f} MB", flush=True)
    print(f"[{N} x {m}] dropout / leaky_relu = {res['dropout'][0] / res['leaky_relu'][0]:.3f}", flush=True)
    del X

if "--no-epoch" not in sys.argv:
    (ip, ix, dv), Xh, Yh = pkg.datasets.synth_reddit_like(1.0, seed=1)
    n = ip.shape[0] - 1
    sizes = [Xh.shape[1], 128, 128, 128, 1 + int(Yh.max())]
    G = pkg.gcn(pkg.csr_matrix(ip, ix, dv, n), sizes)
    Xd, Yd = pkg.dn_matrix.from_numpy(Xh), pkg.dn_matrix.from_numpy(Yh)

    def epoch(p):
        def run():
            G.set_dropout(p, seed=7, epoch=0)        # a host assignment; the same masks every sample
            G.train_step(ctx, Xd, Yd, 1e-2, 0.9, 0.999, 5e-4, 1e-8)
        return run
    res = alternate({"p=0": epoch(0.0), "p=0.5": epoch(0.5)}, 1)
    for name, (med, lo, hi) in res.items():
        print(f"[epoch {sizes}] {name:6s} {med:7.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
    d = res["p=0.5"][0] - res["p=0"][0]
    passes = 2 * (len(sizes) - 2)                    # forward and backward of every layer but the first
    print(f"[epoch] dropout adds {d * 1e3:.0f} us = {100 * d / res['p=0'][0]:.2f} % "
          f"({passes} passes of {2 * 4 * n * 128 / 1e6:.0f} MB)", flush=True)
    out = __import__("io").StringIO()
    ctx.dump_timers(out, "")
    print("\n".join(ln for ln in out.getvalue().splitlines() if "dropout" in ln), flush=True)
