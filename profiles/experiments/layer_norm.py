"""What layer normalisation costs: mggcn_layer_norm_forward_f32 / _backward_f32 (activation flag set) on
[232 968 x 128] against mggcn_leaky_relu_forward_f32 / _backward_f32 on the same buffers -- the passes they replace, which
move 2 and 3 matrices where the norm moves 3 and 4 -- and one Reddit-shaped epoch with norm="layer" against without.
Device events, medians of 20 samples, the two sides of a comparison alternating inside one process; a kernel sample is
INNER calls back to back.  A manual script, not a test.
Usage: python profiles/experiments/layer_norm.py [--no-epoch]"""
import io
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import __graft_entry__ as g

pkg = g.load_package()
ctx = pkg.context(0)
lib = ctx.lib
N, M, SAMPLES, INNER = 232_968, 128, 20, 10
LEAKY = pkg.ops.LAYER_NORM_LEAKY_RELU


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
    for fn in sides.values():                        # warm-up: code objects, caches, the backward's scratch
        sample(fn, calls)
    got = {name: [] for name in sides}
    for _ in range(SAMPLES):
        for name, fn in sides.items():
            got[name].append(sample(fn, calls))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in got.items()}


def report(res, matrices):
    for name, (med, lo, hi) in res.items():
        mbytes = matrices[name] * 4 * N * M / 1e6
        print(f"[{N} x {M}] {name:20s} {med * 1e3:8.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})  "
              f"{mbytes / med / 1e3:6.2f} TB/s of {mbytes:.0f} MB", flush=True)


rng = np.random.default_rng(M)
dn = pkg.dn_matrix
X, Y, G, T = (dn.from_numpy(rng.standard_normal((N, M), dtype=np.float32)) for _ in range(4))
xhat, rstd = dn(N, M), dn(N, 1)
gamma, beta = dn.from_numpy(np.ones((1, M), dtype=np.float32)), dn.from_numpy(np.zeros((1, M), dtype=np.float32))
G_gamma, G_beta = dn(1, M), dn(1, M)
# out of place, so that thousands of calls see the same input
report(alternate({"layer_norm forward": lambda: pkg.ops.layer_norm(ctx, X, Y, xhat, rstd, gamma, beta, LEAKY),
                  "leaky_relu forward": lambda: pkg.ops.leaky_relu_forward(ctx, X, Y)}, INNER),
       {"layer_norm forward": 3, "leaky_relu forward": 2})
report(alternate({"layer_norm backward": lambda: pkg.ops.layer_norm_backward(ctx, G, Y, xhat, rstd, gamma, T, G_gamma, G_beta, LEAKY),
                  "leaky_relu backward": lambda: pkg.ops.leaky_relu_backward(ctx, Y, G, T)}, INNER),
       {"layer_norm backward": 4, "leaky_relu backward": 3})
del X, Y, G, T, xhat, rstd

if "--no-epoch" not in sys.argv:
    (ip, ix, dv), Xh, Yh = pkg.datasets.synth_reddit_like(1.0, seed=1)
    n = ip.shape[0] - 1
    sizes = [Xh.shape[1], 128, 128, 128, 1 + int(Yh.max())]
    models = {str(norm): pkg.gcn(pkg.csr_matrix(ip, ix, dv.copy(), n), sizes, norm=norm) for norm in (None, "layer")}
    Xd, Yd = dn.from_numpy(Xh), dn.from_numpy(Yh)
    res = alternate({name: (lambda M_=M_: M_.train_step(ctx, Xd, Yd, 1e-2, 0.9, 0.999, 5e-4, 1e-8)) for name, M_ in models.items()}, 1)
    for name, (med, lo, hi) in res.items():
        print(f"[epoch {sizes}] norm={name:6s} {med:7.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
    d = res["layer"][0] - res["None"][0]
    normed = len(sizes) - 2                          # every layer but the last
    print(f"[epoch] layer norm adds {d * 1e3:.0f} us = {100 * d / res['None'][0]:.2f} % "
          f"({normed} normed layers: {normed * 7 * 4 * n * 128 / 1e6:.0f} MB of norm passes)", flush=True)
    out = io.StringIO()
    ctx.dump_timers(out, "")
    print("\n".join(ln for ln in out.getvalue().splitlines() if "norm" in ln or "activation" in ln), flush=True)
