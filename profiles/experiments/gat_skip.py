"""What the skip connection and the layer norm of the attention models cost, on the Reddit-shaped
stand-in (synth_reddit_like(1.0, seed=1)), on the protocol of profiles/experiments/gatdot.py:
  * per call at 128 columns: mggcn_gated_skip_forward_f32 / _backward_f32, with the gate and without, next to
    mggcn_layer_norm_forward_f32 / _backward_f32 on the same shape in the same run.  The norm pair is the yardstick: the
    gated forward moves three [n x m] matrices as the norm's forward does (reads o and r, writes y; the norm reads x, writes
    y and xhat), the gated backward six where the norm's moves four (reads G, act, o, r, writes G_o and G_r; the norm reads
    G, act, xhat, writes G_in) -- 1x and 1.5x are what the bytes say;
  * one epoch of gat([608, 128, 128, 128, 41], heads=4) of every variant, default against skip="gate", norm="layer", in
    the same process.
Device events after a warm-up, medians of SAMPLES samples, the sides of a comparison taking turns.  A manual script, not a
test; not to be run under a profiler.
Usage: python profiles/experiments/gat_skip.py [--no-epoch | --default-only]
--default-only times the default models alone (run it on two checkouts to compare a change against its parent)."""
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
print(f"[graph] n {n}, nnz {A.nnz()}", flush=True)

if "--default-only" not in sys.argv:
    D = 128
    rng = np.random.default_rng(0)
    o, r, G = (dn.from_numpy(rng.standard_normal((n, D), dtype=np.float32)) for _ in range(3))
    w = dn.from_numpy((0.5 / np.sqrt(D) * rng.standard_normal((3, D))).astype(np.float32))
    gamma, beta = dn.from_numpy(np.ones((1, D), dtype=np.float32)), dn.from_numpy(np.zeros((1, D), dtype=np.float32))
    y, xhat, G_o, G_r, G_in = (dn(n, D) for _ in range(5))
    gate, rstd = dn(n, 1), dn(n, 1)
    G_w, G_gamma, G_beta = dn(3, D), dn(1, D), dn(1, D)
    GATE, LEAKY = ops.GATED_SKIP_GATE, ops.GATED_SKIP_LEAKY_RELU
    ops.gated_skip(ctx, o, r, w, y, gate, GATE | LEAKY)
    ops.layer_norm(ctx, o, y, xhat, rstd, gamma, beta, ops.LAYER_NORM_LEAKY_RELU)
    ctx.sync()
    res = alternate({
        "layer_norm_forward": lambda: ops.layer_norm(ctx, o, y, xhat, rstd, gamma, beta, ops.LAYER_NORM_LEAKY_RELU),
        "gated_skip_forward (gate)": lambda: ops.gated_skip(ctx, o, r, w, y, gate, GATE | LEAKY),
        "gated_skip_forward (add)": lambda: ops.gated_skip(ctx, o, r, None, y, None, LEAKY),
        "layer_norm_backward": lambda: ops.layer_norm_backward(ctx, G, y, xhat, rstd, gamma, G_in, G_gamma, G_beta,
                                                               ops.LAYER_NORM_LEAKY_RELU),
        "gated_skip_backward (gate)": lambda: ops.gated_skip_backward(ctx, G, y, o, r, w, gate, G_o, G_r, G_w, GATE | LEAKY),
        "gated_skip_backward (add)": lambda: ops.gated_skip_backward(ctx, G, y, None, None, None, None, G_o, G_o, None, LEAKY),
    })
    for name, (med, lo, hi) in res.items():
        print(f"[{n} x {D}] {name:28s} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
    for mode in ("gate", "add"):
        for p in ("forward", "backward"):
            print(f"[ratio] gated_skip_{p} ({mode}) / layer_norm_{p} = "
                  f"{res[f'gated_skip_{p} ({mode})'][0] / res[f'layer_norm_{p}'][0]:.2f}", flush=True)
    del o, r, G, y, xhat, G_o, G_r, G_in

if "--no-epoch" not in sys.argv:
    sizes = [Xh.shape[1], 128, 128, 128, 1 + int(Yh.max())]
    Xd, Yd = dn.from_numpy(Xh), dn.from_numpy(Yh)
    for variant in ("v1", "v2", "dot"):
        models = {f"{variant} default": pkg.gat(A, sizes, heads=4, variant=variant)}
        if "--default-only" not in sys.argv:
            models[f"{variant} gate+norm"] = pkg.gat(A, sizes, heads=4, variant=variant, skip="gate", norm="layer")
        res = alternate({name: (lambda M_=M_: M_.train_step(ctx, Xd, Yd, 1e-2, 0.9, 0.999, 5e-4, 1e-8))
                         for name, M_ in models.items()})
        for name, (med, lo, hi) in res.items():
            print(f"[epoch {sizes}] {name:16s} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
        del models
