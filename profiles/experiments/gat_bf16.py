"""What bf16 gathers buy the attention kernels, on the Reddit-shaped stand-in
(synth_reddit_like(1.0, seed=1)), on the protocol of profiles/experiments/gatdot.py:
  * per call at d = 128 with 4 heads (float4 path, LPR = 8) and at d = 41 with 1 head (element path, LPR = 64): each of the
    nine sparse calls on fp32 operands next to its _bf16 twin on images, each on the model's layout (v1: Z; GATv2: the halves
    of one [n x 2 d] buffer; dot: the thirds of one [n x 3 d] buffer), and the conversions the model pays for the images of
    that call, listed separately and added;
  * one epoch of gat([608, 128, 128, 128, 41], heads=4) of the three variants with agg_dtype "f32" against "bf16";
  * --epoch-only VARIANT: the f32 epoch of one variant alone (run from a checkout of the parent commit, in the same session,
    to show that f32 did not move).
Device events after a warm-up, medians of SAMPLES samples, the sides of a comparison taking turns in one process.  A manual
script, not a test; not to be run under a profiler.
Usage: python profiles/experiments/gat_bf16.py [--no-epoch] [--epoch-only v1|v2|dot]"""
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
ADAM = (1e-2, 0.9, 0.999, 5e-4, 1e-8)


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
F = A.transpose()
print(f"[graph] n {n}, nnz {F.nnz()}, longest row of F {np.diff(F.indptr.astype(np.int64)).max()}, "
      f"of F^T {np.diff(A.indptr.astype(np.int64)).max()}", flush=True)
sizes = [Xh.shape[1], 128, 128, 128, 1 + int(Yh.max())]


def epochs(models):
    Xd, Yd = dn.from_numpy(Xh), dn.from_numpy(Yh)
    res = alternate({name: (lambda M_=M_: M_.train_step(ctx, Xd, Yd, *ADAM)) for name, M_ in models.items()})
    for name, (med, lo, hi) in res.items():
        print(f"[epoch {sizes}] {name:12s} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
    return res


if "--epoch-only" in sys.argv:
    variant = sys.argv[sys.argv.index("--epoch-only") + 1]
    epochs({f"{variant} f32": pkg.gat(A, sizes, heads=4, variant=variant)})
    sys.exit(0)

import torch


def image(rows, cols):
    return ops.bf16_image(torch.empty((rows, cols), dtype=torch.bfloat16, device="cuda"))


def convert(M, img, c0, c1):
    ops.convert_bf16(ctx, M.t[:, c0:c1], img.t[:, c0:c1])


for D, K in ((128, 4), (41, 1)):
    rng = np.random.default_rng(0)
    Z1 = dn.from_numpy(rng.standard_normal((n, D), dtype=np.float32))
    Z2 = dn.from_numpy(rng.standard_normal((n, 2 * D), dtype=np.float32))         # GATv2's layout: [Zs | Zd]
    Z3 = dn.from_numpy(rng.standard_normal((n, 3 * D), dtype=np.float32))         # the dot model's: [Zq | Zk | Zv]
    G = dn.from_numpy(rng.standard_normal((n, D), dtype=np.float32))
    att1 = dn.from_numpy((0.1 * rng.standard_normal((2, D))).astype(np.float32))
    att2 = dn.from_numpy((0.1 * rng.standard_normal((1, D))).astype(np.float32))
    I1, I2, I3, IG = image(n, D), image(n, 2 * D), image(n, 3 * D), image(n, D)
    for M, img in ((Z1, I1), (Z2, I2), (Z3, I3), (G, IG)):
        convert(M, img, 0, M.m())
    out, P, G_Z1, G_Z2, G_Z3 = dn(n, D), dn(n, D), dn(n, D), dn(n, 2 * D), dn(n, 3 * D)
    s_dst, s_src, lse, Dm, ds_dst, ds_src = (dn(n, K) for _ in range(6))
    ops.gat_scores(ctx, Z1, att1, s_dst, s_src, K)
    # (name, the fp32 call, the bf16 call, the conversions the model makes for that call's images); every backward needs
    # its variant's forward outputs (out, lse, D) in place: the calls of a variant run forward, backward_dst, backward_src
    calls = [
        ("gat_forward (F)", lambda: ops.gat_forward(ctx, F, Z1, s_dst, s_src, out, lse, K),
         lambda: ops.gat_forward_bf16(ctx, F, I1, s_dst, s_src, out, lse, K), lambda: convert(Z1, I1, 0, D)),
        ("gat_backward_dst (F)", lambda: ops.gat_backward_dst(ctx, F, Z1, s_dst, s_src, lse, G, out, Dm, ds_dst, K),
         lambda: ops.gat_backward_dst_bf16(ctx, F, I1, s_dst, s_src, lse, G, out, Dm, ds_dst, K), lambda: convert(Z1, I1, 0, D)),
        ("gat_backward_src (F^T)", lambda: ops.gat_backward_src(ctx, A, Z1, s_dst, s_src, lse, Dm, G, att1, ds_dst, ds_src, G_Z1, K),
         lambda: ops.gat_backward_src_bf16(ctx, A, Z1, s_dst, s_src, lse, Dm, IG, att1, ds_dst, ds_src, G_Z1, K),
         lambda: convert(G, IG, 0, D)),
        ("gatv2_forward (F)", lambda: ops.gatv2_forward(ctx, F, Z2, Z2, att2, out, lse, K),
         lambda: ops.gatv2_forward_bf16(ctx, F, I2, Z2, att2, out, lse, K), lambda: convert(Z2, I2, 0, D)),
        ("gatv2_backward_dst (F)", lambda: ops.gatv2_backward_dst(ctx, F, Z2, Z2, att2, lse, G, out, Dm, G_Z2, P, K),
         lambda: ops.gatv2_backward_dst_bf16(ctx, F, I2, Z2, att2, lse, G, out, Dm, G_Z2, P, K), lambda: convert(Z2, I2, 0, D)),
        ("gatv2_backward_src (F^T)", lambda: ops.gatv2_backward_src(ctx, A, Z2, Z2, att2, lse, Dm, G, G_Z2, K),
         lambda: ops.gatv2_backward_src_bf16(ctx, A, Z2, I2, att2, lse, Dm, IG, G_Z2, K),
         lambda: (convert(Z2, I2, D, 2 * D), convert(G, IG, 0, D))),
        ("gatdot_forward (F)", lambda: ops.gatdot_forward(ctx, F, Z3, Z3, Z3, out, lse, K),
         lambda: ops.gatdot_forward_bf16(ctx, F, Z3, I3, I3, out, lse, K), lambda: convert(Z3, I3, D, 3 * D)),
        ("gatdot_backward_dst (F)", lambda: ops.gatdot_backward_dst(ctx, F, Z3, Z3, Z3, lse, G, out, Dm, G_Z3, K),
         lambda: ops.gatdot_backward_dst_bf16(ctx, F, Z3, I3, I3, lse, G, out, Dm, G_Z3, K), lambda: convert(Z3, I3, D, 3 * D)),
        ("gatdot_backward_src (F^T)", lambda: ops.gatdot_backward_src(ctx, A, Z3, Z3, Z3, lse, Dm, G, G_Z3, G_Z3, K),
         lambda: ops.gatdot_backward_src_bf16(ctx, A, I3, Z3, Z3, lse, Dm, IG, G_Z3, G_Z3, K),
         lambda: (convert(Z3, I3, 0, D), convert(G, IG, 0, D))),
    ]
    for name, f32, b16, conv in calls:
        r = alternate({"f32": f32, "bf16": b16, "convert": conv})
        a, b, c = r["f32"][0], r["bf16"][0], r["convert"][0]
        print(f"[{n} x {D}, heads {K}] {name:26s} f32 {a:8.3f} ms (min {r['f32'][1]:.3f}, max {r['f32'][2]:.3f})  "
              f"bf16 {b:8.3f} ms (min {r['bf16'][1]:.3f}, max {r['bf16'][2]:.3f})  convert {c:6.3f} ms  "
              f"bf16 / f32 {b / a:.3f}, with the conversion {(b + c) / a:.3f}", flush=True)
    del Z1, Z2, Z3, G, I1, I2, I3, IG, out, P, G_Z1, G_Z2, G_Z3

if "--no-epoch" not in sys.argv:
    for variant in ("v1", "v2", "dot"):
        models = {f"{variant} {dt}": pkg.gat(A, sizes, heads=4, variant=variant, agg_dtype=dt) for dt in ("f32", "bf16")}
        r = epochs(models)
        print(f"[epoch ratio] {variant}: bf16 / f32 = {r[variant + ' bf16'][0] / r[variant + ' f32'][0]:.3f}", flush=True)
        conv = {name: ctx.measure(name) for name in sorted(ctx.timers) if "gat-convert" in name}
        print(f"[epoch] {variant} bf16 conversions of the last epoch: {sum(conv.values()):.3f} ms in {len(conv)} timers", flush=True)
        del models
