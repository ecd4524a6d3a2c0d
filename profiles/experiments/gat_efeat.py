"""What edge features in the score cost, on the Reddit-shaped stand-in (synth_reddit_like(1.0, seed=1)) at
de = 8, with the protocol of profiles/experiments/gat.py:
  * per call at 128 columns / 4 heads and at 41 columns / 1 head: mggcn_gat_forward_efeat_f32, mggcn_gat_backward_dst_efeat_f32
    (over F, with E in F's entry order) and mggcn_gat_backward_src_efeat_f32 (over F^T, with the other copy), each beside
    its plain twin in the same process, and the column sum of P_e;
  * one epoch of gat([608, 128, 128, 128, 41], heads=4) with and without edge_attr, the models taking turns, and the
    per-layer timers of one epoch of each.
  * --default-epoch LABEL: nothing of the above, only the epoch of the default gat(A, [608, 128, 128, 128, 41], heads=4) of
    the tree in the CURRENT DIRECTORY (the one whose __graft_entry__.py is there), printed under LABEL.  Run it from a
    built checkout of the parent commit and from this one, one process per side, taking turns, for the comparison of the
    default model against the parent; the GCN epoch of the same comparison is bench.py --gpus 1 --steps 10 --warmup 3 in
    each tree.
Device events after a warm-up, medians of SAMPLES samples, the sides of a comparison taking turns.  A manual script, not a
test; not to be run under a profiler.
Usage: python profiles/experiments/gat_efeat.py [--no-epoch]
       cd <a built tree> && python <this file> --default-epoch LABEL"""
import io
import os
import statistics
import sys
import time

import numpy as np

DEFAULT_EPOCH = sys.argv[sys.argv.index("--default-epoch") + 1] if "--default-epoch" in sys.argv else None
sys.path.insert(0, os.getcwd() if DEFAULT_EPOCH is not None else
                os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import __graft_entry__ as g

pkg = g.load_package()
ctx = pkg.context(0)
lib, ops, dn = ctx.lib, pkg.ops, pkg.dn_matrix
gat_module = sys.modules[pkg.__name__ + ".gat"]
SAMPLES, DE = 7, 8


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
if DEFAULT_EPOCH is not None:
    sizes = [Xh.shape[1], 128, 128, 128, 1 + int(Yh.max())]
    M = pkg.gat(A, sizes, heads=4)
    Xd, Yd = dn.from_numpy(Xh), dn.from_numpy(Yh)
    step = lambda: M.train_step(ctx, Xd, Yd, 1e-2, 0.9, 0.999, 5e-4, 1e-8)
    sample(step)
    v = [sample(step) for _ in range(SAMPLES)]
    print(f"[epoch {sizes}] gat() {DEFAULT_EPOCH:12s} {statistics.median(v):9.3f} ms (min {min(v):.3f}, max {max(v):.3f})", flush=True)
    sys.exit(0)
F = A.transpose()
rng = np.random.default_rng(0)
t0 = time.time()
E_host = (0.5 * rng.standard_normal((A.nnz(), DE), dtype=np.float32))
perm = gat_module.edge_permutation(A)
print(f"[graph] n {n}, nnz {F.nnz()}, de {DE}: E {E_host.nbytes / 1e9:.2f} GB per copy, the permutation took "
      f"{time.time() - t0:.1f} s on the host", flush=True)
E_A, E_F = dn.from_numpy(E_host), dn.from_numpy(E_host[perm])
del perm

for D, K in ((128, 4), (41, 1)):
    Z, G = (dn.from_numpy(rng.standard_normal((n, D), dtype=np.float32)) for _ in range(2))
    att = dn.from_numpy((0.1 * rng.standard_normal((2, D))).astype(np.float32))
    U = dn.from_numpy((0.07 * rng.standard_normal((K, DE))).astype(np.float32))
    out, G_Z = dn(n, D), dn(n, D)
    s_dst, s_src, lse, Dm, ds_dst, ds_src = (dn(n, K) for _ in range(6))
    P_e, G_U = dn(n, K * DE), dn(1, K * DE)
    ops.gat_scores(ctx, Z, att, s_dst, s_src, K)
    ops.gat_forward(ctx, F, Z, s_dst, s_src, out, lse, K)
    ops.gat_backward_dst(ctx, F, Z, s_dst, s_src, lse, G, out, Dm, ds_dst, K)
    ctx.sync()
    res = alternate({
        "gat_forward": lambda: ops.gat_forward(ctx, F, Z, s_dst, s_src, out, lse, K),
        "gat_forward_efeat": lambda: ops.gat_forward_efeat(ctx, F, Z, s_dst, s_src, out, lse, E_F, U, K),
        "gat_backward_dst": lambda: ops.gat_backward_dst(ctx, F, Z, s_dst, s_src, lse, G, out, Dm, ds_dst, K),
        "gat_backward_dst_efeat": lambda: ops.gat_backward_dst_efeat(ctx, F, Z, s_dst, s_src, lse, G, out, Dm, ds_dst, E_F, U, P_e, K),
        "gat_backward_src": lambda: ops.gat_backward_src(ctx, A, Z, s_dst, s_src, lse, Dm, G, att, ds_dst, ds_src, G_Z, K),
        "gat_backward_src_efeat": lambda: ops.gat_backward_src_efeat(ctx, A, Z, s_dst, s_src, lse, Dm, G, att, ds_dst, ds_src, G_Z, E_A, U, K),
        "att_edge column sum": lambda: ops.gatv2_att_grad(ctx, P_e, G_U),
    })
    for name, (med, lo, hi) in res.items():
        print(f"[{n} x {D}, heads {K}, de {DE}] {name:24s} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
    for a in ("gat_forward", "gat_backward_dst", "gat_backward_src"):
        extra = res[a + "_efeat"][0] - res[a][0]
        print(f"[ratio {D} / {K}] {a}_efeat / {a} = {res[a + '_efeat'][0] / res[a][0]:.3f}  (+{extra:.3f} ms = "
              f"{1e9 * extra / (F.nnz() * K):.2f} ps per (entry, head))", flush=True)
    del Z, G, out, G_Z, P_e
del E_A, E_F

if "--no-epoch" not in sys.argv:
    sizes = [Xh.shape[1], 128, 128, 128, 1 + int(Yh.max())]
    models = {"gat()": pkg.gat(A, sizes, heads=4), "gat(edge_attr=E)": pkg.gat(A, sizes, heads=4, edge_attr=E_host)}
    del E_host
    Xd, Yd = dn.from_numpy(Xh), dn.from_numpy(Yh)
    res = alternate({name: (lambda M_=M_: M_.train_step(ctx, Xd, Yd, 1e-2, 0.9, 0.999, 5e-4, 1e-8)) for name, M_ in models.items()})
    for name, (med, lo, hi) in res.items():
        print(f"[epoch {sizes}] {name:18s} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
    for name, M_ in models.items():                    # where the epoch's difference sits: the model's own timers, one epoch each
        M_.train_step(ctx, Xd, Yd, 1e-2, 0.9, 0.999, 5e-4, 1e-8)
        text = io.StringIO()
        ctx.dump_timers(text, "")
        print(f"[timers {name}] " + "  ".join(ln for ln in text.getvalue().splitlines() if "gat-" in ln and "scores" not in ln
                                                 and ("edge" in name or "edge-grad" not in ln)), flush=True)      # the context keeps old timers
