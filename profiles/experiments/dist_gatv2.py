"""What the packed (lse, D) record and the row-partitioned GATv2 cost with one rank, on the Reddit-shaped
stand-in (synth_reddit_like(1.0, seed=1)), in one process, the sides taking turns:
  1. mggcn_gatv2_backward_src_f32 (lse and D as two [n x heads] arrays: the kernel as it was) beside
     mggcn_gatv2_backward_src_rec_f32 (one 8-byte record per (destination, head)) over F^T, at the two layer shapes of the
     epoch [608, 128, 128, 128, 41]: 128 columns with 4 heads and 41 columns with 1 head; either side first; the pack itself
     is timed too, and both sides' outputs are compared as bits;
  2. one epoch of gat(variant="v2") beside one epoch of dist_gat(variant="v2") at P = 1 on the record and on the plain call
     (attn.packed flipped on a second model).  One rank exchanges nothing, so the three run the same kernels but for
     backward_src and the pack; the per-kernel timers are printed.
With --self-gather the rank's three all-gathers run too (device-to-device copies through the process group): what the
exchange costs when nothing is overlapped with it, not a multi-GPU number.  Ranks sharing one GPU are a correctness
rehearsal, not a speed measurement, and more than one physical GPU has not been run.
The protocol of gat.py: device events after a warm-up, medians of SAMPLES samples.  A manual script, not a test; not to be
run under a profiler.
Usage: python profiles/experiments/dist_gatv2.py [--self-gather]"""
import io
import os
import socket
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import __graft_entry__ as g

SELF = "--self-gather" in sys.argv
if SELF:
    os.environ["MGGCN_DIST_SELF_GATHER"] = "1"
import torch
import torch.distributed as dist

s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
if SELF:
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
else:
    dist.init_process_group("gloo", rank=0, world_size=1)

pkg = g.load_package()
D = pkg.dist
dctx = D.dist_context(overlap=True, device_index=0)
ctx = dctx.ctx
lib, ops, dn = ctx.lib, pkg.ops, pkg.dn_matrix
SAMPLES, K = 7, 4
ADAM = (1e-2, 0.9, 0.999, 5e-4, 1e-8)


def sample(fn):
    ctx.record("exp-begin", 0)
    fn()
    ctx.record("exp-end", 0)
    ctx.sync()
    return float(lib.mggcn_event_elapsed_ms(ctx.events["exp-begin"], ctx.events["exp-end"]))


def alternate(sides):
    for fn in sides.values():                        # warm-up: code objects, caches
        sample(fn)
    got = {name: [] for name in sides}
    for _ in range(SAMPLES):
        for name, fn in sides.items():
            got[name].append(sample(fn))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in got.items()}


(ip, ix, dv), Xh, Yh = pkg.datasets.synth_reddit_like(1.0, seed=1)
n = ip.shape[0] - 1
A = pkg.csr_matrix(ip, ix, dv.copy(), n)             # F^T: what backward_src walks
F = A.transpose()
print(f"[graph] n {n}, nnz {A.nnz()}, longest row of F^T {np.diff(A.indptr.astype(np.int64)).max()}", flush=True)

if not SELF:
    for W, H in ((128, 4), (41, 1)):
        rng = np.random.default_rng(W)
        Z2, G = dn.from_numpy(rng.standard_normal((n, 2 * W), dtype=np.float32)), dn.from_numpy(rng.standard_normal((n, W), dtype=np.float32))
        att = dn.from_numpy((0.1 * rng.standard_normal((1, W))).astype(np.float32))
        out, P, lse, Dm = dn(n, W), dn(n, W), dn(n, H), dn(n, H)
        outs = {name: dn(n, 2 * W) for name in ("plain", "record")}
        ops.gatv2_forward(ctx, F, Z2, Z2, att, out, lse, H)
        ops.gatv2_backward_dst(ctx, F, Z2, Z2, att, lse, G, out, Dm, outs["plain"], P, H)
        rec = torch.empty(n * H * 2, dtype=torch.float32, device=ctx.device)
        ops.gatv2_pack_dst(ctx, lse, Dm, rec)
        ctx.sync()
        sides = {
            "plain": lambda: ops.gatv2_backward_src(ctx, A, Z2, Z2, att, lse, Dm, G, outs["plain"], H),
            "record": lambda: ops.gatv2_backward_src_rec(ctx, A, Z2, Z2, att, rec, G, outs["record"], H),
        }
        for turn, order in enumerate((("plain", "record"), ("record", "plain"))):       # either side first
            res = alternate({name: sides[name] for name in order})
            for name in ("plain", "record"):
                med, lo, hi = res[name]
                print(f"[{n} x {W}, heads {H}] turn {turn} gatv2_backward_src {name:6s} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
            print(f"[{n} x {W}, heads {H}] turn {turn} record - plain = {res['record'][0] - res['plain'][0]:+.3f} ms, "
                  f"record / plain = {res['record'][0] / res['plain'][0]:.4f}", flush=True)
        med, lo, hi = alternate({"pack": lambda: ops.gatv2_pack_dst(ctx, lse, Dm, rec)})["pack"]
        print(f"[{n} x {W}, heads {H}] gatv2_pack_dst {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
        same = torch.equal(outs["plain"].t[:, :W].contiguous().view(torch.int32), outs["record"].t[:, :W].contiguous().view(torch.int32))
        print(f"[{n} x {W}, heads {H}] G_Zs bit-equal: {same}", flush=True)
        assert same
        del Z2, G, out, P, outs, rec

sizes = [Xh.shape[1], 128, 128, 128, 1 + int(Yh.max())]
p = D.partition_bounds(n, 1)
Ad, ATd = D.dist_row_csr_matrix(dctx, A, p, p, keep_rows=True), D.dist_row_csr_matrix(dctx, F, p, p)
single = pkg.gat(pkg.csr_matrix(ip, ix, dv.copy(), n), sizes, heads=K, variant="v2")
X1, Y1 = dn.from_numpy(Xh), dn.from_numpy(Yh)
Xd, Yd = D.dist_row_dn_matrix(dctx, Xh), D.dist_row_dn_matrix(dctx, Yh)
sides = {"gat v2": lambda: single.train_step(ctx, X1, Y1, *ADAM)}
parts = {}
for name, packed in (("dist_gat v2 plain", False), ("dist_gat v2 record", True)):      # the timers printed are the last side's
    if SELF and not packed:
        continue                                     # a layer that exchanges reads the gathered record
    parts[name] = D.dist_gat(dctx, Ad, ATd, sizes, heads=K, variant="v2")
    for layer in parts[name].layers():
        layer.attn.packed = packed
    sides[name] = lambda G=parts[name]: G.train_step(dctx, Xd, Yd, *ADAM)
res = alternate(sides)
for name, (med, lo, hi) in res.items():
    print(f"[epoch {sizes}, P = 1, self-gather {SELF}] {name:18s} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
for name in parts:
    print(f"[ratio] {name} / gat v2 = {res[name][0] / res['gat v2'][0]:.4f}", flush=True)
text = io.StringIO()
ctx.dump_timers(text, "")
print("\n".join(ln for ln in text.getvalue().splitlines() if "gatv2-" in ln), flush=True)
dist.destroy_process_group()
