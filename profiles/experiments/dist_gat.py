"""What the row-partitioned GAT costs with one rank: one epoch of
dist_gat([608, 128, 128, 128, 41], heads=4) beside one epoch of gat on the same sizes, in one process on the Reddit-shaped
stand-in (synth_reddit_like(1.0, seed=1)), the two taking turns.  One rank exchanges nothing, so the two run the same
kernels but for backward_src, which dist_gat calls on the packed record (plus the pack) and gat on three scalar arrays: by
gat_rec.log that is about 9 ms less in each of the three 128-wide layers and about 0.6 ms more in the 41-wide one, so
dist_gat should come out some 26 ms below gat, and everything else should agree (the per-kernel timers are printed).
With --self-gather the rank's all-gathers run too (device-to-device copies of n x out floats through the process group):
what the exchange costs when nothing is overlapped with it, not a multi-GPU number.  Ranks sharing one GPU are a
correctness rehearsal, not a speed measurement, and more than one physical GPU has not been run.
The protocol of gat.py: device events after a warm-up, medians of SAMPLES samples.  A manual script, not a test; not to be
run under a profiler.
Usage: python profiles/experiments/dist_gat.py [--self-gather]"""
import io
import os
import socket
import statistics
import sys

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
lib, dn = ctx.lib, pkg.dn_matrix
SAMPLES, K = 7, 4
ADAM = (1e-2, 0.9, 0.999, 5e-4, 1e-8)


def sample(fn):
    ctx.record("exp-begin", 0)
    fn()
    ctx.record("exp-end", 0)
    ctx.sync()
    return float(lib.mggcn_event_elapsed_ms(ctx.events["exp-begin"], ctx.events["exp-end"]))


def alternate(sides):
    for fn in sides.values():
        sample(fn)
    got = {name: [] for name in sides}
    for _ in range(SAMPLES):
        for name, fn in sides.items():
            got[name].append(sample(fn))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in got.items()}


(ip, ix, dv), Xh, Yh = pkg.datasets.synth_reddit_like(1.0, seed=1)
n = ip.shape[0] - 1
sizes = [Xh.shape[1], 128, 128, 128, 1 + int(Yh.max())]
A = pkg.csr_matrix(ip, ix, dv.copy(), n)
p = D.partition_bounds(n, 1)
single = pkg.gat(pkg.csr_matrix(ip, ix, dv.copy(), n), sizes, heads=K)
part = D.dist_gat(dctx, D.dist_row_csr_matrix(dctx, A, p, p, keep_rows=True), D.dist_row_csr_matrix(dctx, A.transpose(), p, p), sizes, heads=K)
X1, Y1 = dn.from_numpy(Xh), dn.from_numpy(Yh)
Xd, Yd = D.dist_row_dn_matrix(dctx, Xh), D.dist_row_dn_matrix(dctx, Yh)
res = alternate({"gat": lambda: single.train_step(ctx, X1, Y1, *ADAM), "dist_gat": lambda: part.train_step(dctx, Xd, Yd, *ADAM)})
for name, (med, lo, hi) in res.items():
    print(f"[epoch {sizes}, P = 1, self-gather {SELF}] {name:8s} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
print(f"[ratio] dist_gat / gat = {res['dist_gat'][0] / res['gat'][0]:.4f}", flush=True)
text = io.StringIO()
ctx.dump_timers(text, "")
print("\n".join(ln for ln in text.getvalue().splitlines() if "gat-" in ln), flush=True)
dist.destroy_process_group()
