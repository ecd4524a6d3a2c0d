"""What the packed max-backward record and the row-partitioned GraphSAGE cost, on the Reddit-shaped stand-in
(synth_reddit_like(1.0, seed=1)), on the protocol of profiles/experiments/sage.py:
  * per call at d = 128 and d = 41, in one run, the sides taking turns: mggcn_agg_max_pack_f32, mggcn_agg_max_backward_rec_f32
    and mggcn_agg_max_backward_f32 on the same (arg, G); the record call's G_B must carry the plain call's bits;
  * the epoch [608, 128, 128, 128, 41] of dist_sage at ONE rank (nothing exchanged: the plain kernels) next to sage's, both
    aggregators, in the same process;
  * the same epoch with FOUR ranks sharing the one GPU over gloo (every collective staged through the host): this measures
    the code path -- the packs, the record kernels over row blocks, the all-reduces --, not scaling.  Nothing here has run on
    more than one physical GPU.
Device events (calls) and the host's wall clock around train_step + synchronisation (epochs) after a warm-up, medians of
SAMPLES samples with their minimum and maximum.  A manual script, not a test; not to be run under a profiler.
Usage: python profiles/experiments/dist_sage.py
       python profiles/experiments/dist_sage.py --sage-epoch TREE LABEL
The second form prints only sage's epoch, from the built checkout at TREE (this one, or the parent commit's): run it for the
two trees in turn to see that the one-GPU model costs what it did."""
import os
import socket
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if len(sys.argv) == 4 and sys.argv[1] == "--sage-epoch":
    ROOT = os.path.abspath(sys.argv[2])
sys.path.insert(0, ROOT)
import __graft_entry__ as g                              # noqa: E402

SAMPLES = 7
SIZES = [608, 128, 128, 128, 41]
ADAM = (1e-2, 0.9, 0.999, 5e-4, 1e-8)
RANKS = 4


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def init(rank, P, port):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=P)
    return dist


def load(pkg, path):
    ip, ix, dv = (np.load(os.path.join(path, f"{k}.npy"), mmap_mode="r") for k in ("ip", "ix", "dv"))
    n = ip.shape[0] - 1
    A = pkg.csr_matrix(np.array(ip), np.array(ix), np.array(dv), n)
    A.normalize(True)
    return A, n, np.load(os.path.join(path, "X.npy")), np.load(os.path.join(path, "Y.npy"))


def timed_epochs(step, sync):
    for _ in range(2):
        step()
    wall = []
    for _ in range(SAMPLES):
        sync()
        t0 = time.perf_counter()
        res = step()
        wall.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(wall), min(wall), max(wall), res[0]


def dist_epochs(pkg, dctx, A, n, Xh, Yh, tag, barrier=None):
    """the epoch of dist_sage for both aggregators on this rank's context; returns {aggr: (median, min, max, loss)}"""
    D = pkg.dist
    p = D.partition_bounds(n, dctx.P)
    Ad, ATd = D.dist_row_csr_matrix(dctx, A, p, p), D.dist_row_csr_matrix(dctx, A.transpose(), p, p)
    Xd, Yd = D.dist_row_dn_matrix(dctx, Xh), D.dist_row_dn_matrix(dctx, Yh)
    out = {}
    for aggr in ("mean", "max"):
        model = D.dist_sage(dctx, Ad, ATd, SIZES, aggr=aggr)
        if barrier is not None:
            barrier()
        out[aggr] = timed_epochs(lambda: model.train_step(dctx, Xd, Yd, *ADAM), dctx.sync)
        del model
    return out


def rank_main(rank, P, port, path, q):
    dist = init(rank, P, port)
    try:
        pkg = g.load_package()
        dctx = pkg.dist.dist_context(overlap=True, device_index=0)
        A, n, Xh, Yh = load(pkg, path)
        q.put((rank, dist_epochs(pkg, dctx, A, n, Xh, Yh, f"P = {P}", dist.barrier), None))
    except Exception:
        import traceback
        q.put((rank, None, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def sage_epoch(label):
    pkg = g.load_package()
    ctx = pkg.context(0)
    (ip, ix, dv), Xh, Yh = pkg.datasets.synth_reddit_like(1.0, seed=1)
    n = ip.shape[0] - 1
    X, Y = pkg.dn_matrix.from_numpy(Xh), pkg.dn_matrix.from_numpy(Yh.reshape(-1, 1).astype(np.int32))
    for aggr in ("mean", "max"):
        model = pkg.sage(pkg.csr_matrix(ip, ix, dv.copy(), n), SIZES, aggr=aggr)
        med, lo, hi, loss = timed_epochs(lambda: model.train_step(ctx, X, Y, *ADAM), ctx.sync)
        print(f"[sage epoch] {label:7s} aggr={aggr:4s} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f}) loss {loss:.4f}", flush=True)
        del model


def main():
    import torch.multiprocessing as mp
    pkg = g.load_package()
    ctx = pkg.context(0)
    lib, ops, dn = ctx.lib, pkg.ops, pkg.dn_matrix

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
    Yh = Yh.reshape(-1, 1).astype(np.int32)
    path = tempfile.mkdtemp(prefix="dist_sage_")
    for k, a in (("ip", ip), ("ix", ix), ("dv", dv), ("X", Xh), ("Y", Yh)):
        np.save(os.path.join(path, f"{k}.npy"), a)
    A, n, _, _ = load(pkg, path)
    F = A.transpose()
    F_T = F.transpose()                                   # the row-sorted pattern of A: what every backward walks
    print(f"[graph] n {n}, nnz {A.nnz()}", flush=True)

    # ---- the calls -----------------------------------------------------------------------------------------------------------
    import torch
    rng = np.random.default_rng(3)
    for d in (128, 41):
        B = dn.from_numpy(rng.standard_normal((n, d), dtype=np.float32))
        G = dn.from_numpy(rng.standard_normal((n, d), dtype=np.float32))
        out, G_B, G_B_rec = dn(n, d), dn(n, d), dn(n, d)
        arg = dn(n, d, dtype=np.int32)
        rec = torch.empty(n * d * 2, dtype=torch.int32, device="cuda")
        ops.agg_max_forward(ctx, F, B, out, arg)
        res = alternate({
            "agg_max_backward (plain)": lambda: ops.agg_max_backward(ctx, F_T, arg, G, G_B),
            "agg_max_pack": lambda: ops.agg_max_pack(ctx, arg, G, rec),
            "agg_max_backward_rec": lambda: ops.agg_max_backward_rec(ctx, F_T, rec, d, G_B_rec),
            "pack + backward_rec": lambda: (ops.agg_max_pack(ctx, arg, G, rec), ops.agg_max_backward_rec(ctx, F_T, rec, d, G_B_rec)),
        })
        for name, (med, lo, hi) in res.items():
            print(f"[d = {d}] {name:28s} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
        plain, both = res["agg_max_backward (plain)"], res["pack + backward_rec"]
        print(f"[d = {d}] plain - (pack + rec) = {plain[0] - both[0]:+.3f} ms; the plain call's spread (max - min) "
              f"{plain[2] - plain[1]:.3f} ms", flush=True)
        same = bool((G_B.numpy().view(np.uint32) == G_B_rec.numpy().view(np.uint32)).all())
        print(f"[d = {d}] the record call's G_B has the plain call's bits: {same}", flush=True)
        assert same
        del B, G, out, G_B, G_B_rec, arg, rec
    del F, F_T

    # ---- the epoch at one rank, next to sage ---------------------------------------------------------------------------------
    def show(tag, name, r):
        print(f"[epoch {SIZES}] {tag:8s} {name:28s} {r[0]:9.3f} ms (min {r[1]:.3f}, max {r[2]:.3f}); loss {r[3]:.4f}", flush=True)

    X, Y = dn.from_numpy(Xh), dn.from_numpy(Yh)
    for aggr in ("mean", "max"):
        model = pkg.sage(pkg.csr_matrix(ip, ix, dv.copy(), n), SIZES, aggr=aggr)
        show("one GPU", f"sage(aggr='{aggr}')", timed_epochs(lambda: model.train_step(ctx, X, Y, *ADAM), ctx.sync))
        del model
    del X, Y
    dist = init(0, 1, free_port())
    dctx = pkg.dist.dist_context(overlap=True, device_index=0)
    for aggr, r in dist_epochs(pkg, dctx, A, n, Xh, Yh, "P = 1").items():
        show("P = 1", f"dist_sage(aggr='{aggr}')", r)
    dist.destroy_process_group()
    del dctx, A
    torch.cuda.empty_cache()

    # ---- four ranks sharing the GPU ------------------------------------------------------------------------------------------
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = free_port()
    procs = [mpc.Process(target=rank_main, args=(r, RANKS, port, path, q)) for r in range(RANKS)]
    for pr in procs:
        pr.start()
    res = sorted([q.get(timeout=900) for _ in range(RANKS)], key=lambda t: t[0])
    for pr in procs:
        pr.join(timeout=60)
    for rank, out, err in res:
        assert err is None, err
        for aggr, r in out.items():
            show(f"P = {RANKS}", f"dist_sage(aggr='{aggr}') rank {rank}", r)
    for k in ("ip", "ix", "dv", "X", "Y"):
        os.remove(os.path.join(path, f"{k}.npy"))
    os.rmdir(path)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--sage-epoch":
        assert os.path.dirname(os.path.abspath(g.__file__)) == ROOT        # the package of TREE, not of this checkout
        sage_epoch(sys.argv[3])
    else:
        main()
