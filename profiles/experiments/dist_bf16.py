"""fp32 against bf16 aggregation on the row partition: dist_gcn(agg_dtype="f32") and dist_gcn(agg_dtype="bf16") on the same
graph, alternating epoch by epoch in ONE process group, for every exchange schedule.

  python profiles/experiments/dist_bf16.py --gpus N            one rank per GPU over RCCL (needs N GPUs)
  python profiles/experiments/dist_bf16.py --gpus 1 --ranks R  R ranks sharing cuda:0 over gloo (a one-GPU box)

Per mode and dtype it prints, from rank 0 (times: max over ranks):
  exchange_bytes   this rank's payload handed to the shard exchange in one epoch (dist_context.exchange_bytes): exact
  exchange ms      sum of the epoch's "matmul-exchange" timers (dctx.profile_exchange, a separate pass of 3 epochs)
  epoch ms         median of 20 train_step epochs, HIP events on the compute stream around the step
Over gloo the exchange is staged through the host (device -> host, gloo, host -> device, with the streams synchronised), so
there only the byte counts and the compute side mean anything; what a multi-GPU run should be held against is the fp32
schedule of the same run (the exchange term halves, the compute term does not move).
"""
import argparse
import os
import socket
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ADAM = (1e-2, 0.9, 0.999, 5e-4, 1e-8)


def _rank_main(rank, P, port, args, shared_gpu):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dev = 0 if shared_gpu else rank
    torch.cuda.set_device(dev)
    if shared_gpu:
        dist.init_process_group("gloo", rank=rank, world_size=P)
    else:
        dist.init_process_group("nccl", rank=rank, world_size=P, device_id=torch.device("cuda", dev))
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pkg = ge.load_package()
    D = pkg.dist
    say = (lambda *a: print(*a, flush=True)) if rank == 0 else (lambda *a: None)
    (ip, ix, dv), X, Y = pkg.datasets.synth_reddit_like(args.scale, seed=1, symmetric=True)
    n = ip.shape[0] - 1
    C = 1 + int(Y.max())
    sizes = [X.shape[1]] + [args.hidden] * 3 + [(C + P - 1) // P * P]
    say(f"n = {n}, nnz = {int(ip[-1])}, sizes = {sizes}, P = {P}, backend = {dist.get_backend()}"
        f"{' (ranks share cuda:0; host-staged exchange)' if shared_gpu else ''}")
    A = pkg.csr_matrix(ip, ix, dv, n)
    A.normalize(True)
    A_T = A.transpose()
    p = D.partition_bounds(n, P)
    dctx = D.dist_context(overlap=True, device_index=dev)
    Ad, ATd = D.dist_row_csr_matrix(dctx, A, p, p), D.dist_row_csr_matrix(dctx, A_T, p, p)
    Xd, Yd = D.dist_row_dn_matrix(dctx, X), D.dist_row_dn_matrix(dctx, Y)
    st = dctx.ctx.cuda_streams[0]

    def over_ranks(v):
        t = torch.tensor([v], dtype=torch.float64, device="cpu" if shared_gpu else f"cuda:{dev}")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t[0])

    for mode in args.modes.split(","):
        models = {agg: D.dist_gcn(dctx, Ad, ATd, sizes, fused=True, mode=mode, agg_dtype=agg) for agg in ("f32", "bf16")}
        ms = {agg: [] for agg in models}
        nbytes, exch, loss = {}, {}, {}
        for it in range(args.warmup + args.steps):
            for agg, G in models.items():                              # alternating: both see the same machine state
                beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                dctx.exchange_bytes = 0
                beg.record(st)
                loss[agg], _ = G.train_step(dctx, Xd, Yd, *ADAM)
                end.record(st)
                end.synchronize()
                nbytes[agg] = dctx.exchange_bytes
                if it >= args.warmup:
                    ms[agg].append(beg.elapsed_time(end))
        dctx.profile_exchange = True                                   # the exchange timers: a pass of their own
        for agg, G in models.items():
            tot = []
            for it in range(3):
                G.train_step(dctx, Xd, Yd, *ADAM)
                if it:
                    tot.append(sum(dctx.measure(k) for k in list(dctx.ctx.timers) if k.endswith("matmul-exchange")))
            exch[agg] = float(np.mean(tot))
        dctx.profile_exchange = False
        for agg, G in models.items():
            buf = G.bcast_buffer.numel() * G.bcast_buffer.element_size() + G.bcast_buffer2.numel() * G.bcast_buffer2.element_size()
            e, x = over_ranks(float(np.median(ms[agg]))), over_ranks(exch[agg])
            say(f"mode={mode:9s} agg={agg:4s}: exchange_bytes/epoch {nbytes[agg]:>12d}  receive buffers {buf / 1e6:8.2f} MB  "
                f"exchange {x:8.3f} ms  epoch {e:8.3f} ms  loss {loss[agg]:.4f}")
        say(f"mode={mode:9s} bf16 / f32: exchange bytes {nbytes['bf16'] / max(nbytes['f32'], 1):.3f}")
        del models
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--ranks", type=int, default=0, help="ranks sharing cuda:0 over gloo (with --gpus 1); default 2")
    ap.add_argument("--scale", type=float, default=1.0, help="share of the Reddit shape")
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--modes", default="allgather,halo,rounds")
    args = ap.parse_args()
    import torch.multiprocessing as mp
    shared = args.gpus == 1
    P = (args.ranks or 2) if shared else args.gpus
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    mp.spawn(_rank_main, args=(P, port, args, shared), nprocs=P, join=True)


if __name__ == "__main__":
    main()
