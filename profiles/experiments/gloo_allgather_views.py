"""Forms of a gloo all-gather of [rows x d] fp32 host shards (the rehearsals' all-gather schedule, dist.gloo_all_gather_rows),
CPU only, P processes on loopback; ms per call, mean of 50 after one warm-up.  Every form yields one [P*rows x d] tensor.
Usage: python profiles/experiments/gloo_allgather_views.py <rows> <d> <P> [intra-op threads per rank]"""
import os
import sys
import time

import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def main(rank, P, rows, d, threads):
    if threads:
        torch.set_num_threads(threads)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29751")
    dist.init_process_group("gloo", rank=rank, world_size=P)
    x = torch.randn(rows, d)

    def t(fn, n=50):
        fn()
        dist.barrier()
        s = time.perf_counter()
        for _ in range(n):
            fn()
        return (time.perf_counter() - s) / n * 1e3

    def into_tensor():
        dist.all_gather_into_tensor(torch.empty(P * rows, d), x)

    def list_cat():
        ps = [torch.empty(rows, d) for _ in range(P)]
        dist.all_gather(ps, x)
        torch.cat(ps, 0)

    def list_views():
        o = torch.empty(P * rows, d)
        dist.all_gather(list(o.split(rows)), x)

    def broadcasts_views():
        o = torch.empty(P * rows, d)
        for i in range(P):
            v = o[i * rows:(i + 1) * rows]
            if rank == i:
                v.copy_(x)
            dist.broadcast(v, src=i)

    def broadcasts_views_np():
        o = torch.empty(P * rows, d)
        for i in range(P):
            v = o[i * rows:(i + 1) * rows]
            if rank == i:
                v.numpy()[...] = x.numpy()
            dist.broadcast(v, src=i)

    r = {k: round(t(f), 3) for k, f in (("P broadcasts into views, numpy own copy", broadcasts_views_np), ("all_gather_into_tensor", into_tensor), ("all_gather(list)+cat", list_cat),
                                         ("all_gather(list of views)", list_views), ("P broadcasts into views", broadcasts_views))}
    if rank == 0:
        print(f"torch {torch.__version__} P={P} rows={rows} d={d} intra-op threads={torch.get_num_threads()}", r, flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    rows, d, P = (int(a) for a in sys.argv[1:4])
    threads = int(sys.argv[4]) if len(sys.argv) > 4 else 0
    mp.spawn(main, args=(P, rows, d, threads), nprocs=P)
