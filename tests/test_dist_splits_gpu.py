"""Split-aware training on the row partition: dist_gcn.set_splits with gloo ranks sharing one GPU, as test_dist_gpu.py
starts them.  Judged against oracle.Gcn(f64acc=True) with the class count padded to a multiple of P (src/main.cpp:135),
its loss taken over n_train and its gradient rows outside the training split zeroed, at the bars of test_dist_gpu.py.
One rank of three holds no training row."""
import datetime
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest

from test_dist_gpu import ROOT, _data, _free_port
from test_gpu_splits import _oracle_split_epoch

pytestmark = pytest.mark.gpu

N, F, C, HIDDEN, EPOCHS = 1536, 20, 5, [16, 16], 3
NAMES = ("train", "val", "test", "other")


def _sets(P):
    """drawn after X and Y like test_gpu_splits.py; the middle third (rank 1 of 3) trains on nothing"""
    rng = np.random.default_rng(22)
    rng.standard_normal((N, F), dtype=np.float32)
    rng.integers(0, C, size=(N, 1))
    S = rng.choice(4, size=N, p=(0.5, 0.2, 0.25, 0.05)).astype(np.int32)
    mid = slice(N // 3, 2 * N // 3)
    S[mid] = np.where(S[mid] == 0, 1, S[mid])
    return S


def _worker(rank, P, port, mode, train_set, S, q, resync):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=P, timeout=datetime.timedelta(seconds=240))
    try:
        pkg, (ip, ix, dv), X, Y = _data(N, F, C)
        D = pkg.dist
        dctx = D.dist_context(overlap=True, device_index=0)
        A = pkg.csr_matrix(ip, ix, dv, N)
        A.normalize(True)
        A_T = A.transpose()
        p = D.partition_bounds(N, P)
        sizes = [F] + HIDDEN + [(C + P - 1) // P * P]
        G = D.dist_gcn(dctx, D.dist_row_csr_matrix(dctx, A, p, p, None), D.dist_row_csr_matrix(dctx, A_T, p, p, None),
                       sizes, fused=True, mode=mode)
        Xd, Yd = D.dist_row_dn_matrix(dctx, X), D.dist_row_dn_matrix(dctx, Y)
        G.set_splits(dctx, D.dist_row_dn_matrix(dctx, S.reshape(-1, 1)), train_set)
        local_train = int((S[p[rank]:p[rank + 1]] == train_set).sum())
        out = []
        for ep in range(EPOCHS):
            if ep == EPOCHS - 1:                        # the last epoch through the one-sync step
                la = G.train_step(dctx, Xd, Yd, 1e-2, 0.9, 0.999, 5e-4, 1e-8)
                out.append((la, G.split_metrics(), None, None))
                continue
            la = G.train_forward(dctx, Xd, Yd)
            met = G.split_metrics()
            G.backward(dctx)
            dctx.sync()
            grads = [l.GW().local.numpy().copy() for l in G.layers()]
            gb = [l.Gb().local.numpy().copy() for l in G.layers()]
            G.adam_update(dctx, 1e-2, 0.9, 0.999, 5e-4, 1e-8)
            dctx.sync()
            out.append((la, met, grads, gb))
            for l, (W, b) in zip(G.layers(), resync[ep]):
                assert np.abs(l.W().local.numpy() - W).max() <= 2.05e-2
                assert np.abs(l.b().local.numpy() - b).max() <= 2.05e-2
                l.W().local.init(W)
                l.b().local.init(b)
            dctx.sync()
        q.put((rank, out, local_train))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("P,mode,train_set", [(2, "allgather", 0), (3, "allgather", 0), (2, "halo", 0), (3, "halo", 2),
                                              (2, "rounds", 0)])
def test_dist_gcn_with_splits_matches_oracle(oracle, P, mode, train_set):
    _, (ip, ix, dv), X, Y = _data(N, F, C)
    S = _sets(P)
    Cp = (C + P - 1) // P * P
    O = oracle.Gcn(oracle.Csr(ip.copy(), ix.copy(), dv.copy(), N), [F] + HIDDEN + [Cp], f64acc=True)
    want, resync = [], []
    for _ in range(EPOCHS):
        per, grads = _oracle_split_epoch(oracle, O, X, Y, S, train_set)
        want.append((per, grads))
        O.adam_update()
        resync.append([(l.lin.W.copy(), l.lin.b.copy()) for l in O.layers])
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, P, port, mode, train_set, S, q, resync)) for r in range(P)]
    for pr in procs:
        pr.start()
    try:
        res = sorted([q.get(timeout=300) for _ in range(P)], key=lambda t: t[0])
        for pr in procs:
            pr.join(timeout=60)
            assert pr.exitcode == 0
    finally:                                  # a rank that never met the others must not outlive the test
        for pr in procs:
            if pr.is_alive():
                pr.terminate()
                pr.join(timeout=30)
    if P == 3 and train_set == 0:
        assert res[1][2] == 0 and res[0][2] > 0                           # a rank without a training row
    for rank, out, _ in res:
        for e, ((la, met, grads, gb), (per, ograds)) in enumerate(zip(out, want)):
            assert la == met[NAMES[train_set]]
            for name in NAMES:
                ol, oa, cnt = per[name]
                loss, acc = met[name]
                print(f"[dist splits] P={P} {mode} rank {rank} epoch {e} {name}: loss {loss!r} (oracle {ol!r}), "
                      f"acc {acc!r} (oracle {oa!r}), {cnt} rows")
                assert abs(loss - ol) <= 1e-4 * abs(ol), (rank, e, name, loss, ol)
                assert abs(acc - oa) <= 3.0 / cnt, (rank, e, name, acc, oa)
                assert met["counts"][name] == cnt
            if grads is None:
                continue
            for g, b, (ow, ob) in zip(grads, gb, ograds):
                assert np.abs(g - ow).max() <= 1e-4 * np.abs(ow).max(), (rank, e)
                assert np.abs(b.reshape(-1) - ob.reshape(-1)).max() <= 1e-4 * np.abs(ob).max(), (rank, e)
        assert out[-1][0][0] < out[0][0][0]                                # the training split's loss falls
    for rank, out, _ in res[1:]:                                           # every rank reports the same eight numbers
        for e in range(EPOCHS):
            assert out[e][0] == res[0][1][e][0] and out[e][1] == res[0][1][e][1], (rank, e)
