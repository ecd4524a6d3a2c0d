"""Dropout on the row partition (dist_gcn(dropout=p)): every rank drops ITS rows of the mask the single-GPU model draws,
so the reference is the oracle's P-shard simulation wrapped with the GLOBAL mask (dropout_ref.oracle_dropout: row0 =
p[rank]), at the bars of test_dist_gpu.py.  Fresh spawned children share the one GPU over gloo, as in test_dist_gpu.py; a
child never raises between two collectives (its peers would wait for it): it collects what it found and reports at the end."""
import traceback

import numpy as np
import pytest

import dropout_ref
from test_dist_gpu import _assert_epochs_match, _data, _oracle_epochs
from test_gpu_dist_bf16 import _init, _spawn

pytestmark = pytest.mark.gpu
ADAM = (1e-2, 0.9, 0.999, 5e-4, 1e-8)
P_DROP, SEED = 0.5, 0xC0FFEE1234567


def _worker(rank, P, port, n, F, C, hidden, mode, epochs, overlap, resync, q):
    """test_dist_gpu._worker with dropout: per epoch (loss, acc, [G_W], [G_b]), the last epoch through train_step; the
    parameters continue from the oracle's after every epoch (a step farther than an Adam sign flip is reported)"""
    dist = _init(rank, P, port)
    try:
        pkg, (ip, ix, dv), X, Y = _data(n, F, C)
        D = pkg.dist
        dctx = D.dist_context(overlap=overlap, device_index=0)
        A = pkg.csr_matrix(ip, ix, dv, n)
        A.normalize(True)
        A_T = A.transpose()
        p = D.partition_bounds(n, P)
        sizes = [F] + hidden + [(C + P - 1) // P * P]
        G = D.dist_gcn(dctx, D.dist_row_csr_matrix(dctx, A, p, p), D.dist_row_csr_matrix(dctx, A_T, p, p), sizes,
                       fused=True, mode=mode, dropout=P_DROP)
        G.set_dropout(P_DROP, SEED, 0)
        Xd, Yd = D.dist_row_dn_matrix(dctx, X), D.dist_row_dn_matrix(dctx, Y)
        out, bad = [], []
        if [l.row0 for l in G.layers()] != [p[rank]] * len(G.layers()):
            bad.append(("row0", [l.row0 for l in G.layers()]))
        for ep in range(epochs):
            if ep == epochs - 1 and epochs > 1:         # last epoch through the one-sync step
                loss, acc = G.train_step(dctx, Xd, Yd, *ADAM)
                out.append((loss, acc, None, None))
                continue
            loss, acc = G.train_forward(dctx, Xd, Yd)
            G.backward(dctx)
            dctx.sync()
            grads = [l.GW().local.numpy().copy() for l in G.layers()]
            gb = [l.Gb().local.numpy().copy() for l in G.layers()]
            G.adam_update(dctx, *ADAM)
            dctx.sync()
            out.append((loss, acc, grads, gb))
            for li, (l, (W, b)) in enumerate(zip(G.layers(), resync[ep])):
                if np.abs(l.W().local.numpy() - W).max() > 2.05e-2 or np.abs(l.b().local.numpy() - b).max() > 2.05e-2:
                    bad.append(("more than a sign flip", ep, li))
                l.W().local.init(W)
                l.b().local.init(b)
            dctx.sync()
        if G.dropout_epoch != epochs:
            bad.append(("dropout_epoch", G.dropout_epoch))
        def plain():
            H = G(dctx, Xd)
            dctx.sync()
            return H.local.numpy().copy()
        clean, again = plain(), plain()                           # a plain call never drops: twice the same bits
        if not np.array_equal(clean.view(np.uint32), again.view(np.uint32)) or G.dropout_epoch != epochs:
            bad.append(("a plain forward dropped",))
        q.put((rank, out, bad, None))
    except Exception:
        q.put((rank, None, None, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("P,mode,overlap", [(2, "allgather", True), (2, "halo", True), (2, "rounds", True),
                                            (4, "allgather", True), (2, "allgather", False)])
def test_dist_dropout_matches_the_globally_masked_oracle(oracle, P, mode, overlap):
    n, F, C, hidden, epochs = 1536, 20, 5, [16, 16], 3
    _, (ip, ix, dv), X, Y = _data(n, F, C)
    O = oracle.DistGcn(oracle.Csr(ip, ix, dv, n), [F] + hidden + [C], P)
    dropout_ref.oracle_dropout(O, P_DROP, seed=SEED)
    want, resync = _oracle_epochs(O, X, Y, epochs)
    plain = oracle.DistGcn(oracle.Csr(ip, ix, dv, n), [F] + hidden + [C], P)
    assert abs(plain.train_forward(X, Y)[0] - want[0][0]) > 1e-4 * abs(want[0][0])      # the masks matter at this bar
    res = _spawn(_worker, P, (n, F, C, hidden, mode, epochs, overlap, resync))
    for rank, out, bad, err in res:
        assert err is None, err
        assert not bad, (rank, bad)
        _assert_epochs_match(rank, out, want, n)
    for r in range(1, P):
        for e in range(epochs):
            assert res[r][1][e][0] == res[0][1][e][0]                       # same global loss on every rank
