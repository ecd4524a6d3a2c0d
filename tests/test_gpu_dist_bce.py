"""Multi-label training on the row partition (dist_gcn(loss="bce")): the loss is row-local, so every rank runs the pass on
its rows of the single-GPU run and the reference is the wrapped SINGLE-GPU oracle (bce_ref.oracle_bce; the class count
is a multiple of P, so nothing is padded).  The sixteen sums ride on the last layer's gradient all-reduce in train_step
(a 16-float tail on that layer only).  Fresh spawned children share the one GPU over gloo, as in test_dist_gpu.py; a child
never raises between two collectives (its peers would wait for it): it collects what it found and reports at the end."""
import os
import sys
import traceback

import numpy as np
import pytest

import bce_ref as ref
import layernorm_ref
from test_dist_gpu import _data
from test_gpu_dist_bf16 import _init, _spawn

pytestmark = pytest.mark.gpu
ADAM = layernorm_ref.ADAM
TOL = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker(rank, P, port, n, F, C, hidden, mode, epochs, overlap, resync, q):
    """per epoch (loss, f1, gradients or None, the sixteen global sums, split_metrics()), the last epoch through
    train_step; after every Adam step the parameters are checked against the oracle's up to a sign flip and continued
    from the oracle's"""
    dist = _init(rank, P, port)
    try:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        pkg = _data(n, F, C)[0]
        (ip, ix, dv), X, T, S = ref.model_data(pkg, n, F, C)
        D = pkg.dist
        dctx = D.dist_context(overlap=overlap, device_index=0)
        A = pkg.csr_matrix(ip, ix, dv, n)
        A.normalize(True)
        A_T = A.transpose()
        p = D.partition_bounds(n, P)
        sizes = [F] + hidden + [C]
        Ad, A_Td = D.dist_row_csr_matrix(dctx, A, p, p), D.dist_row_csr_matrix(dctx, A_T, p, p)
        G = D.dist_gcn(dctx, Ad, A_Td, sizes, fused=True, mode=mode, loss="bce")
        out, bad = [], []
        tails = [l.lin.tail.numel() for l in G.layers()]
        if tails != [8] * len(hidden) + [16]:
            bad.append(("only the last layer's tail holds sixteen floats", tails))
        soft = D.dist_gcn(dctx, Ad, A_Td, sizes, fused=True, mode=mode)
        if [l.lin.tail.numel() for l in soft.layers()] != [8] * (len(hidden) + 1):
            bad.append(("a softmax model keeps its 8-float tails", [l.lin.tail.numel() for l in soft.layers()]))
        del soft
        G.set_splits(dctx, S[p[rank]:p[rank + 1]], 0)
        Xd, Td = D.dist_row_dn_matrix(dctx, X), D.dist_row_dn_matrix(dctx, T)
        for ep in range(epochs):
            if ep == epochs - 1 and epochs > 1:         # last epoch through the one-sync step
                loss, f1 = G.train_step(dctx, Xd, Td, *ADAM)
                out.append((loss, f1, None, G.loss_layer.global_sums.copy(), G.split_metrics()))
                continue
            loss, f1 = G.train_forward(dctx, Xd, Td)
            sums, metrics = G.loss_layer.global_sums.copy(), G.split_metrics()
            G.backward(dctx)
            dctx.sync()
            grads = {"G_W": [l.GW().local.numpy().copy() for l in G.layers()],
                     "G_b": [l.Gb().local.numpy().copy() for l in G.layers()]}
            G.adam_update(dctx, *ADAM)
            dctx.sync()
            out.append((loss, f1, grads, sums, metrics))
            for li, (l, (W, b)) in enumerate(zip(G.layers(), resync[ep])):
                for mine, theirs in ((l.W().local, W), (l.b().local, b)):
                    if np.abs(mine.numpy() - theirs).max() > 2.05e-2:
                        bad.append(("more than a sign flip", ep, li, mine.shape()))
                    mine.init(theirs)
            dctx.sync()
        q.put((rank, out, bad, None))
    except Exception:
        q.put((rank, None, None, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def _oracle_epochs(O, B, X, T, epochs):
    want, resync = [], []
    for _ in range(epochs):
        ol, of1 = O.train_forward(X, T)
        O.backward()
        want.append((ol, of1, {"G_W": [l.lin.G_W.copy() for l in O.layers], "G_b": [l.lin.G_b.copy() for l in O.layers]},
                     dict(B.per)))
        O.adam_update()
        resync.append([(l.lin.W.copy(), l.lin.b.copy()) for l in O.layers])
    return want, resync


@pytest.mark.parametrize("P,mode,overlap", [(2, "allgather", True), (2, "halo", True), (2, "rounds", True),
                                            (4, "allgather", True), (2, "allgather", False)])
def test_dist_bce_matches_the_wrapped_single_gpu_oracle(pkg, oracle, P, mode, overlap):
    n, F, C, hidden, epochs = 1536, 20, 8, [16, 16], 3
    assert C % P == 0
    (ip, ix, dv), X, T, S = ref.model_data(pkg, n, F, C)
    sizes = [F] + hidden + [C]
    O = oracle.Gcn(oracle.Csr(ip, ix, dv, n), sizes, f64acc=True)
    B = ref.oracle_bce(oracle, O, T, S, 0)
    want, resync = _oracle_epochs(O, B, X, T, epochs)
    res = _spawn(_worker, P, (n, F, C, hidden, mode, epochs, overlap, resync))
    for rank, out, bad, err in res:
        assert err is None, err
        assert not bad, (rank, bad)
        for e, ((loss, f1, grads, sums, metrics), (ol, of1, og, per)) in enumerate(zip(out, want)):
            print(f"[dist bce] P={P} {mode} rank {rank} epoch {e}: loss {loss!r} oracle {ol!r}, f1 {f1!r} oracle {of1!r}")
            assert abs(loss - ol) <= TOL * abs(ol), (rank, e, loss, ol)
            assert metrics["train"] == (loss, f1)
            for nm in ("train", "val", "test"):
                wl, _, wc, rows = per[nm]
                assert metrics["counts"][nm] == rows and abs(metrics[nm][0] - wl) <= TOL * abs(wl), (rank, e, nm)
                assert all(abs(a - b) <= 3 for a, b in zip(metrics["confusion"][nm], wc)), (rank, e, nm, metrics["confusion"][nm], wc)
            assert sums.shape == (16,)
            if grads is None:
                continue
            for what in ("G_W", "G_b"):                                         # all-reduced: the global gradient on every rank
                for li, (g, w) in enumerate(zip(grads[what], og[what])):
                    err_ = layernorm_ref.relerr(g, w)
                    assert err_ <= TOL, (rank, e, what, li, err_)
    for r in range(1, P):
        for e in range(epochs):
            mine, first = res[r][1][e], res[0][1][e]
            assert np.array_equal(mine[3].view(np.uint32), first[3].view(np.uint32)), (r, e, mine[3], first[3])   # the sixteen sums
            assert repr(mine[4]) == repr(first[4]), (r, e)                      # split_metrics(), nan included
            assert mine[0] == first[0] and mine[1] == first[1]
