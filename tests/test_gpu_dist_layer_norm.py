"""Layer normalisation on the row partition (dist_gcn(norm="layer")): it is row-local, so every rank normalises exactly
its rows of the single-GPU run and the reference is the wrapped SINGLE-GPU oracle (layernorm_ref.oracle_layer_norm; the
class count is a multiple of P, so nothing is padded).  gamma / beta are replicated; their gradients ride on the
all-reduce of the same layer's G_W / G_b.  Fresh spawned children share the one GPU over gloo, as in test_dist_gpu.py; a
child never raises between two collectives (its peers would wait for it): it collects what it found and reports at the end."""
import traceback

import numpy as np
import pytest

import layernorm_ref as ref
from test_dist_gpu import _data
from test_gpu_dist_bf16 import _init, _spawn

pytestmark = pytest.mark.gpu
ADAM = ref.ADAM
TOL = 1e-4
GRADS = ("G_W", "G_b", "G_gamma", "G_beta")


def _worker(rank, P, port, n, F, C, hidden, mode, epochs, overlap, resync, q):
    """per epoch (loss, acc, {gradient name: [per layer]}), the last epoch through train_step; after every Adam step the
    parameters (gamma and beta included) are reported, checked against the oracle's up to a sign flip and continued from
    the oracle's"""
    dist = _init(rank, P, port)
    try:
        pkg, (ip, ix, dv), X, Y = _data(n, F, C)
        D = pkg.dist
        dctx = D.dist_context(overlap=overlap, device_index=0)
        A = pkg.csr_matrix(ip, ix, dv, n)
        A.normalize(True)
        A_T = A.transpose()
        p = D.partition_bounds(n, P)
        sizes = [F] + hidden + [C]
        G = D.dist_gcn(dctx, D.dist_row_csr_matrix(dctx, A, p, p), D.dist_row_csr_matrix(dctx, A_T, p, p), sizes,
                       fused=True, mode=mode, norm="layer")
        out, bad, params = [], [], []
        if [l.norm is not None for l in G.layers()] != [True] * len(hidden) + [False]:
            bad.append(("which layers have a norm", [l.norm is not None for l in G.layers()]))
        for li, l in enumerate(G.layers()[:-1]):
            g, b = ref.params(l.AHW.m(), 5 + li)                    # oracle_layer_norm's
            l.norm.gamma.init(g)
            l.norm.beta.init(b)
            if l.norm.xhat.shape() != (p[rank + 1] - p[rank], l.AHW.m()):
                bad.append(("xhat holds this rank's rows", li, l.norm.xhat.shape()))
        Xd, Yd = D.dist_row_dn_matrix(dctx, X), D.dist_row_dn_matrix(dctx, Y)
        for ep in range(epochs):
            if ep == epochs - 1 and epochs > 1:         # last epoch through the one-sync step
                loss, acc = G.train_step(dctx, Xd, Yd, *ADAM)
                out.append((loss, acc, None))
                continue
            loss, acc = G.train_forward(dctx, Xd, Yd)
            G.backward(dctx)
            dctx.sync()
            grads = {"G_W": [l.GW().local.numpy().copy() for l in G.layers()],
                     "G_b": [l.Gb().local.numpy().copy() for l in G.layers()],
                     "G_gamma": [l.norm.G_gamma.numpy().copy() for l in G.layers()[:-1]],
                     "G_beta": [l.norm.G_beta.numpy().copy() for l in G.layers()[:-1]]}
            G.adam_update(dctx, *ADAM)
            dctx.sync()
            out.append((loss, acc, grads))
            params.append([(l.norm.gamma.numpy().copy(), l.norm.beta.numpy().copy()) for l in G.layers()[:-1]])
            for li, (l, (W, b, gamma, beta)) in enumerate(zip(G.layers(), resync[ep])):
                pairs = [(l.W().local, W), (l.b().local, b)] + ([(l.norm.gamma, gamma), (l.norm.beta, beta)] if gamma is not None else [])
                for mine, theirs in pairs:
                    if np.abs(mine.numpy() - theirs).max() > 2.05e-2:
                        bad.append(("more than a sign flip", ep, li, mine.shape()))
                    mine.init(theirs)
            dctx.sync()
        # row-local: this rank's rows through ops.layer_norm alone are the bits they have in the whole matrix
        m = hidden[0]
        Z = np.random.default_rng(77).standard_normal((n, m), dtype=np.float32)
        g, b = (pkg.dn_matrix.from_numpy(a, dctx.ctx.device) for a in ref.params(m, 5))
        res = []
        for rows in (Z, Z[p[rank]:p[rank + 1]]):
            dn = lambda r, c: pkg.dn_matrix(r, c, device=dctx.ctx.device)
            Zd, xhat, rstd = pkg.dn_matrix.from_numpy(rows, dctx.ctx.device), dn(rows.shape[0], m), dn(rows.shape[0], 1)
            pkg.ops.layer_norm(dctx.ctx, Zd, Zd, xhat, rstd, g, b, pkg.ops.LAYER_NORM_LEAKY_RELU)
            dctx.sync()
            res.append((Zd.numpy(), xhat.numpy(), rstd.numpy()))
        for what, whole, shard in zip(("y", "xhat", "rstd"), res[0], res[1]):
            if not np.array_equal(whole[p[rank]:p[rank + 1]].view(np.uint32), shard.view(np.uint32)):
                bad.append(("the shard's rows are not the whole matrix's", what))
        q.put((rank, out, bad, params, None))
    except Exception:
        q.put((rank, None, None, None, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def _oracle_epochs(O, X, Y, epochs):
    """the wrapped single-GPU oracle's own run: per epoch (loss, acc, gradients) and the parameters after its Adam step"""
    want, resync = [], []
    for _ in range(epochs):
        ol, oa = O.train_forward(X, Y)
        O.backward()
        want.append((ol, oa, {"G_W": [l.lin.G_W.copy() for l in O.layers], "G_b": [l.lin.G_b.copy() for l in O.layers],
                              "G_gamma": [l.norm.G_gamma.copy() for l in O.layers[:-1]],
                              "G_beta": [l.norm.G_beta.copy() for l in O.layers[:-1]]}))
        O.adam_update()
        resync.append([(l.lin.W.copy(), l.lin.b.copy()) + ((l.norm.gamma.copy(), l.norm.beta.copy()) if hasattr(l, "norm")
                                                           else (None, None)) for l in O.layers])
    return want, resync


@pytest.mark.parametrize("P,mode,overlap", [(2, "allgather", True), (2, "halo", True), (2, "rounds", True),
                                            (4, "allgather", True), (2, "allgather", False)])
def test_dist_layer_norm_matches_the_wrapped_single_gpu_oracle(oracle, P, mode, overlap):
    n, F, C, hidden, epochs = 1536, 20, 8, [16, 16], 3
    assert C % P == 0
    _, (ip, ix, dv), X, Y = _data(n, F, C)
    sizes = [F] + hidden + [C]
    O = oracle.Gcn(oracle.Csr(ip, ix, dv, n), sizes)
    ref.oracle_layer_norm(oracle, O)
    want, resync = _oracle_epochs(O, X, Y, epochs)
    plain = oracle.Gcn(oracle.Csr(ip, ix, dv, n), sizes)
    assert abs(plain.train_forward(X, Y)[0] - want[0][0]) > 100 * TOL * abs(want[0][0])      # the norm matters at this bar
    res = _spawn(_worker, P, (n, F, C, hidden, mode, epochs, overlap, resync))
    for rank, out, bad, params, err in res:
        assert err is None, err
        assert not bad, (rank, bad)
        for e, ((loss, acc, grads), (ol, oa, og)) in enumerate(zip(out, want)):
            assert abs(loss - ol) <= TOL * abs(ol), (rank, e, loss, ol)
            assert abs(acc - oa) <= 3.0 / n, (rank, e, acc, oa)
            if grads is None:
                continue
            for what in GRADS:                                                  # all-reduced: the global gradient on every rank
                assert len(grads[what]) == len(og[what])
                for li, (g, w) in enumerate(zip(grads[what], og[what])):
                    err_ = ref.relerr(g, w)
                    assert err_ <= TOL, (rank, e, what, li, err_)
    for r in range(1, P):
        for e in range(epochs):
            assert res[r][1][e][0] == res[0][1][e][0]                           # same global loss on every rank
        for mine, first in zip(res[r][3], res[0][3]):                           # gamma / beta stay replicas after Adam
            for (g, b), (g0, b0) in zip(mine, first):
                assert np.array_equal(g.view(np.uint32), g0.view(np.uint32)) and np.array_equal(b.view(np.uint32), b0.view(np.uint32))
