"""The row-partitioned GAT on the device (mg-gcn_amd/dist_gat.py): dist_attention against the single-GPU attention bit
for bit at P = 1, 2, 4, the model against the reference model of gat_ref.py, and dist_gat at P = 1 against gat bit for bit --
over gloo, and over ProcessGroupNCCL with the self-gather on, where the exchange really runs on the comm stream.

Multi-rank cases: fresh spawned children that share the one GPU over gloo (at most four, next to the parent), started with
_init / _spawn of test_gpu_dist_bf16.py.  A child never raises between two collectives (its peers would wait for it): it
collects what it found and reports at the end.

G_att with attention dropout has no bar of its own in gat_dropout_ref.py.  G_att[0] = sum_i ds_dst[i, k] Z[i, c] and
G_att[1] = sum_j ds_src[j, k] Z[j, c]: an error of ds_dst within DROP_TOL["ds_dst"] of its scale sd moves G_att[0] by at most
that bar times sum_i sd[i, k] |Z[i, c]|, which is the scale gat_ref.attention gives G_att -- so row 0 is held to
DROP_TOL["ds_dst"] and row 1 to DROP_TOL["ds_src"] on that scale, built from the dropout restatement's own sd and ss."""
import os
import sys
import traceback

import numpy as np
import pytest

import bce_ref
import dist_gat_ref as dgr
import gat_dropout_ref as dref
import gat_ref as ref
from gat_ref import relerr, rowdist
from test_gpu_dist_bf16 import _init, _spawn
from test_gpu_gat import N, TOL, _model_data

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADAM = ref.ADAM
MSEED = 0xC0FFEE123


def _pkg():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as ge
    return ge.load_package()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the operator ------------------------------------------------------------------------------------------------------------------
OP_NAMES = dgr.ROW_NAMES
OP_CASES = [(K, dh, drop) for K, dh in dgr.OP_SHAPES for drop in (False, True)]


def _op_worker(rank, P, port, q):
    """per case: this rank's rows of the host Z and G through dist_attention, the whole graph through attention in the same
    process; reports the outputs that are not the single-GPU rows bit for bit, and the all-reduced G_att"""
    dist = _init(rank, P, port)
    try:
        pkg = _pkg()
        D, dn = pkg.dist, pkg.dn_matrix
        dctx = D.dist_context(overlap=True, device_index=0)
        ctx = dctx.ctx
        indptr, indices = ref.kernel_graph_long()
        n = indptr.size - 1
        F = pkg.csr_matrix(indptr.copy(), indices.copy(), np.ones(indices.size, dtype=np.float32), n)
        A = F.transpose()                                               # F^T: holds the long rows
        p = D.partition_bounds(n, P)
        lo, hi = p[rank], p[rank + 1]
        # F lists its columns in no order: its rows are kept; A is a transpose() output (ascending): the merge of the blocks
        Fb = D.dist_row_csr_matrix(dctx, F, p, p, keep_rows=True).row_block_global()
        FTb = D.dist_row_csr_matrix(dctx, A, p, p).row_block_global()
        bad, gatt = [], {}
        for K, dh, drop in OP_CASES:
            c, _ = dgr.op_case(K, dh, drop)
            d = K * dh
            whole = None if not drop else dref.drop_tuple(dgr.DROP_P, dref.SEED, dref.STREAM, 0, 0)
            mine = None if not drop else dref.drop_tuple(dgr.DROP_P, dref.SEED, dref.STREAM, lo, 0)
            one = pkg.attention("w_", n, n, d, K)
            one.init(c["att"])
            Z1, G1, out1, GZ1 = dn.from_numpy(c["Z"]), dn.from_numpy(c["G"]), dn(n, d), dn(n, d)
            one(ctx, F, Z1, out1, whole)
            one.backward(ctx, F, A, Z1, G1, out1, GZ1, whole)
            part = D.dist_attention(dctx, "p_", n, d, K)
            part.init(c["att"])
            Zl, Gl = dn.from_numpy(c["Z"][lo:hi], ctx.device), dn.from_numpy(c["G"][lo:hi], ctx.device)
            outl, GZl = dn(hi - lo, d), dn(hi - lo, d)
            for _ in range(2):                                          # the second call meets the buffers the first one left
                part(ctx, Fb, Zl, outl, mine)
                part.backward(ctx, Fb, FTb, Zl, Gl, outl, GZl, mine)
            dctx.all_reduce_sum([part.G_att.t])
            ctx.sync()
            got = dict(out=outl, lse=part.lse, D=part.D, ds_dst=part.ds_dst, ds_src=part.ds_src, G_Z=GZl)
            want = dict(out=out1, lse=one.lse, D=one.D, ds_dst=one.ds_dst, ds_src=one.ds_src, G_Z=GZ1)
            for nm in OP_NAMES:
                g, w = _bits(got[nm].numpy()), _bits(want[nm].numpy()[lo:hi])
                if not np.array_equal(g, w):
                    bad.append((K, dh, drop, nm, int((g != w).sum()), float(rowdist(got[nm].numpy(), c["want"][nm][lo:hi], c["scale"][nm][lo:hi]).max())))
            if not np.abs(GZl.numpy()).max() > 0:
                bad.append((K, dh, drop, "G_Z is all zeros"))
            gatt[(K, dh, drop)] = (part.G_att.numpy().copy(), one.G_att.numpy().copy())
        q.put((rank, bad, gatt, None))
    except Exception:
        q.put((rank, None, None, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def _gatt_bars(c, drop):
    """(scale [2 x d], bar per row) of G_att, see the module docstring"""
    if not drop:
        return c["scale"]["G_att"], (ref.ROW_TOL, ref.ROW_TOL)
    K = c["scale"]["ds_dst"].shape[1]
    absZ = np.abs(c["Z"].astype(np.float64)).reshape(c["Z"].shape[0], K, -1)
    ga = np.stack([(c["scale"]["ds_dst"][:, :, None] * absZ).sum(axis=0), (c["scale"]["ds_src"][:, :, None] * absZ).sum(axis=0)])
    return ga.reshape(2, -1), (dref.DROP_TOL["ds_dst"], dref.DROP_TOL["ds_src"])


@pytest.mark.parametrize("P", [1, 2, 4])
def test_dist_attention_gives_the_single_gpu_rows_bit_for_bit(P):
    """kernel_graph_long as F (n = 320) at (4, 32), (3, 7), (1, 260), plain and with attention dropout p = 0.5: out, lse, D,
    ds_dst, ds_src and G_Z of every rank are the single-GPU attention's rows bit for bit; the all-reduced G_att is within the
    row-scaled bar of the restatement and has the same bits on every rank"""
    res = _spawn(_op_worker, P, ())
    for rank, bad, gatt, err in res:
        assert err is None, err
        assert not bad, (rank, bad)
    for K, dh, drop in OP_CASES:
        c, _ = dgr.op_case(K, dh, drop)
        scale, bars = _gatt_bars(c, drop)
        first = res[0][2][(K, dh, drop)][0]
        for rank, _, gatt, _ in res:
            mine, single = gatt[(K, dh, drop)]
            np.testing.assert_array_equal(_bits(mine), _bits(first), err_msg=f"rank {rank} {(K, dh, drop)}")
            for what, g in (("partitioned", mine), ("single", single)):
                dist_ = rowdist(g, c["want"]["G_att"], scale)
                print(f"[dist-gat] P={P} rank {rank} K={K} dh={dh} drop={drop} G_att {what}: {dist_[0]:.3e}, {dist_[1]:.3e} (bars {bars})")
                assert dist_[0] <= bars[0] and dist_[1] <= bars[1], (what, rank, K, dh, drop, dist_)


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def _state(G):
    """every parameter, gradient and Adam moment of a dist_gat, as bits"""
    out = []
    for l in G.layers():
        ts = [l.W().local, l.b().local, l.att().local, l.GW().local, l.Gb().local, l.Gatt().local,
              l.lin.mW, l.lin.vW, l.lin.mb, l.lin.vb, l.attn.m, l.attn.v]
        out.append([None if t is None else _bits(t.numpy()).copy() for t in ts])
    return out


def _model_worker(rank, P, port, cfg, resync, q):
    """three epochs, the last through train_step: per epoch (result, gradient buffers -- read before Adam, after it in the
    train_step epoch --, parameters after Adam, split_metrics, the state's bits); after every epoch the parameters are checked against the reference's up to a sign flip and continued
    from the reference's.  Also the bytes the first epoch handed to the exchange"""
    dist = _init(rank, P, port)
    try:
        pkg = _pkg()
        D = pkg.dist
        sizes, heads = cfg["sizes"], cfg["heads"]
        (ip, ix, dv), X, Y = _model_data(pkg, sizes, seed=cfg.get("data_seed", 0))
        targets = cfg.get("T", Y)
        dctx = D.dist_context(overlap=cfg["overlap"], device_index=0)
        A = pkg.csr_matrix(ip.copy(), ix.copy(), dv.copy(), N)
        A_T = A.transpose()
        p = D.partition_bounds(N, P)
        G = D.dist_gat(dctx, D.dist_row_csr_matrix(dctx, A, p, p, keep_rows=True), D.dist_row_csr_matrix(dctx, A_T, p, p), sizes, heads=heads,
                       loss=cfg.get("loss", "softmax"), dropout=cfg.get("p", 0.0), attn_dropout=cfg.get("attn", 0.0))
        if "p" in cfg:
            G.set_dropout(cfg["p"], seed=MSEED, epoch=4)
        S = cfg.get("S")
        if S is not None:
            G.set_splits(dctx, S[p[rank]:p[rank + 1]].copy())
        Xd, Yd = D.dist_row_dn_matrix(dctx, X), D.dist_row_dn_matrix(dctx, targets)
        out, bad, nbytes = [], [], None
        for ep in range(3):
            dctx.exchange_bytes = 0
            if ep == 2:                                                 # the one-sync step
                res = G.train_step(dctx, Xd, Yd, *ADAM)
            else:
                res = G.train_forward(dctx, Xd, Yd)
                G.backward(dctx)
                dctx.sync()
            nbytes = int(dctx.exchange_bytes) if ep == 0 else nbytes
            metrics = G.split_metrics() if S is not None else None
            grads = [(l.GW().local.numpy().copy(), l.Gb().local.numpy().copy(), l.Gatt().local.numpy().copy()) for l in G.layers()]
            if ep != 2:
                G.adam_update(dctx, *ADAM)
                dctx.sync()
            params = [(l.W().local.numpy().copy(), l.b().local.numpy().copy(), l.att().local.numpy().copy()) for l in G.layers()]
            out.append((res, grads, params, metrics, _state(G)))
            for li, (l, theirs) in enumerate(zip(G.layers(), resync[ep])):
                for nm, mine, t in zip(("W", "b", "att"), (l.W().local, l.b().local, l.att().local), theirs):
                    if np.abs(mine.numpy() - t).max() > 2.05 * ADAM[0]:
                        bad.append(("more than a sign flip", ep, li, nm))
                    mine.init(t)
            dctx.sync()
        q.put((rank, out, bad, nbytes, None))
    except Exception:
        q.put((rank, None, None, None, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def _reference_epochs(O, X, Y, epochs=3):
    """the reference's own epochs: per epoch (result, gradients, the gradient buffers after Adam), and its parameters after
    every Adam step.  Adam adds the weight decay to G_W and G_att in place, in the reference as on the device, so after a
    train_step the buffers hold the decayed gradients: the last epoch is compared with those"""
    want, resync = [], []
    for _ in range(epochs):
        res = O.train_forward(X, Y)
        O.backward()
        grads = _reference_grads(O)
        O.adam_update()
        want.append((res, grads, _reference_grads(O)))
        resync.append([(l.lin.W.copy(), l.lin.b.copy(), l.att.copy()) for l in O.layers])
    return want, resync


def _reference_grads(O):
    return [(l.lin.G_W.copy(), l.lin.G_b.copy(), l.G_att.copy()) for l in O.layers]


def _assert_model(P, res, want, n_acc, exact_score=False):
    for rank, out, bad, nbytes, err in res:
        assert err is None, err
        assert not bad, (rank, bad)
        for e, ((got, grads, params, metrics, state), (wres, before, after)) in enumerate(zip(out, want)):
            wgrads = after if e == 2 else before                        # epoch 2 is a train_step: read after its Adam
            print(f"[dist-gat] P={P} rank {rank} epoch {e}: {got!r} (reference {wres!r})")
            assert np.isfinite(wres[0]), "the reference overflowed: the input is outside its range"
            assert abs(got[0] - wres[0]) <= TOL * abs(wres[0]), (rank, e, got, wres)
            assert got[1] == wres[1] or abs(got[1] - wres[1]) <= 3.0 / n_acc, (rank, e, got, wres)
            for li, (g, w) in enumerate(zip(grads, wgrads)):
                for nm, a, b in zip(("G_W", "G_b", "G_att"), g, w):
                    d = relerr(a, b)
                    print(f"[dist-gat]   epoch {e} layer {li} {nm}: {d:.3e}")
                    assert d <= TOL, (rank, e, li, nm, d)
    for rank, out, _, _, _ in res[1:]:                                  # the replicas stay bitwise equal, after every epoch
        for e, (mine, first) in enumerate(zip(out, res[0][1])):
            assert mine[0] == first[0], (rank, e)
            assert repr(mine[3]) == repr(first[3]), (rank, e)
            for li, (a, b) in enumerate(zip(mine[4], first[4])):
                for ti, (x, y) in enumerate(zip(a, b)):
                    assert (x is None) == (y is None) and (x is None or np.array_equal(x, y)), (rank, e, li, ti)
    assert res[0][1][-1][4][0][6] is not None                          # ... the Adam moments among them


def _oracle(oracle, csr, sizes, heads, cls=ref.oracle_gat, **kw):
    ip, ix, dv = csr
    per_layer = [heads] * (len(sizes) - 2) + [1]
    return cls(oracle, oracle.Csr(ip.copy(), ix.copy(), dv.copy(), N), sizes, per_layer, **kw)


@pytest.mark.parametrize("P,overlap,sizes,heads", [(2, True, [48, 32, 32, 7], 4), (2, False, [48, 32, 32, 7], 4),
                                                   (4, True, [48, 32, 32, 7], 4), (4, False, [48, 32, 32, 7], 4),
                                                   (2, True, [16, 64, 8, 5], 2)])
def test_dist_gat_epochs_match_the_reference(pkg, oracle, P, overlap, sizes, heads):
    """n = 1024, three epochs against gat_ref.oracle_gat by the rules of test_gat_epochs_match_the_reference: loss at TOL,
    accuracy within 3 / n, G_W, G_b and G_att at TOL, parameters never more than a sign flip away; the state is bit-equal on
    all ranks after every epoch, and the first epoch hands the exchange the bytes DESIGN.md 3.10 states.  [16, 64, 8, 5] with
    2 heads ends in a layer of dh = 5: the element path, next to two float4 layers of other widths"""
    csr, X, Y = _model_data(pkg, sizes)
    want, resync = _reference_epochs(_oracle(oracle, csr, sizes, heads), X, Y)
    res = _spawn(_model_worker, P, (dict(sizes=sizes, heads=heads, overlap=overlap), resync))
    _assert_model(P, res, want, N)
    for rank, _, _, nbytes, _ in res:
        assert nbytes == dgr.exchange_bytes(N, P, sizes, heads), (rank, nbytes)
    assert res[0][1][-1][0][0] < res[0][1][0][0][0]                     # it trains: the loss of epoch 2 against epoch 0


def test_dist_gat_bce_with_splits_matches_the_reference(pkg, oracle):
    """loss="bce" + set_splits at P = 2 against the reference model under bce_ref.oracle_bce: the training split's loss at
    TOL, every split's loss, row count and confusion counts as test_gpu_dist_bce.py checks them"""
    sizes, heads, P = [48, 32, 32, 7], 4, 2
    csr, X, _ = _model_data(pkg, sizes)
    T = (np.random.default_rng(3).random((N, sizes[-1])) < 0.2).astype(np.int32)
    S = np.random.default_rng(23).choice(3, size=N, p=(0.6, 0.2, 0.2)).astype(np.int32)
    O = _oracle(oracle, csr, sizes, heads)
    B = bce_ref.oracle_bce(oracle, O, T, S, 0)
    want, resync, pers = [], [], []
    for _ in range(3):
        r = O.train_forward(X, T)
        O.backward()
        grads = _reference_grads(O)
        pers.append(dict(B.per))
        O.adam_update()
        want.append((r, grads, _reference_grads(O)))
        resync.append([(l.lin.W.copy(), l.lin.b.copy(), l.att.copy()) for l in O.layers])
    res = _spawn(_model_worker, P, (dict(sizes=sizes, heads=heads, overlap=True, loss="bce", T=T, S=S), resync))
    _assert_model(P, res, want, int((S == 0).sum()))
    for rank, out, _, _, _ in res:
        for e, ((got, _, _, metrics, _), per) in enumerate(zip(out, pers)):
            assert metrics["train"] == got
            for nm in ("train", "val", "test"):
                wl, _, wc, rows = per[nm]
                assert metrics["counts"][nm] == rows and abs(metrics[nm][0] - wl) <= TOL * abs(wl), (rank, e, nm)
                assert all(abs(a - b) <= 3 for a, b in zip(metrics["confusion"][nm], wc)), (rank, e, nm, metrics["confusion"][nm], wc)


def test_dist_gat_dropout_epochs_match_the_reference(pkg, oracle):
    """(dropout, attn_dropout) = (0.5, 0.6) at P = 2 against gat_dropout_ref.oracle_gat_dropout on data seed 2 (the seed at
    which the reference's own loss stays finite), at the bars of test_gat_dropout_epochs_match_the_reference"""
    sizes, heads, P = [48, 32, 32, 7], 4, 2
    csr, X, Y = _model_data(pkg, sizes, seed=2)
    O = _oracle(oracle, csr, sizes, heads, cls=dref.oracle_gat_dropout, p=0.5, attn_p=0.6, seed=MSEED, epoch=4)
    want, resync = _reference_epochs(O, X, Y)
    res = _spawn(_model_worker, P, (dict(sizes=sizes, heads=heads, overlap=True, p=0.5, attn=0.6, data_seed=2), resync))
    _assert_model(P, res, want, N)


# ---- one rank: dist_gat is gat -----------------------------------------------------------------------------------------------------
def _single_state(G):
    out = []
    for l in G.layers():
        ts = [l.W(), l.b(), l.att(), l.GW(), l.Gb(), l.Gatt(), l.lin.mW, l.lin.vW, l.lin.mb, l.lin.vb, l.attn.m, l.attn.v]
        out.append([_bits(t.numpy()).copy() for t in ts])
    return out


def _p1_worker(rank, P, port, backend, q):
    """one rank: dist_gat against gat in one process, three epochs (the last through train_step), fused and per-tensor
    Adam, overlap on and off; over gloo also the checks on dropout that need no second rank"""
    dist = _init(rank, P, port, backend)
    try:
        pkg = _pkg()
        D = pkg.dist
        sizes, heads = [48, 32, 32, 7], 4
        (ip, ix, dv), X, Y = _model_data(pkg, sizes)
        bad = []

        def matrix():
            return pkg.csr_matrix(ip.copy(), ix.copy(), dv.copy(), N)

        def epochs(step3, train_forward, backward, adam, sync):
            res = []
            for ep in range(3):
                if ep == 2:
                    res.append(step3())
                else:
                    res.append(train_forward())
                    backward()
                    adam()
                    sync()
            return res
        for overlap in (True, False):
            dctx = D.dist_context(overlap=overlap, device_index=0)
            ctx = dctx.ctx
            if dctx.self_gather != (backend == "nccl"):
                bad.append(("self_gather", dctx.self_gather))
            A = matrix()
            p = D.partition_bounds(N, 1)
            Ad, ATd = D.dist_row_csr_matrix(dctx, A, p, p, keep_rows=True), D.dist_row_csr_matrix(dctx, A.transpose(), p, p)
            Xd, Yd = D.dist_row_dn_matrix(dctx, X), D.dist_row_dn_matrix(dctx, Y)
            X1, Y1 = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
            for fused in (True, False):
                for kw in (dict(), dict(dropout=0.5, attn_dropout=0.6)):
                    G1 = pkg.gat(matrix(), sizes, heads=heads, fused=fused, **kw)
                    Gd = D.dist_gat(dctx, Ad, ATd, sizes, heads=heads, fused=fused, **kw)
                    if Gd.layers()[0].attn.exchanging != (backend == "nccl"):
                        bad.append(("exchanging", backend))
                    r1 = epochs(lambda: G1.train_step(ctx, X1, Y1, *ADAM), lambda: G1.train_forward(ctx, X1, Y1),
                                lambda: G1.backward(ctx), lambda: G1.adam_update(ctx, *ADAM), ctx.sync)
                    rd = epochs(lambda: Gd.train_step(dctx, Xd, Yd, *ADAM), lambda: Gd.train_forward(dctx, Xd, Yd),
                                lambda: Gd.backward(dctx), lambda: Gd.adam_update(dctx, *ADAM), dctx.sync)
                    if r1 != rd:
                        bad.append((overlap, fused, kw, "results", r1, rd))
                    for li, (a, b) in enumerate(zip(_single_state(G1), _state(Gd))):
                        for ti, (x, y) in enumerate(zip(a, b)):
                            if not np.array_equal(x, y):
                                bad.append((overlap, fused, kw, "state", li, ti, int((x != y).sum())))
                    if not r1[-1][0] < r1[0][0] and not kw:
                        bad.append(("does not train", r1))
        if backend == "gloo":
            # dropout=0, attn_dropout=0 registers no dropout timer (a fresh context: timers are per context); a model with
            # feature dropout registers them
            for kw, expect in ((dict(dropout=0.0, attn_dropout=0.0), False), (dict(dropout=0.5, attn_dropout=0.6), True)):
                dctx = D.dist_context(overlap=True, device_index=0)
                A = matrix()
                Ad, ATd = D.dist_row_csr_matrix(dctx, A, p, p, keep_rows=True), D.dist_row_csr_matrix(dctx, A.transpose(), p, p)
                Xd, Yd = D.dist_row_dn_matrix(dctx, X), D.dist_row_dn_matrix(dctx, Y)
                G = D.dist_gat(dctx, Ad, ATd, sizes, heads=heads, **kw)
                clean = D.dist_gat(dctx, Ad, ATd, sizes, heads=heads)
                # a plain call never drops, and takes no epoch number
                o0, o1 = clean(dctx, Xd).local, G(dctx, Xd).local
                dctx.sync()
                if G.dropout_epoch != 0 or not np.array_equal(_bits(o0.numpy()), _bits(o1.numpy())):
                    bad.append(("a plain call dropped", kw, G.dropout_epoch))
                if not np.abs(o1.numpy()).max() > 0:
                    bad.append(("a plain call gave zeros", kw))
                if any("dropout" in t for t in dctx.ctx.timers):
                    bad.append(("a forward that does not train registered a dropout timer", kw))
                G.train_step(dctx, Xd, Yd, *ADAM)
                if any("dropout" in t for t in dctx.ctx.timers) != expect:
                    bad.append(("dropout timers", kw, sorted(t for t in dctx.ctx.timers if "dropout" in t)))
                if any("gat-exchange" in t for t in dctx.ctx.timers):
                    bad.append(("one rank exchanged", sorted(dctx.ctx.timers)))
        else:
            names = sorted(t for t in ctx.timers if "gat-exchange" in t)
            if names != sorted(f"{li}_{t}" for li in range(3) for t in ("0_gat-exchange", "1_gat-exchange-G", "1_gat-exchange-rec")):
                bad.append(("exchange timers", names))
        q.put((rank, bad, None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("backend", ["gloo", "nccl"])
def test_one_rank_is_the_single_gpu_model_bit_for_bit(backend):
    """P = 1: every parameter, gradient and Adam moment of dist_gat after three epochs has the bits of gat's, fused and
    per-tensor Adam, plain and with both dropouts.  Over gloo a single rank exchanges nothing (Z_all is Z_loc); over nccl
    with MGGCN_DIST_SELF_GATHER=1 every exchange runs through ProcessGroupNCCL with real stream ordering, overlap on and
    off, which the gloo path hides behind synchronisations.  Over gloo also: a plain call never drops (dist_gat has no evaluate(), like dist_gcn), and
    dist_gat(dropout=0, attn_dropout=0) registers no dropout timer"""
    (rank, bad, err), = _spawn(_p1_worker, 1, (backend,))
    assert err is None, err
    assert not bad, bad
