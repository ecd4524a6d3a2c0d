"""The row-partitioned GATv2 on the device (mg-gcn_amd/dist_gat.py, variant="v2"): dist_attention_v2 against the single-GPU
attention_v2 bit for bit at P = 1, 2, 4, the model against the reference model of gatv2_ref.py, dist_gat(variant="v2") at
P = 1 against gat(variant="v2") bit for bit -- over gloo, and over ProcessGroupNCCL with the self-gather on, where the three
exchanges really run on the comm stream --, the export on two ranks, and the default variant against the model as it was.

Multi-rank cases: fresh spawned children that share the one GPU over gloo (at most four, next to the parent), started with
_init / _spawn of test_gpu_dist_bf16.py.  A child never raises between two collectives (its peers would wait for it): it
collects what it found and reports at the end.

The all-reduced G_att is held to gatv2_ref.BAR["G_att"] = ROW_TOL on the scale of the exact restatement: test_dist_gatv2_cpu.py
shows that the fp32 twin of the rank-summed G_att stays within ROW_TOL / 8, which is gatv2_ref.bar_rule's condition for it."""
import os
import sys
import traceback

import numpy as np
import pytest

import bce_ref
import dist_gatv2_ref as dgr
import gat_ref as ref
import gatv2_ref as v2
from gat_ref import rowdist
from test_gpu_dist_bf16 import _init, _spawn
from test_gpu_dist_gat import _assert_model, _reference_epochs, _reference_grads, _single_state, _state
from test_gpu_gat import N, TOL, _model_data
from test_gpu_gatv2 import MODELS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADAM = ref.ADAM
MSEED = 0xC0FFEE123
EXCHANGES = ("0_gatv2-exchange", "1_gatv2-exchange-G", "1_gatv2-exchange-rec")


def _pkg():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as ge
    return ge.load_package()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the operator ------------------------------------------------------------------------------------------------------------------
def _op_worker(rank, P, port, q):
    """per shape: this rank's rows of the host Z2 = [Zs | Zd] and G through dist_attention_v2 (twice), the whole graph through
    attention_v2 in the same process; reports the outputs that are not the single-GPU rows bit for bit, and the all-reduced
    G_att next to the single-GPU one"""
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
        for K, dh in dgr.OP_SHAPES:
            d = K * dh
            Zs, Zd, G, att = v2.inputs(n, n, K, dh)
            Z2 = np.concatenate([Zs, Zd], axis=1)
            one = pkg.attention_v2("w_", n, d, K)
            one.init(att)
            Z1, G1, out1, GZ1 = dn.from_numpy(Z2), dn.from_numpy(G), dn(n, d), dn(n, 2 * d)
            one(ctx, F, Z1, out1)
            one.backward(ctx, F, A, Z1, G1, out1, GZ1)
            part = D.dist_attention_v2(dctx, "p_", n, d, K)
            part.init(att)
            if part.exchanging != (P > 1):
                bad.append((K, dh, "exchanging", part.exchanging))
            Zl, Gl = dn.from_numpy(Z2[lo:hi], ctx.device), dn.from_numpy(G[lo:hi], ctx.device)
            outl, GZl = dn(hi - lo, d), dn(hi - lo, 2 * d)
            for _ in range(2):                                          # the second call meets the buffers the first one left
                part(ctx, Fb, Zl, outl)
                part.backward(ctx, Fb, FTb, Zl, Gl, outl, GZl)
            dctx.all_reduce_sum([part.G_att.t])
            ctx.sync()
            got = dict(out=outl.numpy(), lse=part.lse.numpy(), D=part.D.numpy(), P=part.P.numpy(), G_Zs=GZl.numpy()[:, :d],
                       G_Zd=GZl.numpy()[:, d:])
            want = dict(out=out1.numpy(), lse=one.lse.numpy(), D=one.D.numpy(), P=one.P.numpy(), G_Zs=GZ1.numpy()[:, :d],
                        G_Zd=GZ1.numpy()[:, d:])
            for nm in dgr.ROW_NAMES:
                g, w = _bits(got[nm]), _bits(want[nm][lo:hi])
                if not np.array_equal(g, w):
                    bad.append((K, dh, nm, int((g != w).sum())))
            for nm in ("G_Zs", "G_Zd"):
                if not np.abs(got[nm]).max() > 0:
                    bad.append((K, dh, nm + " is all zeros"))
            gatt[(K, dh)] = (part.G_att.numpy().copy(), one.G_att.numpy().copy())
        q.put((rank, bad, gatt, None))
    except Exception:
        q.put((rank, None, None, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("P", [1, 2, 4])
def test_dist_attention_v2_gives_the_single_gpu_rows_bit_for_bit(P):
    """kernel_graph_long as F (n = 320, keep_rows) at (4, 32), (3, 7), (1, 260), every call twice: out, lse, D, G_Zd, P and
    G_Zs of every rank are the single-GPU attention_v2's rows bit for bit and G_Z2 is not all zeros; the all-reduced G_att
    has the same bits on every rank and is within gatv2_ref.BAR["G_att"] of the fp64 restatement on its scale"""
    res = _spawn(_op_worker, P, ())
    for rank, bad, gatt, err in res:
        assert err is None, err
        assert not bad, (rank, bad)
    for K, dh in dgr.OP_SHAPES:
        c = dgr.op_case(K, dh)
        first = res[0][2][(K, dh)][0]
        for rank, _, gatt, _ in res:
            mine, single = gatt[(K, dh)]
            np.testing.assert_array_equal(_bits(mine), _bits(first), err_msg=f"rank {rank} {(K, dh)}")
            for what, g in (("partitioned", mine), ("single", single)):
                dist_ = float(rowdist(g, c["want"]["G_att"], c["scale"]["G_att"]).max())
                print(f"[dist-gatv2] P={P} rank {rank} K={K} dh={dh} G_att {what}: {dist_:.3e} (bar {v2.BAR['G_att']:.0e})")
                assert dist_ <= v2.BAR["G_att"], (what, rank, K, dh, dist_)


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def _dist_model(pkg, dctx, csr, P, sizes, heads, **kw):
    D = pkg.dist
    ip, ix, dv = csr
    A = pkg.csr_matrix(ip.copy(), ix.copy(), dv.copy(), N)
    p = D.partition_bounds(N, P)
    return D.dist_gat(dctx, D.dist_row_csr_matrix(dctx, A, p, p, keep_rows=True), D.dist_row_csr_matrix(dctx, A.transpose(), p, p),
                      sizes, heads=heads, **kw), p


def _epochs(G, dctx, Xd, Yd, S, resync, bad):
    """three epochs, the last through train_step: per epoch (result, gradient buffers -- read before Adam, after it in the
    train_step epoch --, parameters after Adam, split_metrics, the state's bits); after every epoch the parameters are checked
    against the reference's up to a sign flip and continued from the reference's"""
    out = []
    for ep in range(3):
        if ep == 2:                                                 # the one-sync step
            res = G.train_step(dctx, Xd, Yd, *ADAM)
        else:
            res = G.train_forward(dctx, Xd, Yd)
            G.backward(dctx)
            dctx.sync()
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
    return out


def _model_worker(rank, P, port, cfg, resync, q):
    """the epochs of _epochs on dist_gat(variant="v2"); cfg: sizes, heads, overlap, and optionally loss / T / S (BCE with
    splits), p (feature dropout from epoch 4 of MSEED, after the replay check: training forward 4 run twice gives the same
    bits, forward 5 others), both_adam (a second model with per-tensor Adam through the same epochs: the same bits).  Also
    the bytes the first epoch handed to the exchange and the exchange timers"""
    dist = _init(rank, P, port)
    try:
        pkg = _pkg()
        D = pkg.dist
        sizes, heads = cfg["sizes"], cfg["heads"]
        csr, X, Y = _model_data(pkg, sizes)
        targets = cfg.get("T", Y)
        dctx = D.dist_context(overlap=cfg["overlap"], device_index=0)
        kw = dict(loss=cfg.get("loss", "softmax"), dropout=cfg.get("p", 0.0), variant="v2")
        G, p = _dist_model(pkg, dctx, csr, P, sizes, heads, **kw)
        bad = []
        if G.variant != "v2" or any(type(l).__name__ != "dist_gatv2_layer" for l in G.layers()):
            bad.append(("not a v2 model", G.variant))
        S = cfg.get("S")
        if S is not None:
            G.set_splits(dctx, S[p[rank]:p[rank + 1]].copy())
        Xd, Yd = D.dist_row_dn_matrix(dctx, X), D.dist_row_dn_matrix(dctx, targets)
        if "p" in cfg:
            def forward_backward(epoch):
                G.set_dropout(cfg["p"], seed=MSEED, epoch=epoch)
                res = G.train_forward(dctx, Xd, Yd)
                G.backward(dctx)
                dctx.sync()
                return res, [_bits(t.local.numpy()).copy() for l in G.layers() for t in (l.GW(), l.Gb(), l.Gatt())]
            first, other, again = forward_backward(4), forward_backward(5), forward_backward(4)
            if first[0] != again[0] or not all(np.array_equal(a, b) for a, b in zip(first[1], again[1])):
                bad.append(("set_dropout(epoch=4) did not replay training forward 4", first[0], again[0]))
            if first[0] == other[0] or all(np.array_equal(a, b) for a, b in zip(first[1], other[1])):
                bad.append(("training forward 5 drew the mask of forward 4", first[0], other[0]))
            try:
                G.set_dropout(cfg["p"], seed=MSEED, epoch=9, attn=0.1)
                bad.append(("set_dropout(attn=0.1) was taken",))
            except ValueError:
                if G.attn_dropout_p != 0.0 or G.dropout_epoch != 5:
                    bad.append(("a refused set_dropout stored something", G.attn_dropout_p, G.dropout_epoch))
            G.set_dropout(cfg["p"], seed=MSEED, epoch=4)
        dctx.exchange_bytes = 0
        out = _epochs(G, dctx, Xd, Yd, S, resync, bad)
        nbytes = None
        if "p" not in cfg and S is None:
            # one epoch more, counted: forward, backward (the exchanges do not depend on the values)
            dctx.exchange_bytes = 0
            G.train_forward(dctx, Xd, Yd)
            G.backward(dctx)
            dctx.sync()
            nbytes = int(dctx.exchange_bytes)
        names = sorted(t for t in dctx.ctx.timers if "exchange" in t)
        if names != sorted(f"{li}_{t}" for li in range(len(sizes) - 1) for t in EXCHANGES):
            bad.append(("exchange timers", names))
        if cfg.get("both_adam"):
            G2, _ = _dist_model(pkg, dctx, csr, P, sizes, heads, fused=False, **kw)
            out2 = _epochs(G2, dctx, Xd, Yd, S, resync, bad)
            for e, (a, b) in enumerate(zip(out, out2)):
                if a[0] != b[0]:
                    bad.append(("per-tensor Adam: another result", e, a[0], b[0]))
                for li, (x, y) in enumerate(zip(a[4], b[4])):
                    for ti, (u, w) in enumerate(zip(x, y)):
                        if (u is None) != (w is None) or (u is not None and not np.array_equal(u, w)):
                            bad.append(("per-tensor Adam: other bits", e, li, ti))
        q.put((rank, out, bad, nbytes, None))
    except Exception:
        q.put((rank, None, None, None, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def _oracle(oracle, csr, sizes, heads, **kw):
    ip, ix, dv = csr
    per_layer = [heads] * (len(sizes) - 2) + [1]
    return v2.oracle_gatv2(oracle, oracle.Csr(ip.copy(), ix.copy(), dv.copy(), N), sizes, per_layer, **kw)


@pytest.mark.parametrize("P,overlap,model,both_adam", [(2, True, 0, True), (4, False, 0, False), (2, False, 1, False), (4, True, 1, True)])
def test_dist_gatv2_epochs_match_the_reference(pkg, oracle, P, overlap, model, both_adam):
    """n = 1024, the two models of test_gpu_gatv2.py, three epochs against gatv2_ref.oracle_gatv2 by the rules of
    test_gatv2_epochs_match_the_reference: loss at TOL, accuracy within 3 / n, G_W, G_b and G_att at TOL, parameters never more
    than a sign flip away; the state is bit-equal on all ranks after every epoch, fused and per-tensor Adam give the same bits,
    and an epoch hands the exchange the bytes DESIGN.md 3.10.5 states"""
    sizes, heads = MODELS[model]
    csr, X, Y = _model_data(pkg, sizes)
    want, resync = _reference_epochs(_oracle(oracle, csr, sizes, heads), X, Y)
    res = _spawn(_model_worker, P, (dict(sizes=sizes, heads=heads, overlap=overlap, both_adam=both_adam), resync))
    _assert_model(P, res, want, N)
    for rank, _, _, nbytes, _ in res:
        assert nbytes == dgr.exchange_bytes_v2(N, P, sizes, heads), (rank, nbytes)
    assert res[0][1][-1][0][0] < res[0][1][0][0][0]                     # it trains: the loss of epoch 2 against epoch 0


def test_dist_gatv2_dropout_epochs_match_the_reference_and_replay(pkg, oracle):
    """dropout = 0.5 at P = 2 against the reference model with the numpy mask, from epoch 4 of seed 0xC0FFEE123 (a rank drops
    its own rows of the global mask); before that, on every rank: set_dropout(epoch=4) replays training forward 4 to the bit,
    forward 5 differs, and set_dropout(attn=0.1) is refused and stores nothing"""
    sizes, heads = MODELS[0]
    P = 2
    csr, X, Y = _model_data(pkg, sizes)
    O = _oracle(oracle, csr, sizes, heads, p=0.5, seed=MSEED, epoch=4)
    want, resync = _reference_epochs(O, X, Y)
    res = _spawn(_model_worker, P, (dict(sizes=sizes, heads=heads, overlap=True, p=0.5), resync))
    _assert_model(P, res, want, N)


def test_dist_gatv2_bce_with_splits_matches_the_reference(pkg, oracle):
    """loss="bce" + set_splits at P = 2 against the reference model under bce_ref.oracle_bce: the training split's loss at
    TOL, every split's loss, row count and confusion counts as test_gpu_dist_gat.py checks them"""
    sizes, heads = MODELS[1]
    P = 2
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


# ---- one rank: dist_gat(variant="v2") is gat(variant="v2"); the default is the model as it was -------------------------------------
def _p1_worker(rank, P, port, backend, q):
    """one rank: dist_gat(variant="v2") against gat(variant="v2") in one process after three train_steps, fused and
    per-tensor Adam, overlap on and off; returns the results and the state's bits of the fused, overlapping run.  Over gloo
    also: nothing is exchanged, and dist_gat(variant="v1") and dist_gat() give the same bits after one train_step and launch
    nothing of v2"""
    dist = _init(rank, P, port, backend)
    try:
        pkg = _pkg()
        D = pkg.dist
        sizes, heads = MODELS[1]
        csr, X, Y = _model_data(pkg, sizes)
        ip, ix, dv = csr
        bad, keep = [], None
        X1, Y1 = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
        for overlap in (True, False):
            dctx = D.dist_context(overlap=overlap, device_index=0)
            ctx = dctx.ctx
            if dctx.self_gather != (backend == "nccl"):
                bad.append(("self_gather", dctx.self_gather))
            Xd, Yd = D.dist_row_dn_matrix(dctx, X), D.dist_row_dn_matrix(dctx, Y)
            for fused in (True, False):
                G1 = pkg.gat(pkg.csr_matrix(ip.copy(), ix.copy(), dv.copy(), N), sizes, heads=heads, fused=fused, variant="v2")
                Gd, _ = _dist_model(pkg, dctx, csr, 1, sizes, heads, fused=fused, variant="v2")
                if Gd.layers()[0].attn.exchanging != (backend == "nccl"):
                    bad.append(("exchanging", backend))
                r1 = [G1.train_step(ctx, X1, Y1, *ADAM) for _ in range(3)]
                rd = [Gd.train_step(dctx, Xd, Yd, *ADAM) for _ in range(3)]
                if r1 != rd:
                    bad.append((overlap, fused, "results", r1, rd))
                for li, (a, b) in enumerate(zip(_single_state(G1), _state(Gd))):
                    for ti, (x, y) in enumerate(zip(a, b)):
                        if not np.array_equal(x, y):
                            bad.append((overlap, fused, "state", li, ti, int((x != y).sum())))
                if not r1[-1][0] < r1[0][0]:
                    bad.append(("does not train", r1))
                if overlap and fused:
                    keep = (rd, _state(Gd))
            names = sorted(t for t in ctx.timers if "exchange" in t)
            expect = sorted(f"{li}_{t}" for li in range(len(sizes) - 1) for t in EXCHANGES) if backend == "nccl" else []
            if names != expect:
                bad.append(("exchange timers", backend, names))
        if backend == "gloo":
            dctx = D.dist_context(overlap=True, device_index=0)
            Xd, Yd = D.dist_row_dn_matrix(dctx, X), D.dist_row_dn_matrix(dctx, Y)
            Ga, _ = _dist_model(pkg, dctx, csr, 1, sizes, heads)
            Gb, _ = _dist_model(pkg, dctx, csr, 1, sizes, heads, variant="v1")
            ra, rb = Ga.train_step(dctx, Xd, Yd, *ADAM), Gb.train_step(dctx, Xd, Yd, *ADAM)
            if ra != rb or Ga.variant != "v1" or Gb.variant != "v1":
                bad.append(("variant=\"v1\" is not the default", ra, rb))
            for li, (a, b) in enumerate(zip(_state(Ga), _state(Gb))):
                for ti, (x, y) in enumerate(zip(a, b)):
                    if not np.array_equal(x, y):
                        bad.append(("variant=\"v1\" state", li, ti))
            if [type(l).__name__ for l in Gb.layers()] != ["dist_gat_layer"] * 3 or Gb.layers()[0].W().local.shape() != (sizes[0], sizes[1]):
                bad.append(("variant=\"v1\" built other layers",))
            if any("gatv2" in t for t in dctx.ctx.timers) or hasattr(Gb, "P_buffer"):
                bad.append(("a v1 model launched or allocated something of v2", sorted(dctx.ctx.timers)))
        q.put((rank, bad, keep, None))
    except Exception:
        q.put((rank, None, None, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_one_rank_is_the_single_gpu_model_bit_for_bit_over_gloo_and_nccl():
    """P = 1: every parameter, gradient and Adam moment of dist_gat(variant="v2") after three train_steps, and the three
    losses, have the bits of gat(variant="v2")'s, fused and per-tensor Adam, overlap on and off.  Over gloo a single rank
    exchanges nothing (Z2_all is Z2, G_all is G, rec_all is rec); over nccl with MGGCN_DIST_SELF_GATHER=1 the three exchanges
    of every layer run through ProcessGroupNCCL with real stream ordering, which the gloo path hides behind
    synchronisations -- and give the gloo run's bits.  Over gloo also: variant="v1" is the default, bit for bit, and
    launches and allocates nothing of v2"""
    runs = {}
    for backend in ("gloo", "nccl"):
        (rank, bad, keep, err), = _spawn(_p1_worker, 1, (backend,))
        assert err is None, err
        assert not bad, (backend, bad)
        runs[backend] = keep
    assert runs["gloo"][0] == runs["nccl"][0]
    for li, (a, b) in enumerate(zip(runs["gloo"][1], runs["nccl"][1])):
        for ti, (x, y) in enumerate(zip(a, b)):
            np.testing.assert_array_equal(x, y, err_msg=f"layer {li} tensor {ti}")


# ---- the export ----------------------------------------------------------------------------------------------------------------------
def _alpha_worker(rank, P, port, X, q):
    """a rank's export (after attention_weights(dctx, X), and again from the state) and its pattern"""
    dist = _init(rank, P, port)
    try:
        pkg = _pkg()
        D = pkg.dist
        sizes, heads = MODELS[1]
        csr, _, _ = _model_data(pkg, sizes)
        dctx = D.dist_context(overlap=True, device_index=0)
        G, p = _dist_model(pkg, dctx, csr, P, sizes, heads, variant="v2")
        refused = False
        try:
            G.attention_weights(dctx)
        except ValueError:
            refused = True
        first = G.attention_weights(dctx, D.dist_row_dn_matrix(dctx, X))
        again = G.attention_weights(dctx, layers=[2, 0])
        dctx.sync()
        timers = sorted(t for t in dctx.ctx.timers if "exchange" in t)
        first, again = [a.numpy().copy() for a in first], [a.numpy().copy() for a in again]
        ip, ix = G.attention_pattern()
        q.put((rank, dict(first=first, again=again, indptr=ip.copy(), indices=ix.copy(), refused=refused, bounds=list(p),
                          timers=timers), None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_dist_gatv2_exports_the_single_gpu_rows_bit_for_bit(pkg):
    """two ranks sharing the GPU: rank r's export is rows [p_r, p_{r+1}) of the single-GPU gat(variant="v2")'s export from the
    same (seed-99) weights, bit for bit, in every layer; its pattern is those rows of the single-GPU pattern with global
    columns; an export from the state (layers=[2, 0]) repeats the bits and runs no collective beyond the forward's one
    exchange per layer; no forward yet is refused on every rank"""
    sizes, heads = MODELS[1]
    per_layer = [heads] * (len(sizes) - 2) + [1]
    csr, X, _ = _model_data(pkg, sizes)
    ctx = pkg.context(0)
    G = pkg.gat(pkg.csr_matrix(csr[0].copy(), csr[1].copy(), csr[2].copy(), N), sizes, heads=heads, variant="v2")
    single = G.attention_weights(ctx, pkg.dn_matrix.from_numpy(X))
    ctx.sync()
    single = [a.numpy() for a in single]
    indptr, indices = G.attention_pattern()
    ip = indptr.astype(np.int64)
    res = _spawn(_alpha_worker, 2, (X,))
    covered = 0
    for rank, r, err in res:
        assert err is None, err
        assert r["refused"]
        assert r["timers"] == sorted(f"{li}_{EXCHANGES[0]}" for li in range(3)), r["timers"]
        lo, hi = r["bounds"][rank], r["bounds"][rank + 1]
        e0, e1 = int(ip[lo]), int(ip[hi])
        np.testing.assert_array_equal(r["indptr"].astype(np.int64), ip[lo:hi + 1] - ip[lo])
        np.testing.assert_array_equal(r["indices"], indices[e0:e1])
        assert int(r["indices"].max()) >= hi - lo                       # global columns: beyond the rank's own rows
        for li in range(3):
            assert r["first"][li].shape == (e1 - e0, per_layer[li])
            np.testing.assert_array_equal(_bits(r["first"][li]), _bits(single[li][e0:e1]), err_msg=f"rank {rank} layer {li}")
            assert np.abs(r["first"][li]).max() > 0
        for a, li in zip(r["again"], (2, 0)):
            np.testing.assert_array_equal(_bits(a), _bits(single[li][e0:e1]), err_msg=f"rank {rank} layer {li} from the state")
        covered += e1 - e0
    assert covered == indices.size and e1 - e0 > 0
