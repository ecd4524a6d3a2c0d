"""The row-partitioned GraphSAGE on the device (mg-gcn_amd/dist_sage.py): dist_max_aggregate against the single-GPU kernels bit
for bit at P = 2, 4, dist_sage at P = 1 against sage bit for bit -- over gloo, and over ProcessGroupNCCL with the self-gather
on, where the exchanges really run on the comm stream --, and dist_sage at P = 2, 4 against tests/sage_ref.py.

n = 300 (test_gpu_sage.py's graph: unsorted rows, duplicate entries, self-loops), sizes [24, 32, 32, 7] and [21, 13, 5]: the
second puts 21- and 13-wide records on the element path.  Multi-rank cases: fresh spawned children that share the one GPU
over gloo (at most four, next to the parent), started with _init / _spawn of test_gpu_dist_bf16.py.  A child never raises
between two collectives (its peers would wait for it): it collects what it found and reports at the end.

The model at P > 1 is checked as test_gpu_sage.py checks sage.  SELECTION: every rank returns its rows of every layer's input,
M and arg; assembled, M and arg must equal sage_ref.agg_max on those very bits, exactly.  ARITHMETIC: the fp64 restatement
runs with the device's args (and the device's masks), and the loss, the logits and every all-reduced gradient of a first
training pass are held to EIGHT TIMES the fp32 twin's worst distance over these tensors.  Then three train_steps: before each
the ranks return their parameters, and the step's loss and logits are held to eight times the twin's worst distance over the
two, the restatement and the twin running on those parameters with that step's args and masks.  No constant of its own."""
import os
import sys
import traceback

import numpy as np
import pytest

import dropout_ref
import sage_ref as ref
from test_gpu_dist_bf16 import _init, _spawn
from test_gpu_sage import ADAM, CONFIGS, N, SEED, _dist, _inputs, _param_bits, _tensors

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ([24, 32, 32, 7], [21, 13, 5])
EXCHANGES = ("0_sage-exchange", "1_sage-exchange-rec")


def _pkg():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as ge
    return ge.load_package()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def _host_pair(pkg, d, aggr):
    """(A, A_T) on the host as sage makes them: column-normalised for mean, as they are for max"""
    A = pkg.csr_matrix(d["ip"].copy(), d["ix"].copy(), d["dv"].copy(), N)
    if aggr == "mean":
        A.normalize(True)
    return A, A.transpose()


def _dist_model(pkg, dctx, d, sizes, aggr, **kw):
    D = pkg.dist
    A, A_T = _host_pair(pkg, d, aggr)
    p = D.partition_bounds(N, dctx.P)
    return D.dist_sage(dctx, D.dist_row_csr_matrix(dctx, A, p, p), D.dist_row_csr_matrix(dctx, A_T, p, p), sizes, aggr=aggr,
                       weights=d["weights"], **kw), p


# ---- the operator ------------------------------------------------------------------------------------------------------------------
def _op_worker(rank, P, port, q):
    """per overlap setting and width: this rank's rows of a host B and G through dist_max_aggregate (every call twice), the
    whole graph through ops.agg_max_forward / ops.agg_max_backward in the same process; reports what is not the single-GPU
    rows bit for bit, the bytes handed to the exchange and the exchange timers"""
    dist = _init(rank, P, port)
    try:
        import torch
        from importlib import import_module
        pkg = _pkg()
        D, dn, ops = pkg.dist, pkg.dn_matrix, pkg.ops
        sorted_row_block = import_module(pkg.__name__ + ".dist_sage").sorted_row_block
        d0 = _inputs(pkg, SIZES[0])
        A, F = _host_pair(pkg, d0, "max")
        A_sorted = F.transpose()
        p = D.partition_bounds(N, P)
        lo, hi = p[rank], p[rank + 1]
        bad = []
        for overlap in (True, False):
            dctx = D.dist_context(overlap=overlap, device_index=0)
            ctx, dev = dctx.ctx, dctx.ctx.device
            Fb = D.dist_row_csr_matrix(dctx, F, p, p).row_block_global()
            FTb = sorted_row_block(D.dist_row_csr_matrix(dctx, A, p, p).row_block_global())
            shared = torch.empty(N * 32, dtype=torch.float32, device=dev)
            for d, buf in ((32, shared), (21, shared), (13, None)):
                rng = np.random.default_rng(d)
                B = (np.round(2 * rng.standard_normal((N, d))) / 2).astype(np.float32)             # ties everywhere
                G = rng.standard_normal((N, d)).astype(np.float32)
                base = rng.standard_normal((N, d)).astype(np.float32)
                B1, G1, M1, arg1 = dn.from_numpy(B), dn.from_numpy(G), dn(N, d), dn(N, d, dtype=np.int32)
                ops.agg_max_forward(ctx, F, B1, M1, arg1)
                want = {}
                for discard in (True, False):
                    GB1 = dn.from_numpy(base)
                    ops.agg_max_backward(ctx, A_sorted, arg1, G1, GB1, accumulate=not discard)
                    ctx.sync()
                    want[discard] = GB1.numpy()
                part = D.dist_max_aggregate(dctx, "t_", Fb, FTb, True, buf)
                if not part.exchanging or part.row0 != lo:
                    bad.append((overlap, d, "exchanging / row0", part.exchanging, part.row0))
                Bl, Gl, Ml = dn.from_numpy(B[lo:hi], dev), dn.from_numpy(G[lo:hi], dev), dn(hi - lo, d)
                dctx.exchange_bytes = 0
                for _ in range(2):                                      # the second call meets the buffers the first one left
                    part(ctx, Bl, Ml)
                ctx.sync()
                if dctx.exchange_bytes != 2 * (hi - lo) * d * 4:
                    bad.append((overlap, d, "forward bytes", dctx.exchange_bytes))
                for nm, got, w in (("M", Ml.numpy(), M1.numpy()), ("arg", part.arg.numpy(), arg1.numpy())):
                    if not np.array_equal(_bits(got), _bits(w[lo:hi])):
                        bad.append((overlap, d, nm, int((_bits(got) != _bits(w[lo:hi])).sum())))
                if not (part.arg.numpy().view(np.uint32) < N).any():
                    bad.append((overlap, d, "arg selects nothing"))
                for discard in (True, False):
                    dctx.exchange_bytes = 0
                    for started in (False, True):                       # backward() starts the exchange itself, or finds it started
                        GBl = dn.from_numpy(base[lo:hi], dev)
                        if started:
                            part.start_backward(ctx, Gl)
                        part.backward(ctx, Gl, GBl, discard)
                        ctx.sync()
                        g, w = _bits(GBl.numpy()), _bits(want[discard][lo:hi])
                        if not np.array_equal(g, w):
                            bad.append((overlap, d, "G_B", discard, started, int((g != w).sum())))
                        if not np.abs(GBl.numpy() - base[lo:hi]).max() > 0:
                            bad.append((overlap, d, "G_B is its initial value"))
                    if dctx.exchange_bytes != 2 * (hi - lo) * d * 8:
                        bad.append((overlap, d, "backward bytes", dctx.exchange_bytes))
            names = sorted(t for t in ctx.timers if "exchange" in t)
            if names != sorted("t_" + t for t in EXCHANGES):
                bad.append((overlap, "exchange timers", names))
        q.put((rank, bad, None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("P", [2, 4])
def test_dist_max_aggregate_gives_the_single_gpu_rows_bit_for_bit(P):
    """widths 32 (four columns per lane), 21 and 13 (the element path), overlap on and off, every call twice: M, arg and G_B
    (overwritten and accumulated) of every rank are the single-GPU rows bit for bit, and a rank hands the exchange
    n/P . d . 4 bytes per forward and n/P . d . 8 per backward"""
    for rank, bad, err in _spawn(_op_worker, P, ()):
        assert err is None, err
        assert not bad, (rank, bad)


# ---- the model at P = 1 ----------------------------------------------------------------------------------------------------------
def _single_worker(rank, P, port, backend, aggrs, q):
    """per aggr, sizes and configuration: three train_steps of sage and of dist_sage on one rank; reports what differs"""
    dist = _init(rank, P, port, backend=backend)
    try:
        pkg = _pkg()
        D, dn = pkg.dist, pkg.dn_matrix
        dctx = D.dist_context(overlap=True, device_index=0)
        ctx1 = pkg.context(0)
        bad, dropped = [], False
        if dctx.self_gather != (backend == "nccl"):
            bad.append(("self_gather", dctx.self_gather))
        for aggr in aggrs:
            for sizes in SIZES:
                for config, kw in CONFIGS.items():
                    d = _inputs(pkg, sizes, kw.get("loss", "softmax"))
                    one = pkg.sage(pkg.csr_matrix(d["ip"].copy(), d["ix"].copy(), d["dv"].copy(), N), sizes, aggr=aggr,
                                   weights=d["weights"], **kw)
                    part, _ = _dist_model(pkg, dctx, d, sizes, aggr, **kw)
                    for m in (one, part):
                        if kw.get("dropout"):
                            m.set_dropout(kw["dropout"], seed=SEED)
                    X1, Y1 = dn.from_numpy(d["X"].copy()), dn.from_numpy(d["Y"].copy())
                    Xd, Yd = D.dist_row_dn_matrix(dctx, d["X"].copy()), D.dist_row_dn_matrix(dctx, d["Y"].copy())
                    want = [one.train_step(ctx1, X1, Y1, *ADAM) for _ in range(3)]
                    got = [part.train_step(dctx, Xd, Yd, *ADAM) for _ in range(3)]
                    key = (aggr, tuple(sizes), config)
                    if [tuple(map(float, x)) for x in got] != [tuple(map(float, x)) for x in want]:
                        bad.append(key + ("losses", got, want))
                    if not all(np.isfinite(x[0]) for x in want) or not (kw.get("dropout") or want[2][0] < want[0][0]):
                        bad.append(key + ("does not train", want))
                    a, b = _param_bits(part), _param_bits(one)
                    if len(a) != len(b) or not all(np.array_equal(x, y) for x, y in zip(a, b)):
                        bad.append(key + ("parameters",))
                    if not np.array_equal(_bits(part.layers()[-1].Y.numpy()), _bits(one.layers()[-1].Y.numpy())):
                        bad.append(key + ("logits",))
                    kept = part.layers()[0].M
                    part.reset_input_cache()
                    if kept is None or part.layers()[0].M is not None:
                        bad.append(key + ("reset_input_cache() did not drop layer 0's kept aggregate",))
                    if aggr == "max" and part.layers()[1].agg.exchanging != (backend == "nccl"):
                        bad.append(key + ("exchanging",))
                    dropped = dropped or bool(kw.get("dropout"))         # the context keeps every model's timers
                    if not dropped and any("dropout" in t for t in dctx.ctx.timers):
                        bad.append(key + ("a model without dropout registered a dropout timer",))
        names = {t.split("_", 1)[1] for t in dctx.ctx.timers if "sage-exchange" in t}
        if names != (set(EXCHANGES) if backend == "nccl" and "max" in aggrs else set()):
            bad.append(("exchange timers", sorted(names)))
        q.put((rank, bad, None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("aggr", ["mean", "max"])
def test_one_rank_is_sage_bit_for_bit(aggr):
    """three train_steps under plain, norm="layer", dropout=0.5 and loss="bce", both size lists: the losses, every parameter
    and the logits of sage, bit for bit; nothing is exchanged, and the default model registers no dropout timer"""
    for rank, bad, err in _spawn(_single_worker, 1, ("gloo", (aggr,))):
        assert err is None, err
        assert not bad, (rank, bad)


def test_one_rank_over_rccl_with_the_self_gather_is_sage_bit_for_bit():
    """the same over ProcessGroupNCCL with dist_context.self_gather: the all-gathers of H and of the records run on the comm
    stream, and the record kernels replace the plain ones"""
    for rank, bad, err in _spawn(_single_worker, 1, ("nccl", ("mean", "max"))):
        assert err is None, err
        assert not bad, (rank, bad)


# ---- the model at P = 2, 4 -------------------------------------------------------------------------------------------------------
def _params(G):
    """(weights, norms) of the model as sage_ref.Sage takes them, host copies"""
    weights = [(l.lin.W.numpy().copy(), l.lin.b.numpy().copy(), l.res_lin.W.numpy().copy(), l.res_lin.b.numpy().copy())
               for l in G.layers()]
    norms = [(l.norm.gamma.numpy().copy(), l.norm.beta.numpy().copy()) for l in G.layers() if l.norm is not None]
    return weights, norms or None


def _forward_state(G, aggr):
    """this rank's rows of what the last forward left: per layer its input H, M and arg (max, layers above the first), and
    the logits"""
    layers = G.layers()
    out = dict(H=[None] + [l.H.numpy().copy() for l in layers[1:]], M=[l.M.numpy().copy() for l in layers],
               logits=layers[-1].Y.numpy().copy(), arg=[None] * len(layers))
    if aggr == "max":
        out["arg"] = [None] + [l.agg.arg.numpy().view(np.uint32).copy() for l in layers[1:]]
    return out


def _model_worker(rank, P, port, cases, overlap, tmp, q):
    """per case (aggr, config, sizes, mode): a first training pass (loss, forward state, gradients after the all-reduce), then
    three train_steps with the parameters before and the forward state after each; save must raise and create nothing"""
    dist = _init(rank, P, port)
    try:
        pkg = _pkg()
        D = pkg.dist
        dctx = D.dist_context(overlap=overlap, device_index=0)
        out, bad = [], []
        for aggr, config, sizes, mode in cases:
            kw = CONFIGS[config]
            d = _inputs(pkg, sizes, kw.get("loss", "softmax"))
            G, p = _dist_model(pkg, dctx, d, sizes, aggr, mode=mode, **kw)
            if [l.row0 for l in G.layers()] != [p[rank]] * len(G.layers()):
                bad.append((aggr, config, "row0", [l.row0 for l in G.layers()]))
            if kw.get("dropout"):
                G.set_dropout(kw["dropout"], seed=SEED)
            Xd, Yd = D.dist_row_dn_matrix(dctx, d["X"].copy()), D.dist_row_dn_matrix(dctx, d["Y"].copy())
            res = dict(loss=G.train_forward(dctx, Xd, Yd)[0], state=_forward_state(G, aggr))
            G.backward(dctx)
            dctx.sync()
            grads = []
            for l in G.layers():
                g = dict(W_l=l.lin.G_W.numpy().copy(), b_l=l.lin.G_b.numpy().copy(), W_r=l.res_lin.G_W.numpy().copy(),
                         b_r=l.res_lin.G_b.numpy().copy())
                if l.norm is not None:
                    g.update(gamma=l.norm.G_gamma.numpy().copy(), beta=l.norm.G_beta.numpy().copy())
                grads.append(g)
            res["grads"] = grads
            res["steps"] = []
            for _ in range(3):
                params = _params(G)
                loss = G.train_step(dctx, Xd, Yd, *ADAM)[0]
                res["steps"].append(dict(params=params, loss=loss, state=_forward_state(G, aggr)))
            try:
                G.save(dctx, os.path.join(tmp, f"rank{rank}.ckpt"))
                bad.append((aggr, config, "save did not raise"))
            except ValueError as e:
                if "sage" not in str(e):
                    bad.append((aggr, config, "save", str(e)))
            out.append(res)
        q.put((rank, out, bad, None))
    except Exception:
        q.put((rank, None, None, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def _rows(res, pick):
    """the ranks' row shards of one tensor, stacked"""
    return np.concatenate([pick(r) for r in res], axis=0)


def _check_pass(pkg, what, aggr, kw, sizes, F, d, weights, norms, epoch, dev_loss, states, dev_grads):
    """selection exactly and arithmetic at eight times the twin for one training forward (and backward, with ``dev_grads``) of
    the device on ``weights``: ``states`` are the ranks' forward states, ``epoch`` the number of that training forward.
    Without ``dev_grads`` the states were read after a whole train_step, whose backward has overwritten the layers' inputs
    (the activation's gradient is formed in place): arg and the logits are still the forward's, so the restatement runs
    with the step's args and the selection itself is not checked again"""
    first = dev_grads is not None
    L = len(sizes) - 1
    loss_kind, p = kw.get("loss", "softmax"), kw.get("dropout", 0.0)
    logits = _rows(states, lambda s: s["logits"])
    args = [None] * L
    if aggr == "max":
        for l in range(1, L):
            arg = _rows(states, lambda s: s["arg"][l])
            args[l] = arg
            if not first:
                continue
            H = _rows(states, lambda s: s["H"][l])
            want_M, want_arg = ref.agg_max(F[0], F[1], H)
            assert (arg == want_arg).all(), (what, l, np.argwhere(arg != want_arg)[:4].tolist())
            assert (_bits(_rows(states, lambda s: s["M"][l])) == _bits(want_M)).all(), (what, l)
        want_M0, _ = ref.agg_max(F[0], F[1], d["X"])
        assert (_bits(_rows(states, lambda s: s["M"][0])) == _bits(want_M0)).all(), what
    masks = [None] * L
    if p:
        scale = dropout_ref.params(p)[1]
        masks = [None] + [(dropout_ref.mask(N, sizes[l], 0, p, SEED, epoch * 64 + l), scale) for l in range(1, L)]
        for l in range(1, L) if first else ():                 # the ranks dropped their rows of the global mask (row0 = p_r)
            H = _rows(states, lambda s: s["H"][l])
            assert ((H != 0) == masks[l][0]).all(), (what, l, "the dropped elements are not the global mask's")
    runs = {}
    for dtype in (np.float64, np.float32):
        R = ref.Sage(F, sizes, weights, aggr, dtype, norm=kw.get("norm"), norms=norms, loss=loss_kind, masks=masks)
        lv = R.train_forward(d["X"], d["Y"], args)
        runs[dtype] = _tensors(lv, R.logits, R.backward() if first else [])
    want, twin = runs[np.float64], runs[np.float32]
    dev = _tensors(dev_loss, logits, dev_grads or [])
    assert set(dev) == set(want)
    twin_worst = max(_dist(twin[k], want[k]) for k in want)
    dev_dist = {k: _dist(dev[k], want[k]) for k in want}
    worst = max(dev_dist, key=dev_dist.get)
    print(f"[dist-sage] {what}: twin worst {twin_worst:.3e}, device worst {dev_dist[worst]:.3e} ({worst}), "
          f"ratio {dev_dist[worst] / twin_worst:.2f} of 8")
    assert 0 < twin_worst < 1e-4
    assert dev_dist[worst] <= 8.0 * twin_worst, (what, worst, dev_dist[worst], 8.0 * twin_worst)


def _check_model(pkg, P, cases, res):
    for rank, out, bad, err in res:
        assert err is None, err
        assert not bad, (rank, bad)
    for ci, (aggr, config, sizes, mode) in enumerate(cases):
        kw = CONFIGS[config]
        d = _inputs(pkg, sizes, kw.get("loss", "softmax"))
        _, A_T = _host_pair(pkg, d, aggr)
        F = (A_T.indptr, A_T.indices, A_T.data)
        mine = [out[ci] for _, out, _, _ in res]
        what = f"P={P} {aggr} {config} {sizes} {mode}"
        for r in mine[1:]:                                       # the global loss and the summed gradients: the same bits everywhere
            assert r["loss"] == mine[0]["loss"] and [s["loss"] for s in r["steps"]] == [s["loss"] for s in mine[0]["steps"]]
            for g, g0 in zip(r["grads"], mine[0]["grads"]):
                assert all(np.array_equal(_bits(g[k]), _bits(g0[k])) for k in g0), what
        norms = None
        if kw.get("norm"):
            norms = [(np.ones((1, s), dtype=np.float32), np.zeros((1, s), dtype=np.float32)) for s in sizes[1:-1]]
        _check_pass(pkg, what + " first pass", aggr, kw, sizes, F, d, d["weights"], norms, 0, mine[0]["loss"],
                    [r["state"] for r in mine], mine[0]["grads"])
        for s in range(3):
            weights, norms = mine[0]["steps"][s]["params"]
            for r in mine[1:]:                                   # the replicas stay bit-equal
                assert all(np.array_equal(_bits(a), _bits(b)) for wa, wb in zip(r["steps"][s]["params"][0], weights)
                           for a, b in zip(wa, wb)), (what, s)
            _check_pass(pkg, what + f" step {s}", aggr, kw, sizes, F, d, weights, norms, 1 + s, mine[0]["steps"][s]["loss"],
                        [r["steps"][s]["state"] for r in mine], None)
        losses = [s["loss"] for s in mine[0]["steps"]]
        assert np.isfinite(losses).all() and (kw.get("dropout") or losses[-1] < mine[0]["loss"]), (what, losses)


@pytest.mark.parametrize("aggr", ["mean", "max"])
@pytest.mark.parametrize("P", [2, 4])
def test_dist_sage_matches_the_reference(pkg, tmp_path, P, aggr):
    """plain, norm="layer", dropout=0.5 and loss="bce" on both size lists; the exchange on the comm stream for one aggregator
    and on the compute stream for the other at each P; save raises on every rank and nothing is created"""
    cases = [(aggr, config, sizes, "allgather") for sizes in SIZES for config in CONFIGS]
    res = _spawn(_model_worker, P, (cases, (P == 2) == (aggr == "max"), str(tmp_path)))
    _check_model(pkg, P, cases, res)
    assert list(tmp_path.iterdir()) == []


def test_dist_sage_mean_on_the_halo_and_rounds_schedules(pkg, tmp_path):
    cases = [("mean", "plain", sizes, mode) for sizes in SIZES for mode in ("halo", "rounds")]
    res = _spawn(_model_worker, 2, (cases, True, str(tmp_path)))
    _check_model(pkg, 2, cases, res)


@pytest.mark.parametrize("aggr", ["mean", "max"])
def test_two_ranks_drop_the_rows_the_single_gpu_model_drops(pkg, tmp_path, aggr):
    """dropout = 0.5 at P = 2: the dropped elements of every layer's input, the ranks' rows stacked, are those of the single-GPU
    model on the same seed (the row0 = p_r check test_gpu_dist_dropout.py makes for dist_gcn)"""
    sizes = SIZES[0]
    cases = [(aggr, "dropout", sizes, "allgather")]
    res = _spawn(_model_worker, 2, (cases, True, str(tmp_path)))
    for rank, out, bad, err in res:
        assert err is None, err
        assert not bad, (rank, bad)
    d = _inputs(pkg, sizes)
    ctx = pkg.context(0)
    one = pkg.sage(pkg.csr_matrix(d["ip"].copy(), d["ix"].copy(), d["dv"].copy(), N), sizes, aggr=aggr, weights=d["weights"],
                   dropout=0.5)
    one.set_dropout(0.5, seed=SEED)
    one.train_forward(ctx, pkg.dn_matrix.from_numpy(d["X"].copy()), pkg.dn_matrix.from_numpy(d["Y"].copy()))
    ctx.sync()
    for l in range(1, len(sizes) - 1):
        H1 = one.layers()[l].H.numpy()
        H = _rows([out[0]["state"] for _, out, _, _ in res], lambda s: s["H"][l])
        assert ((H == 0) == (H1 == 0)).all() and (H == 0).any() and (H != 0).any(), l
        # shifted by one rank's rows the pattern is another one: the check can see a wrong row0
        assert ((np.roll(H, N // 2, axis=0) == 0) != (H1 == 0)).any()
