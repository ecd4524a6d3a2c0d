"""Edge sampling with values in the models (gcn and sage(aggr="mean") with edge_rescale=) on the device, on a graph of 1000
vertices with one hub whose row of ~1000 entries is sliced by the row-split plan, in the forward matrix and in its transpose:
the identity setting gives the unsampled model's bits, a real sample follows a float64 restatement of forward + loss on the
restated and rescaled matrix of every epoch at the suite's model bar, an epoch replays, every forward that is not a training
forward keeps the full graph's bits, the options compose, and "off" owns nothing."""
import numpy as np
import pytest

import edge_sample_ref as es_ref
import edge_sample_val_ref as vref

pytestmark = pytest.mark.gpu

TOL = 1e-4                          # the suite's model bar (test_gpu_gcn.py, test_gpu_agg_bf16.py)
ADAM = (1e-2, 0.9, 0.999, 5e-4, 1e-8)
N, SIZES = 1000, [16, 32, 5]
SEED = 0xABCDEF0123456789
TIMERS = ("sample-count", "sample-scan", "sample-compact", "sample-plan")
KINDS = ("gcn", "sage")


@pytest.fixture()
def ctx(pkg):
    return pkg.context(0)           # a context per test: its timers are this test's


_data = {}


def _graph():
    """self-loops, six random neighbours per vertex, and vertex 0 joined with everybody in both directions"""
    if "g" not in _data:
        rng = np.random.default_rng(7)
        rows = [set([i]) | set(int(j) for j in rng.integers(0, N, size=6)) | {0} for i in range(N)]
        rows[0] = set(range(N))
        ip = np.zeros(N + 1, dtype=np.uint32)
        ip[1:] = np.cumsum([len(r) for r in rows])
        ix = np.concatenate([np.array(sorted(r), dtype=np.uint32) for r in rows])
        X = rng.standard_normal((N, SIZES[0])).astype(np.float32)
        Y = rng.integers(0, SIZES[-1], size=(N, 1)).astype(np.int32)
        w = lambda a, b: (rng.standard_normal((a, b)) / np.sqrt(a)).astype(np.float32)
        bias = lambda b: (0.1 * rng.standard_normal((1, b))).astype(np.float32)
        gcn_w = [(w(a, b), bias(b)) for a, b in zip(SIZES[:-1], SIZES[1:])]
        sage_w = [(w(a, b), bias(b), w(a, b), bias(b)) for a, b in zip(SIZES[:-1], SIZES[1:])]
        _data["g"] = (ip, ix, np.ones(ix.size, dtype=np.float32), X, Y, {"gcn": gcn_w, "sage": sage_w})
    return _data["g"]


def _make(pkg, kind, weights=None, **kw):
    ip, ix, dv, X, Y, W = _graph()
    A = pkg.csr_matrix(ip.copy(), ix.copy(), dv.copy(), N)
    weights = W[kind] if weights is None else weights
    model = pkg.gcn(A, SIZES, weights=weights, **kw) if kind == "gcn" else pkg.sage(A, SIZES, aggr="mean", weights=weights, **kw)
    return model, pkg.dn_matrix.from_numpy(X.copy()), pkg.dn_matrix.from_numpy(Y.copy())


def _weights(kind, model):
    """the model's current parameters in the shape of its ``weights=`` argument"""
    if kind == "gcn":
        return [(l.W().numpy().copy(), l.b().numpy().copy()) for l in model.layers()]
    return [(l.lin.W.numpy().copy(), l.lin.b.numpy().copy(), l.res_lin.W.numpy().copy(), l.res_lin.b.numpy().copy())
            for l in model.layers()]


def _param_bits(model):
    out = []
    for layer in model.layers():
        for _, owner in layer.owners():
            for _, p, *_ in owner.params_table:
                out.append(getattr(owner, p).numpy().view(np.uint32).copy())
    return out


def _restated_forward(model, fanout, keep, rescale, epoch):
    """the forward matrix of training forward ``epoch``: the restated sample of model.A_T, rescaled (float64 row factors)"""
    F = model.A_T
    thr = es_ref.thresholds(F.indptr, fanout, keep)
    if rescale == "row":
        scale = vref.row_factors(F.indptr, F.indices, F.data, thr, seed=SEED, epoch=epoch)[0].astype(np.float32)
    else:
        scale = vref.inverse_factors(thr)
    _, sp, sx, sv = vref.sample_val(F.indptr, F.indices, F.data, thr, 0, scale, rescale == "row", seed=SEED, epoch=epoch)
    return sp, sx, sv


# ---- identity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_identity_setting_gives_the_unsampled_bits(pkg, ctx, kind):
    """fanout=10**6, edge_rescale="row": every entry is kept and every factor is exactly 1; the four sample passes and the
    device-plan SpMM run, the hub's row is sliced, and three train_steps give the unsampled model's losses and parameters bit
    for bit (a graph this small runs the unsampled model on the host row-split plan with the same split)"""
    plain, X, Y = _make(pkg, kind)
    want = [plain.train_step(ctx, X, Y, *ADAM) for _ in range(3)]
    assert not any(t in ctx.timers for t in TIMERS)
    sampled, X, Y = _make(pkg, kind, fanout=10 ** 6, edge_rescale="row")
    sampled.set_sampling(fanout=10 ** 6, seed=SEED)
    got = [sampled.train_step(ctx, X, Y, *ADAM) for _ in range(3)]
    assert got == want
    for i, (a, b) in enumerate(zip(_param_bits(sampled), _param_bits(plain))):
        np.testing.assert_array_equal(a, b, err_msg=f"parameter {i}")
    assert all(t in ctx.timers and ctx.measure(t) > 0.0 for t in TIMERS)
    assert sampled.sample_epoch == 3 and sampled.sampled_forward and sampled.edge_rescale == "row"
    for S, M in zip(sampled.sampler.pair, (sampled.A_T, sampled.A)):
        indptr, indices = S.numpy()
        np.testing.assert_array_equal(indptr, M.indptr)
        np.testing.assert_array_equal(indices, M.indices)
        np.testing.assert_array_equal(S.values_numpy().view(np.uint32), M.data.view(np.uint32))
        assert S.plan.cap_split >= 1 and int(S.plan.read()[2][2]) >= 1         # the hub's row is sliced on both sides


# ---- a real sample -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rescale", ["row", "inverse"])
@pytest.mark.parametrize("fanout,keep", [(None, 0.5), (4, 1.0)])
@pytest.mark.parametrize("kind", KINDS)
def test_sampled_training_follows_the_restatement(pkg, ctx, kind, fanout, keep, rescale):
    """the loss of training forwards 0-2 against float64 forward + loss on each epoch's restated matrix, from the weights the
    device model holds in front of that forward"""
    model, X, Y = _make(pkg, kind, fanout=fanout, edge_keep=keep, edge_rescale=rescale)
    model.set_sampling(fanout=fanout, keep=keep, seed=SEED)
    _, _, _, Xh, Yh, _ = _graph()
    loss_fn = vref.gcn_loss if kind == "gcn" else vref.sage_mean_loss
    full = loss_fn((model.A_T.indptr, model.A_T.indices, model.A_T.data), N, Xh, Yh, _weights(kind, model))
    for epoch in range(3):
        weights = _weights(kind, model)
        want = loss_fn(_restated_forward(model, fanout, keep, rescale, epoch), N, Xh, Yh, weights)
        loss, _ = model.train_step(ctx, X, Y, *ADAM)
        print(f"[edge-sample-val] {kind} fanout={fanout} keep={keep} {rescale} epoch {epoch}: loss {loss:.7f}, restated {want:.7f}, "
              f"relative error {abs(loss - want) / abs(want):.2e}")
        assert abs(loss - want) <= TOL * abs(want), (epoch, loss, want)
        if epoch == 0:
            assert abs(loss - full) > TOL * abs(full)                        # and the sample is not the full graph
    assert model.sample_epoch == 3
    S = model.sampler.pair[0]
    assert 0 < S.nnz() < model.A_T.nnz()


@pytest.mark.parametrize("kind", KINDS)
def test_an_epoch_replays(pkg, ctx, kind):
    a, X, Y = _make(pkg, kind, edge_keep=0.5, edge_rescale="row")
    a.set_sampling(keep=0.5, seed=SEED)
    first, second = a.train_forward(ctx, X, Y), a.train_forward(ctx, X, Y)      # forwards 0 and 1 from the same weights
    assert first != second
    b, X, Y = _make(pkg, kind, edge_rescale="row")
    b.set_sampling(keep=0.5, seed=SEED, epoch=1)
    assert b.train_forward(ctx, X, Y) == second and b.sample_epoch == 2
    b.set_sampling(keep=0.5, seed=SEED, epoch=0, rescale="inverse")
    assert b.train_forward(ctx, X, Y) != first and b.edge_rescale == "inverse"  # another rescale is another matrix


@pytest.mark.parametrize("kind", KINDS)
def test_other_forwards_keep_the_full_graphs_bits(pkg, ctx, kind):
    model, X, Y = _make(pkg, kind, fanout=4, edge_rescale="row")
    model.set_sampling(fanout=4, seed=SEED)
    for _ in range(2):
        model.train_step(ctx, X, Y, *ADAM)
    assert model.sampled_forward
    twin, Xt, Yt = _make(pkg, kind, weights=_weights(kind, model))             # never sampled
    out = model(ctx, X)
    ctx.sync()
    assert not model.sampled_forward
    want = twin(ctx, Xt)
    ctx.sync()
    np.testing.assert_array_equal(out.numpy().view(np.uint32), want.numpy().view(np.uint32))
    assert model.evaluate(ctx, X, Y) == twin.evaluate(ctx, Xt, Yt)
    assert model.sample_epoch == 2                                              # neither moved the epoch
    if kind == "sage":                                                          # the kept agg(X) is the full graph's, untouched
        l0, t0 = model.layers()[0], twin.layers()[0]
        assert l0._M_sampled is not None and l0.M is not l0._M_sampled
        np.testing.assert_array_equal(l0.M.numpy().view(np.uint32), t0.M.numpy().view(np.uint32))
        before = l0.M.numpy().copy()
        model.train_step(ctx, X, Y, *ADAM)
        np.testing.assert_array_equal(l0.M.numpy(), before)


OPTIONS = [("gcn", dict(dropout=0.5)), ("gcn", dict(norm="layer")), ("gcn", dict(loss="bce")), ("gcn", dict(residual_layer=True)),
           ("gcn", dict(fused=False)), ("sage", dict(dropout=0.5)), ("sage", dict(norm="layer")), ("sage", dict(loss="bce")),
           ("sage", dict(fused=False))]


@pytest.mark.parametrize("kind,kw", OPTIONS, ids=lambda v: v if isinstance(v, str) else "-".join(f"{k}={x}" for k, x in v.items()))
def test_options_compose(pkg, ctx, kind, kw):
    model, X, Y = _make(pkg, kind, fanout=4, edge_keep=0.75, edge_rescale="row", **kw)
    model.set_sampling(fanout=4, keep=0.75, seed=SEED)
    if kw.get("loss") == "bce":
        rng = np.random.default_rng(3)
        Y = pkg.dn_matrix.from_numpy(rng.integers(0, 2, size=(N, SIZES[-1])).astype(np.int32))
    for _ in range(2):
        loss, score = model.train_step(ctx, X, Y, *ADAM)
        assert np.isfinite(loss) and loss > 0.0
    assert all(np.isfinite(p.view(np.float32)).all() for p in _param_bits(model))
    assert model.sample_epoch == 2 and all(t in ctx.timers for t in TIMERS)


def test_bf16_aggregation_on_a_sample(pkg, ctx):
    """gcn(agg_dtype="bf16") on a sample: the restatement with every aggregated operand rounded to bf16, at the bf16 tests' bar"""
    model, X, Y = _make(pkg, "gcn", edge_keep=0.5, edge_rescale="row", agg_dtype="bf16")
    model.set_sampling(keep=0.5, seed=SEED)
    _, _, _, Xh, Yh, _ = _graph()
    for epoch in range(2):
        weights = _weights("gcn", model)
        F = _restated_forward(model, None, 0.5, "row", epoch)
        want = vref.gcn_loss(F, N, Xh, Yh, weights, round_operand=vref.bf16_round)
        loss, _ = model.train_step(ctx, X, Y, *ADAM)
        print(f"[edge-sample-val] bf16 epoch {epoch}: loss {loss:.7f}, restated {want:.7f}")
        assert abs(loss - want) <= TOL * abs(want), (epoch, loss, want)


@pytest.mark.parametrize("kind", KINDS)
def test_off_owns_nothing(pkg, ctx, kind):
    for kw in (dict(), dict(edge_rescale="row"), dict(edge_rescale="inverse", fanout=None, edge_keep=1.0)):
        model, X, Y = _make(pkg, kind, **kw)
        model.train_step(ctx, X, Y, *ADAM)
        assert model.sampler is None and not model.sampled_forward and model.sample_epoch == 0
        assert not any(t in ctx.timers for t in TIMERS)
        agg = model.layers()[0].A if kind == "gcn" else model.layers()[0].agg
        assert agg.sample is None
    model.set_sampling(fanout=4, seed=SEED)                  # on ...
    model.train_step(ctx, X, Y, *ADAM)
    assert model.sampler is not None and model.sampler.plans is not None
    model.set_sampling()                                     # ... and off again: the sampler and its plans are gone
    model.train_step(ctx, X, Y, *ADAM)
    assert model.sampler is None and not model.sampled_forward and agg.sample is None


def test_device_side_refusals(pkg, ctx):
    model, X, Y = _make(pkg, "gcn", edge_rescale="row")
    model.set_sampling(fanout=4)
    with pytest.raises(ValueError, match="hoist_first_aggregation"):
        model.set_hoist_first_aggregation(True)
    model.set_sampling()
    model.set_hoist_first_aggregation(True)
    with pytest.raises(ValueError, match="hoist_first_aggregation"):
        model.set_sampling(fanout=4)
    assert model.sampler is None
