"""The GraphSAGE model (mg-gcn_amd/sage.py) on the GPU against tests/sage_ref.py: n = 300 from datasets.synth_powerlaw_csr
(unsorted rows, duplicate entries, self-loops), sizes [24, 32, 32, 7] and [20, 12, 5], mean and max, the plain model,
norm="layer", dropout=0.5 and loss="bce".

Selection and arithmetic are checked apart, so that a near-tie hides nothing.  SELECTION: for every max layer that keeps one,
the layer's input is copied from the device and the device's M and arg must equal sage_ref.agg_max on those very bits,
exactly.  ARITHMETIC: the fp64 restatement runs with the device's args -- the model is then a smooth function -- and the
loss, the logits and every parameter gradient are compared with it.  The distance of a tensor is max |x - want| / max |want|;
the bar of a case is EIGHT TIMES the fp32 twin's worst distance over all of these tensors on the same input and the same args
(the rule of cs_ref.model_case: the device adds in another order than the twin, and nothing of the bar comes from the
device).  The worst device / twin ratio over the sixteen cases is printed ([sage] lines) and stands in DESIGN.md 3.13."""
import numpy as np
import pytest

import dropout_ref
import sage_ref as ref

pytestmark = pytest.mark.gpu

N = 300
SIZES = ([24, 32, 32, 7], [20, 12, 5])
CONFIGS = {"plain": {}, "norm": dict(norm="layer"), "dropout": dict(dropout=0.5), "bce": dict(loss="bce")}
ADAM = (1e-2, 0.9, 0.999, 5e-4, 1e-8)
SEED = 11


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


_data = {}


def _inputs(pkg, sizes, loss="softmax"):
    """graph, planted classes (the features are a class centre plus noise), targets; made once and left unchanged"""
    key = (tuple(sizes), loss)
    if key not in _data:
        ip, ix, dv = pkg.datasets.synth_powerlaw_csr(N, 3000, 80, seed=5)
        rng = np.random.default_rng(len(sizes))
        cls = rng.integers(0, sizes[-1], size=N)
        centres = rng.standard_normal((sizes[-1], sizes[0]))
        X = (centres[cls] + 0.7 * rng.standard_normal((N, sizes[0]))).astype(np.float32)
        if loss == "bce":
            Y = (np.arange(sizes[-1])[None, :] == cls[:, None]).astype(np.int32)
            Y |= (rng.random(Y.shape) < 0.1).astype(np.int32)
        else:
            Y = cls.reshape(N, 1).astype(np.int32)
        for a in (ip, ix, dv, X, Y):
            a.setflags(write=False)
        _data[key] = dict(ip=ip, ix=ix, dv=dv, X=X, Y=Y, weights=ref.init_weights(sizes))
    return _data[key]


def _model(pkg, d, sizes, aggr, **kw):
    A = pkg.csr_matrix(d["ip"].copy(), d["ix"].copy(), d["dv"].copy(), N)
    return pkg.sage(A, sizes, aggr=aggr, weights=d["weights"], **kw)


def _device(pkg, d):
    return pkg.dn_matrix.from_numpy(d["X"].copy()), pkg.dn_matrix.from_numpy(d["Y"].copy())


def _param_bits(model):
    out = []
    for layer in model.layers():
        for _, owner in layer.owners():
            for _, p, *_ in owner.params_table:
                out.append(getattr(owner, p).numpy().view(np.uint32).copy())
    return out


def _dist(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / max(np.abs(want).max(), 1e-300))


def _tensors(loss, logits, grads):
    out = {"loss": np.array([loss], dtype=np.float64), "logits": logits}
    for l, g in enumerate(grads):
        for name, t in g.items():
            out[f"{name}{l}"] = t
    return out


@pytest.mark.parametrize("sizes", SIZES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("aggr", ["mean", "max"])
def test_selection_exactly_and_arithmetic_at_eight_times_the_twin(pkg, ctx, aggr, config, sizes):
    kw = CONFIGS[config]
    loss_kind = kw.get("loss", "softmax")
    d = _inputs(pkg, sizes, loss_kind)
    model = _model(pkg, d, sizes, aggr, **kw)
    p = kw.get("dropout", 0.0)
    if p:
        model.set_dropout(p, seed=SEED)
    X, Y = _device(pkg, d)
    L = len(sizes) - 1
    dev_loss, _ = model.train_forward(ctx, X, Y)
    layers = model.layers()
    logits = layers[-1].Y.numpy().copy()
    F = (model.A_T.indptr, model.A_T.indices, model.A_T.data)
    # ---- selection: exactly, on the device's own bits
    args = [None] * L
    if aggr == "max":
        assert layers[0].agg.arg is None                       # layer 0 stores no selection
        for l in range(1, L):
            H = layers[l].H.numpy()
            want_M, want_arg = ref.agg_max(F[0], F[1], H)
            arg = layers[l].agg.arg.numpy().view(np.uint32)
            assert (arg == want_arg).all(), (l, np.argwhere(arg != want_arg)[:4].tolist())
            assert (layers[l].M.numpy().view(np.uint32) == want_M.view(np.uint32)).all(), l
            args[l] = arg.copy()
        want_M0, _ = ref.agg_max(F[0], F[1], d["X"])
        assert (layers[0].M.numpy().view(np.uint32) == want_M0.view(np.uint32)).all()
        assert (model.A.data == d["dv"]).all()                 # the values of A: unused and unchanged
    model.backward(ctx)
    ctx.sync()
    # ---- arithmetic: fp64 and its fp32 twin with the device's args and the device's masks
    masks = [None] * L
    if p:
        scale = dropout_ref.params(p)[1]
        masks = [None] + [(dropout_ref.mask(N, sizes[l], 0, p, SEED, l), scale) for l in range(1, L)]      # epoch 0: stream l
    runs = {}
    for dtype in (np.float64, np.float32):
        R = ref.Sage(F, sizes, d["weights"], aggr, dtype, norm=kw.get("norm"), loss=loss_kind, masks=masks)
        lv = R.train_forward(d["X"], d["Y"], args)
        runs[dtype] = _tensors(lv, R.logits, R.backward())
    want, twin = runs[np.float64], runs[np.float32]
    dev_grads = []
    for layer in layers:
        g = dict(W_l=layer.lin.G_W.numpy(), b_l=layer.lin.G_b.numpy(), W_r=layer.res_lin.G_W.numpy(), b_r=layer.res_lin.G_b.numpy())
        if layer.norm is not None:
            g.update(gamma=layer.norm.G_gamma.numpy(), beta=layer.norm.G_beta.numpy())
        dev_grads.append(g)
    dev = _tensors(dev_loss, logits, dev_grads)
    assert set(dev) == set(want)
    twin_worst = max(_dist(twin[k], want[k]) for k in want)
    dev_dist = {k: _dist(dev[k], want[k]) for k in want}
    worst = max(dev_dist, key=dev_dist.get)
    bar = 8.0 * twin_worst
    print(f"[sage] {aggr} {config} {sizes}: twin worst {twin_worst:.3e}, device worst {dev_dist[worst]:.3e} ({worst}), "
          f"ratio {dev_dist[worst] / twin_worst:.2f} of 8")
    assert 0 < twin_worst < 1e-4
    assert dev_dist[worst] <= bar, (worst, dev_dist[worst], bar)


def _plain(ctx, model, X):
    out = model(ctx, X)
    ctx.sync()
    return out.numpy().copy()


def _steps(ctx, model, X, Y, k):
    return [model.train_step(ctx, X, Y, *ADAM)[0] for _ in range(k)]


@pytest.mark.parametrize("aggr", ["mean", "max"])
def test_same_bits_from_two_models_and_from_both_adam_modes(pkg, ctx, aggr):
    sizes = SIZES[0]
    d = _inputs(pkg, sizes)
    X, Y = _device(pkg, d)
    got = []
    for fused in (True, True, False):
        model = _model(pkg, d, sizes, aggr, norm="layer", dropout=0.5, fused=fused)
        model.set_dropout(0.5, seed=SEED)
        losses = _steps(ctx, model, X, Y, 3)
        got.append((losses, _param_bits(model)))
    for losses, bits in got[1:]:
        assert losses == got[0][0]
        assert len(bits) == len(got[0][1]) and all((a == b).all() for a, b in zip(bits, got[0][1]))


@pytest.mark.parametrize("aggr", ["mean", "max"])
def test_trains_and_aggregates_the_features_once(pkg, ctx, aggr):
    sizes = SIZES[0]
    d = _inputs(pkg, sizes)
    X, Y = _device(pkg, d)
    model = _model(pkg, d, sizes, aggr)
    losses = _steps(ctx, model, X, Y, 30)
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    agg0, agg1 = model.layers()[0].agg, model.layers()[1].agg
    assert agg0.launches == 1 and agg1.launches == 30           # layer 0's aggregate is loop-invariant
    model(ctx, X)
    assert agg0.launches == 1
    model.reset_input_cache()
    model(ctx, X)
    model(ctx, X)
    assert agg0.launches == 2
    X2 = pkg.dn_matrix.from_numpy(d["X"].copy())                      # another buffer: another key
    model(ctx, X2)
    assert agg0.launches == 3


@pytest.mark.parametrize("aggr", ["mean", "max"])
def test_evaluate_and_predict_never_drop(pkg, ctx, aggr):
    sizes = SIZES[1]
    d = _inputs(pkg, sizes)
    X, Y = _device(pkg, d)
    clean = _model(pkg, d, sizes, aggr)
    dropping = _model(pkg, d, sizes, aggr, dropout=0.5)
    dropping.set_dropout(0.5, seed=SEED)
    want = clean.predict(ctx, X)
    assert (dropping.predict(ctx, X) == want).all() and (dropping.predict(ctx, X) == want).all()
    assert dropping.evaluate(ctx, X, Y) == clean.evaluate(ctx, X, Y)
    assert dropping.dropout_epoch == 0                          # no training forward has run: no epoch was spent
    plain = _plain(ctx, dropping, X)
    dropped_loss, _ = dropping.train_forward(ctx, X, Y)
    clean_loss, _ = clean.train_forward(ctx, X, Y)
    assert dropping.dropout_epoch == 1 and dropped_loss != clean_loss
    assert (_plain(ctx, clean, X) == plain).all() and (_plain(ctx, dropping, X) == plain).all()


def test_save_raises_and_creates_nothing(pkg, ctx, tmp_path):
    sizes = SIZES[1]
    d = _inputs(pkg, sizes)
    model = _model(pkg, d, sizes, "max")
    X, Y = _device(pkg, d)
    model.set_splits(np.arange(N) % 3)
    sel = pkg.model_selector(model, split="val")
    sel.step(ctx, X, Y, *ADAM)
    path = tmp_path / "sage.ckpt"
    for call in (lambda: model.save(ctx, str(path)), lambda: model.load(ctx, str(path)), lambda: sel.save_best(ctx, str(path))):
        with pytest.raises(ValueError, match="sage"):
            call()
    assert list(tmp_path.iterdir()) == []
    sel.restore(ctx)                                            # the in-memory restore works
