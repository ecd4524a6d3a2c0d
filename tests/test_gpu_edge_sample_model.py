"""Per-epoch edge sampling in the models (gat of all three variants, sage(aggr="max")) on the device, on the small model data
of test_gpu_gat.py / test_gpu_sage.py: the identity setting gives the unsampled model's bits, real sampling follows the
project's CPU reference models on the restated sample of every epoch at the bars those tests already use, an epoch replays,
every forward that is not a training forward keeps the full graph's bits, "off" owns nothing, the options compose, and the
device-side refusals."""
import numpy as np
import pytest

import edge_sample_ref as es_ref
import gat_ref
import sage_ref
from gat_ref import relerr

pytestmark = pytest.mark.gpu

TOL = 1e-4                          # test_gpu_gat.py's bar
ADAM = (1e-2, 0.9, 0.999, 5e-4, 1e-8)
N = 1024                            # test_gpu_gat.py's model data
GAT_SIZES, HEADS = [48, 32, 32, 7], 4
SAGE_N, SAGE_SIZES = 300, [24, 32, 32, 7]          # test_gpu_sage.py's
SEED = 0xABCDEF0123456789
TIMERS = ("sample-count", "sample-scan", "sample-compact")


@pytest.fixture()
def ctx(pkg):
    return pkg.context(0)           # a context per test: its timers are this test's


_data = {}


def _gat_data(pkg):
    if "gat" not in _data:
        ip, ix, dv = pkg.datasets.synth_powerlaw_csr(N, N * 24, 1200, seed=len(GAT_SIZES) + GAT_SIZES[0])
        rng = np.random.default_rng(0)
        X = rng.standard_normal((N, GAT_SIZES[0]), dtype=np.float32)
        Y = rng.integers(0, GAT_SIZES[-1], size=(N, 1)).astype(np.int32)
        _data["gat"] = ((ip, ix, dv), X, Y)
    return _data["gat"]


def _sage_data(pkg):
    if "sage" not in _data:
        ip, ix, dv = pkg.datasets.synth_powerlaw_csr(SAGE_N, 3000, 80, seed=5)
        rng = np.random.default_rng(len(SAGE_SIZES))
        cls = rng.integers(0, SAGE_SIZES[-1], size=SAGE_N)
        centres = rng.standard_normal((SAGE_SIZES[-1], SAGE_SIZES[0]))
        X = (centres[cls] + 0.7 * rng.standard_normal((SAGE_N, SAGE_SIZES[0]))).astype(np.float32)
        _data["sage"] = ((ip, ix, dv), X, cls.reshape(SAGE_N, 1).astype(np.int32), sage_ref.init_weights(SAGE_SIZES))
    return _data["sage"]


def _csr(pkg, csr, n):
    ip, ix, dv = csr
    return pkg.csr_matrix(ip.copy(), ix.copy(), dv.copy(), n)


def _make(pkg, kind, csr=None, **kw):
    """kind: "v1" | "v2" | "dot" | "sage"; (model, X, Y on the device, host X, host Y)"""
    if kind == "sage":
        c, X, Y, weights = _sage_data(pkg)
        model = pkg.sage(_csr(pkg, csr or c, SAGE_N), SAGE_SIZES, aggr="max", weights=weights, **kw)
    else:
        c, X, Y = _gat_data(pkg)
        model = pkg.gat(_csr(pkg, csr or c, N), GAT_SIZES, heads=HEADS, variant=kind, **kw)
    return model, pkg.dn_matrix.from_numpy(X.copy()), pkg.dn_matrix.from_numpy(Y.copy()), X, Y


def _param_bits(model):
    out = []
    for layer in model.layers():
        for _, owner in layer.owners():
            for _, p, *_ in owner.params_table:
                out.append(getattr(owner, p).numpy().view(np.uint32).copy())
    return out


def _same_bits(a, b):
    assert len(a) == len(b) and len(a) > 0
    for i, (x, y) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(x, y, err_msg=f"parameter {i}")


def _forward_pattern(model):
    """(indptr, indices) of the matrix the model's forward walks, and of the one its backward walks"""
    F_T = model._A_sorted if hasattr(model, "_A_sorted") else model.A
    return (model.A_T.indptr, model.A_T.indices), (F_T.indptr, F_T.indices)


def _restated(model, fanout, keep, seed, epoch):
    """the restated sample of the model's two matrices, each from the matrix itself"""
    (fp, fx), (tp, tx) = _forward_pattern(model)
    thr = es_ref.thresholds(fp, fanout, keep)
    _, sp, sx = es_ref.sample(fp, fx, thr, 0, seed=seed, epoch=epoch)
    _, stp, stx = es_ref.sample(tp, tx, thr, 1, seed=seed, epoch=epoch)
    return (sp, sx), (stp, stx)


# ---- identity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["v1", "v2", "dot", "sage"])
def test_identity_setting_gives_the_unsampled_bits(pkg, ctx, kind):
    """set_sampling(fanout=10**6): every q is 1, the three kernels still run, and three train_steps give the losses and every
    parameter of the unsampled model bit for bit"""
    plain, X, Y, _, _ = _make(pkg, kind)
    want = [plain.train_step(ctx, X, Y, *ADAM) for _ in range(3)]
    assert not any(t in ctx.timers for t in TIMERS)
    sampled, X, Y, _, _ = _make(pkg, kind)
    sampled.set_sampling(fanout=10 ** 6, seed=SEED)
    got = [sampled.train_step(ctx, X, Y, *ADAM) for _ in range(3)]
    assert got == want
    _same_bits(_param_bits(sampled), _param_bits(plain))
    assert all(t in ctx.timers and ctx.measure(t) > 0.0 for t in TIMERS)
    assert sampled.sample_epoch == 3 and sampled.sampled_forward
    for d, (hp, hx) in zip(sampled.sampler.pair, _forward_pattern(sampled)):
        indptr, indices = d.numpy()
        np.testing.assert_array_equal(indptr, hp)
        np.testing.assert_array_equal(indices, hx)
    # the constructor keywords are the same switch
    ctor, X, Y, _, _ = _make(pkg, kind, fanout=10 ** 6)
    assert ctor.sampler is not None and ctor.sample_fanout == 10 ** 6
    assert [ctor.train_step(ctx, X, Y, *ADAM) for _ in range(3)] == want


# ---- real sampling against the CPU reference models --------------------------------------------------------------------------
SETTINGS = [dict(fanout=None, keep=0.5), dict(fanout=4, keep=1.0)]


@pytest.mark.parametrize("setting", SETTINGS, ids=["keep0.5", "fanout4"])
def test_gat_epochs_on_the_sample_match_the_reference(pkg, oracle, ctx, setting):
    """three epochs of gat v1 against gat_ref.oracle_gat whose matrix is replaced each epoch by the restated sample of that
    epoch; the bars are test_gpu_gat.py's (loss and every gradient at TOL, accuracy within 3 / n)"""
    csr, X, Y = _gat_data(pkg)
    G, Xd, Yd, _, _ = _make(pkg, "v1")
    G.set_sampling(seed=SEED, **setting)
    ip, ix, dv = csr
    O = gat_ref.oracle_gat(oracle, oracle.Csr(ip.copy(), ix.copy(), dv.copy(), N), GAT_SIZES, [HEADS, HEADS, 1])
    np.testing.assert_array_equal(O.indptr, G.A_T.indptr)
    np.testing.assert_array_equal(O.indices, G.A_T.indices)
    full = (O.indptr.copy(), O.indices.copy())
    kept = []
    for epoch in range(3):
        for layer, ol in zip(G.layers(), O.layers):             # identical inputs, as test_gpu_gat.py's _sync_oracle_state
            ol.lin.W, ol.lin.b, ol.att = layer.W().numpy().copy(), layer.b().numpy().copy(), layer.att().numpy().copy()
        loss, acc = G.train_forward(ctx, Xd, Yd)
        G.backward(ctx)
        ctx.sync()
        grads = [(l.GW().numpy().copy(), l.Gb().numpy().copy(), l.Gatt().numpy().copy()) for l in G.layers()]
        (sp, sx), (stp, stx) = _restated(G, setting["fanout"], setting["keep"], SEED, epoch)
        for d, (hp, hx) in zip(G.sampler.pair, ((sp, sx), (stp, stx))):           # the device drew the restated sample
            indptr, indices = d.numpy()
            np.testing.assert_array_equal(indptr, hp)
            np.testing.assert_array_equal(indices, hx)
        kept.append(sx.size)
        G.adam_update(ctx, *ADAM)
        O.indptr, O.indices = sp, sx
        ol_, oa = O.train_forward(X, Y)
        O.backward()
        print(f"[edge-sample] gat {setting} epoch {epoch}: kept {sx.size} of {full[1].size}, loss {loss!r} "
              f"(reference {ol_!r}), acc {acc!r} ({oa!r})")
        assert abs(loss - ol_) <= TOL * abs(ol_), (epoch, loss, ol_)
        assert abs(acc - oa) <= 3.0 / N, (epoch, acc, oa)
        for li, (g, ol) in enumerate(zip(grads, O.layers)):
            for name, a, b in zip(("G_W", "G_b", "G_att"), g, (ol.lin.G_W, ol.lin.G_b, ol.G_att)):
                d = relerr(a, b)
                print(f"[edge-sample] gat {setting} epoch {epoch} layer {li} {name}: {d:.3e}")
                assert d <= TOL, (epoch, li, name, d)
    assert len(set(kept)) == 3 and max(kept) < 0.8 * full[1].size                # a fresh, real sample every epoch
    assert G.sample_epoch == 3


def _dist(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / max(np.abs(want).max(), 1e-300))


@pytest.mark.parametrize("setting", SETTINGS, ids=["keep0.5", "fanout4"])
def test_sage_max_epochs_on_the_sample_match_the_reference(pkg, ctx, setting):
    """three epochs of sage(aggr="max") against sage_ref.Sage on the restated sample of each epoch, by the rules of
    test_gpu_sage.py: the selection exactly on the device's own bits, the arithmetic at eight times the fp32 twin's worst
    distance from the fp64 restatement with the device's selection"""
    model, Xd, Yd, X, Y = _make(pkg, "sage")
    model.set_sampling(seed=SEED, **setting)
    L = len(SAGE_SIZES) - 1
    full_nnz = model.A_T.nnz()
    for epoch in range(3):
        weights = [(l.lin.W.numpy().copy(), l.lin.b.numpy().copy(), l.res_lin.W.numpy().copy(), l.res_lin.b.numpy().copy())
                   for l in model.layers()]
        dev_loss, _ = model.train_forward(ctx, Xd, Yd)
        layers = model.layers()
        logits = layers[-1].Y.numpy().copy()
        (sp, sx), (stp, stx) = _restated(model, setting["fanout"], setting["keep"], SEED, epoch)
        for d, (hp, hx) in zip(model.sampler.pair, ((sp, sx), (stp, stx))):
            indptr, indices = d.numpy()
            np.testing.assert_array_equal(indptr, hp)
            np.testing.assert_array_equal(indices, hx)
        assert sx.size < 0.8 * full_nnz
        args = [None] * L
        assert layers[0].agg.arg is None and layers[0].M is None        # no selection stored, the kept agg(X) untouched
        want_M0, _ = sage_ref.agg_max(sp, sx, X)
        assert (layers[0]._M_used.numpy().view(np.uint32) == want_M0.view(np.uint32)).all()
        for l in range(1, L):
            want_M, want_arg = sage_ref.agg_max(sp, sx, layers[l].H.numpy())
            arg = layers[l].agg.arg.numpy().view(np.uint32)
            assert (arg == want_arg).all(), (epoch, l)
            assert (layers[l].M.numpy().view(np.uint32) == want_M.view(np.uint32)).all(), (epoch, l)
            args[l] = arg.copy()
        model.backward(ctx)
        ctx.sync()
        dev = {"loss": np.array([dev_loss], dtype=np.float64), "logits": logits}
        for l, layer in enumerate(layers):
            dev.update({f"W_l{l}": layer.lin.G_W.numpy(), f"b_l{l}": layer.lin.G_b.numpy(),
                        f"W_r{l}": layer.res_lin.G_W.numpy(), f"b_r{l}": layer.res_lin.G_b.numpy()})
        model.adam_update(ctx, *ADAM)
        runs = {}
        for dtype in (np.float64, np.float32):
            R = sage_ref.Sage((sp, sx, np.ones(sx.size, dtype=np.float32)), SAGE_SIZES, weights, "max", dtype)
            lv = R.train_forward(X, Y, args)
            t = {"loss": np.array([lv], dtype=np.float64), "logits": R.logits}
            for l, g in enumerate(R.backward()):
                t.update({f"{k}{l}": v for k, v in g.items()})
            runs[dtype] = t
        want, twin = runs[np.float64], runs[np.float32]
        assert set(dev) == set(want)
        twin_worst = max(_dist(twin[k], want[k]) for k in want)
        dev_dist = {k: _dist(dev[k], want[k]) for k in want}
        worst = max(dev_dist, key=dev_dist.get)
        print(f"[edge-sample] sage {setting} epoch {epoch}: kept {sx.size} of {full_nnz}, twin worst {twin_worst:.3e}, "
              f"device worst {dev_dist[worst]:.3e} ({worst}), ratio {dev_dist[worst] / twin_worst:.2f} of 8")
        assert 0 < twin_worst < 1e-4
        assert dev_dist[worst] <= 8.0 * twin_worst, (epoch, worst, dev_dist[worst], twin_worst)


# ---- replay ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["v1", "sage"])
def test_set_sampling_replays_an_epoch(pkg, ctx, kind):
    model, X, Y, _, _ = _make(pkg, kind)
    model.set_sampling(fanout=6, keep=0.7, seed=SEED)
    runs = []
    for _ in range(3):
        loss = model.train_forward(ctx, X, Y)
        ctx.sync()
        runs.append((loss, [a.tobytes() for d in model.sampler.pair for a in d.numpy()], model.layers()[-1].Z.numpy().tobytes()
                     if kind != "sage" else model.layers()[-1].Y.numpy().tobytes()))
    assert model.sample_epoch == 3 and len({r[1][1] for r in runs}) == 3
    model.set_sampling(fanout=6, keep=0.7, seed=SEED, epoch=1)
    again = model.train_forward(ctx, X, Y)
    ctx.sync()
    out = model.layers()[-1].Y if kind == "sage" else model.layers()[-1].Z
    assert again == runs[1][0] and model.sample_epoch == 2
    assert [a.tobytes() for d in model.sampler.pair for a in d.numpy()] == runs[1][1] and out.numpy().tobytes() == runs[1][2]


# ---- everything that is not a training forward keeps the full graph ------------------------------------------------------------
@pytest.mark.parametrize("kind", ["v1", "v2", "sage"])
def test_plain_forwards_keep_their_bits(pkg, ctx, kind):
    plain, X, Y, _, _ = _make(pkg, kind)
    sampled, _, _, _, _ = _make(pkg, kind, edge_keep=0.5, fanout=8)

    def observe(m):
        out = m(ctx, X)
        ctx.sync()
        res = [out.numpy().copy(), m.predict(ctx, X), m.evaluate(ctx, X, Y)]
        if kind != "sage":
            alphas = m.attention_weights(ctx, X)
            ctx.sync()                                          # the export is enqueued on the compute stream
            res += [a.numpy().copy() for a in alphas]
        return res

    want = observe(plain)
    for when in ("before", "after"):
        got = observe(sampled)
        assert len(got) == len(want)
        for i, (a, b) in enumerate(zip(got, want)):
            assert (a == b) if isinstance(a, dict) else (np.asarray(a).tobytes() == np.asarray(b).tobytes()), (when, i)
        assert not sampled.sampled_forward
        if when == "before":
            assert sampled.sample_epoch == 0                    # no epoch was spent
            l_s, l_p = sampled.train_forward(ctx, X, Y), plain.train_forward(ctx, X, Y)
            assert l_s != l_p and sampled.sample_epoch == 1 and sampled.sampled_forward
    if kind == "sage":                                          # the kept agg(X) of layer 0 is the full graph's, computed once
        assert sampled.layers()[0].agg.launches == 1 + 1        # one full-graph aggregate, one sampled


def test_model_selector_validates_on_the_full_graph(pkg, ctx):
    S = (np.arange(N) % 3).astype(np.int32)
    sampled, X, Y, _, _ = _make(pkg, "v1", edge_keep=0.5)
    sampled.set_splits(S)
    sel = pkg.model_selector(sampled, split="val")
    assert sel.clean
    sel.step(ctx, X, Y, *ADAM)
    twin, _, _, _, _ = _make(pkg, "v1")                          # the same parameters on the full graph
    twin.set_splits(S)
    for a, b in zip(twin.layers(), sampled.layers()):
        for (_, oa), (_, ob) in zip(a.owners(), b.owners()):
            for _, p, *_ in oa.params_table:
                getattr(ob, p).copy_to(ctx, getattr(oa, p))
    twin.loss_layer(ctx, twin(ctx, X), Y)
    assert sel.history[0] == twin.split_metrics()["val"][0]
    assert not pkg.model_selector(twin, split="val").clean


# ---- off ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["v1", "sage"])
def test_off_owns_nothing(pkg, ctx, kind):
    model, X, Y, _, _ = _make(pkg, kind)
    model.train_step(ctx, X, Y, *ADAM)
    assert model.sampler is None and not any(t in ctx.timers for t in TIMERS) and not model.sampled_forward
    assert (model.sample_fanout, model.sample_keep, model.sample_epoch) == (None, 1.0, 0)
    model.set_sampling(keep=0.5)
    assert model.sampler is not None and model.sampler.pair is None             # buffers come with the first draw
    model.set_sampling()                                                        # and off again frees them
    model.train_step(ctx, X, Y, *ADAM)
    assert model.sampler is None and not any(t in ctx.timers for t in TIMERS)


# ---- composition ---------------------------------------------------------------------------------------------------------------
def test_options_compose_on_the_sample(pkg, ctx):
    """one epoch with dropout 0.5, attention dropout 0.3, skip="gate", norm="layer", label_input=0.5 and agg_dtype="bf16" on a
    real sample equals, bit for bit, the same model built over a csr_matrix of the restated sample with the identity setting
    (both go through the sampled path)"""
    csr, _, _ = _gat_data(pkg)
    kw = dict(dropout=0.5, attn_dropout=0.3, skip="gate", norm="layer", label_input=0.5, agg_dtype="bf16")
    fanout, keep = 8, 0.75
    S = (np.arange(N) % 3).astype(np.int32)

    def run(model, X, Y, **sampling):
        model.set_splits(pkg.dn_matrix.from_numpy(S.reshape(-1, 1)))
        model.set_label_input(Y, seed=5)
        model.set_dropout(0.5, seed=11, attn=0.3)
        model.set_sampling(seed=SEED, **sampling)
        res = model.train_step(ctx, X, Y, *ADAM)
        assert model.sampled_forward and np.isfinite(res[0])
        return res, _param_bits(model)

    first, X, Y, _, _ = _make(pkg, "v1", **kw)
    got = run(first, X, Y, fanout=fanout, keep=keep)
    # A of the second model: the restated sample of A itself (rows are sources: the transposed side)
    ip, ix, dv = csr
    F = gat_ref.transpose_pattern(ip, ix, N)
    thr = es_ref.thresholds(F[0], fanout, keep)
    _, ap, ax = es_ref.sample(ip, ix, thr, 1, seed=SEED, epoch=0)
    assert 0.2 * ix.size < ax.size < 0.9 * ix.size
    second, X, Y, _, _ = _make(pkg, "v1", csr=(ap, ax, np.ones(ax.size, dtype=np.float32)), **kw)
    (sp, sx), _ = _restated(first, fanout, keep, SEED, 0)
    np.testing.assert_array_equal(second.A_T.indptr, sp)         # its forward matrix is the restated sample of F, in order
    np.testing.assert_array_equal(second.A_T.indices, sx)
    want = run(second, X, Y, fanout=10 ** 6)
    assert got[0] == want[0]
    _same_bits(got[1], want[1])


# ---- the device-side refusals --------------------------------------------------------------------------------------------------
def test_export_after_a_sampled_forward_and_edge_attr_are_refused(pkg, ctx):
    model, X, Y, _, _ = _make(pkg, "v1", edge_keep=0.5)
    model.train_forward(ctx, X, Y)
    with pytest.raises(ValueError, match="sampl"):
        model.attention_weights(ctx)
    with pytest.raises(ValueError, match="sampl"):
        model.layers()[0].alpha(ctx)
    alphas = model.attention_weights(ctx, X)                                    # with X: a plain forward on the full graph
    assert alphas[0].shape() == (model.A_T.nnz(), HEADS)
    model.attention_weights(ctx)                                                # and now the state is the full graph's
    csr, _, _ = _gat_data(pkg)
    E = np.ones((csr[1].size, 2), dtype=np.float32)
    with pytest.raises(ValueError, match="edge_attr"):
        _make(pkg, "v1", edge_attr=E, fanout=4)
    with_E, _, _, _, _ = _make(pkg, "v1", edge_attr=E)
    with pytest.raises(ValueError, match="edge_attr"):
        with_E.set_sampling(keep=0.5)
    assert with_E.sampler is None
