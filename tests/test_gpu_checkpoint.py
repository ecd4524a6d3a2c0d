"""save / load / predict and model_selector on one GPU (gcn): a resumed run is the uninterrupted run bit for bit, a
refused load changes nothing, a file without the optimiser section resets Adam, execution options are free, and the
selector agrees with the test's own bookkeeping.  The engine is run-to-run deterministic (test_gpu_gcn.py::
test_train_step_equals_the_three_calls), so parameters and moments are compared as uint32 views, never with a tolerance;
the loss scalars are float atomic sums over workgroups and get that test's 2e-6 relative bar."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ADAM = (1e-2, 0.9, 0.999, 5e-4, 1e-8)
N = 1024
RES_SIZES = [24, 16, 32, 16, 6]          # one residual linear where the widths differ, plain adds where they do not
SIZES = [24, 16, 16, 5]
SEED64 = 0xFEDCBA9876543210
LOSS_BAR = 2e-6                          # test_gpu_gcn.py:296: two runs of the same kernels


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


@pytest.fixture(scope="module")
def graph(pkg):
    return pkg.datasets.synth_powerlaw_csr(N, 20 * N, 900)


def _A(pkg, graph):
    ip, ix, dv = graph
    return pkg.csr_matrix(ip, ix, dv.copy(), N)                # the model normalises its matrix in place


CONFIGS = {
    "plain": dict(sizes=SIZES, kw={}, splits=False),
    "res-norm-dropout-splits": dict(sizes=RES_SIZES, kw=dict(residual_layer=True, norm="layer"), splits=True,
                                    dropout=(0.5, SEED64)),
    "bce-splits": dict(sizes=SIZES, kw=dict(loss="bce"), splits=True),
}


def _inputs(pkg, cfg, seed=3):
    rng = np.random.default_rng(seed)
    sizes = cfg["sizes"]
    X = rng.standard_normal((N, sizes[0]), dtype=np.float32)
    if cfg["kw"].get("loss") == "bce":
        Y = (rng.random((N, sizes[-1])) < 0.3).astype(np.int32)
    else:
        Y = rng.integers(0, sizes[-1], size=(N, 1)).astype(np.int32)
    S = rng.integers(0, 3, size=N).astype(np.int32)
    return pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y), S


def _model(pkg, graph, cfg, S, **extra):
    G = pkg.gcn(_A(pkg, graph), cfg["sizes"], **dict(cfg["kw"], **extra))
    if cfg["splits"]:
        G.set_splits(S)
    if "dropout" in cfg:
        G.set_dropout(*cfg["dropout"])
    return G


def _state(pkg, G, ctx):
    """name -> uint32 view of every parameter and every Adam moment"""
    ctx.sync()
    out = {}
    for name, owner, p, m, v in pkg.checkpoint.model_params(G):
        out[name] = getattr(owner, p).numpy().view(np.uint32)
        if getattr(owner, m) is not None:
            out["m." + name] = getattr(owner, m).numpy().view(np.uint32)
            out["v." + name] = getattr(owner, v).numpy().view(np.uint32)
    return out


def _steps(pkg, G):
    return [o.step for o in pkg.checkpoint.model_owners(G)]


def _garbage(pkg, G):
    for _, owner, p, _, _ in pkg.checkpoint.model_params(G):
        t = getattr(owner, p)
        t.init(np.full(t.shape(), 123.0, dtype=np.float32))


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_resume_is_exact(pkg, ctx, graph, tmp_path, name, fused):
    """A trains six epochs; B trains three and saves; C, a fresh object overwritten with garbage, loads and trains three"""
    cfg = CONFIGS[name]
    X, Y, S = _inputs(pkg, cfg)
    path = str(tmp_path / "b.ckpt")
    A = _model(pkg, graph, cfg, S, fused=fused)
    la = [A.train_step(ctx, X, Y, *ADAM)[0] for _ in range(6)]
    B = _model(pkg, graph, cfg, S, fused=fused)
    initial = _state(pkg, B, ctx)
    for _ in range(3):
        B.train_step(ctx, X, Y, *ADAM)
    B.save(ctx, path)
    C = _model(pkg, graph, cfg, S, fused=fused)
    _garbage(pkg, C)
    C.set_dropout(0.0)
    C.load(ctx, path)
    assert (C.dropout_p, C.dropout_seed, C.dropout_epoch) == (B.dropout_p, B.dropout_seed, B.dropout_epoch)
    _same(_state(pkg, C, ctx), _state(pkg, B, ctx))
    lc = [C.train_step(ctx, X, Y, *ADAM)[0] for _ in range(3)]
    sa, sc = _state(pkg, A, ctx), _state(pkg, C, ctx)
    _same(sc, sa)
    assert _steps(pkg, C) == _steps(pkg, A) == [6] * len(_steps(pkg, A))
    assert (C.dropout_p, C.dropout_seed, C.dropout_epoch) == (A.dropout_p, A.dropout_seed, A.dropout_epoch)
    assert C.dropout_epoch == (6 if "dropout" in cfg else 0)
    print("losses", la[3:], lc)
    for a, c in zip(la[3:], lc):
        assert abs(a - c) <= LOSS_BAR * abs(a), (la, lc)
    for k in initial:                                          # not vacuous: training moved every tensor
        assert (sc[k] != initial[k]).any(), k
    # saving what was loaded and trained gives the bytes of the uninterrupted run's file
    pa, pc = str(tmp_path / "a6.ckpt"), str(tmp_path / "c6.ckpt")
    A.save(ctx, pa)
    C.save(ctx, pc)
    assert open(pa, "rb").read() == open(pc, "rb").read()


def test_a_refused_load_changes_nothing(pkg, ctx, graph, tmp_path):
    ds = pkg.datasets
    cfg = CONFIGS["plain"]
    X, Y, S = _inputs(pkg, cfg)
    G = _model(pkg, graph, cfg, S)
    G.set_dropout(0.25, 5, 3)
    G.train_step(ctx, X, Y, *ADAM)
    before, drop, steps = _state(pkg, G, ctx), (G.dropout_p, G.dropout_seed, G.dropout_epoch), _steps(pkg, G)
    rng = np.random.default_rng(0)
    others = {"sizes": dict(sizes=[24, 16, 5]), "norm": dict(norm="layer"), "loss": dict(loss="bce"),
              "residual_layer": dict(residual_layer=True)}
    for field, change in others.items():
        c = dict({"sizes": SIZES, "residual_layer": False, "norm": None, "loss": "softmax", "dropout": (0.5, 9, 9),
                  "step": 4, "optimizer": True}, **change)
        tensors = {k + nm: rng.standard_normal(shape, dtype=np.float32)
                   for nm, shape in ds.checkpoint_tensors(c["sizes"], c["residual_layer"], c["norm"]) for k in ("", "m.", "v.")}
        path = str(tmp_path / f"{field}.ckpt")
        ds.write_checkpoint(path, c, tensors)
        with pytest.raises(ValueError, match=f"{field}: file .*, model ") as e:
            G.load(ctx, path)
        assert path in str(e.value)
        _same(_state(pkg, G, ctx), before)
        assert (G.dropout_p, G.dropout_seed, G.dropout_epoch) == drop and _steps(pkg, G) == steps
    with pytest.raises(ValueError, match=r"sizes: file \[24, 16, 5\], model \[24, 16, 16, 5\]"):
        G.load(ctx, str(tmp_path / "sizes.ckpt"))


def test_a_file_without_the_optimiser_section_resets_adam(pkg, ctx, graph, tmp_path):
    cfg = CONFIGS["plain"]
    X, Y, S = _inputs(pkg, cfg)
    path = str(tmp_path / "weights.ckpt")
    B = _model(pkg, graph, cfg, S)
    for _ in range(2):
        B.train_step(ctx, X, Y, *ADAM)
    B.save(ctx, path, optimizer=False)
    file_cfg, tensors = pkg.datasets.read_checkpoint(path)
    assert not file_cfg["optimizer"] and file_cfg["step"] == 0 and sorted(tensors) == sorted(f"{k}{l}" for k in "Wb" for l in range(3))
    C = _model(pkg, graph, cfg, S)
    C.train_step(ctx, X, Y, *ADAM)                             # moments exist and are not zero
    table = C._adam
    assert table is not None
    C.load(ctx, path)
    st = _state(pkg, C, ctx)
    for k, v in st.items():
        if k[:2] in ("m.", "v."):
            assert not v.any(), k                              # +0.0 in every bit
    assert _steps(pkg, C) == [0] * 3
    D = pkg.gcn(_A(pkg, graph), SIZES, weights=[(tensors[f"W{l}"], tensors[f"b{l}"]) for l in range(3)])
    lc, ld = C.train_step(ctx, X, Y, *ADAM), D.train_step(ctx, X, Y, *ADAM)
    _same(_state(pkg, C, ctx), _state(pkg, D, ctx))
    assert _steps(pkg, C) == [1] * 3 and C._adam is table      # the cached Adam table's raw pointers stayed valid
    assert abs(lc[0] - ld[0]) <= LOSS_BAR * abs(ld[0]) and lc[1] == ld[1]


def test_execution_options_are_free(pkg, ctx, graph, tmp_path):
    """a file from the fp32 fused model loads into the bf16-aggregation and into the unfused model; each next-epoch loss
    against the fp32 fused model's from the same state at the form's own bar: 1e-4, TOL of test_gpu_agg_bf16.py:239 (the
    bf16 model) and TOL of test_gpu_gcn.py:161 (fused and unfused alike)"""
    cfg = CONFIGS["plain"]
    X, Y, S = _inputs(pkg, cfg)
    path = str(tmp_path / "f.ckpt")
    F = _model(pkg, graph, cfg, S)
    for _ in range(2):
        F.train_step(ctx, X, Y, *ADAM)
    F.save(ctx, path)
    want = F.train_step(ctx, X, Y, *ADAM)[0]
    for extra in (dict(agg_dtype="bf16"), dict(fused=False), dict(fused=False, agg_dtype="bf16", hoist_first_aggregation=False)):
        M = _model(pkg, graph, cfg, S, **extra)
        M.load(ctx, path)
        got = M.train_step(ctx, X, Y, *ADAM)[0]
        print("next-epoch loss", extra, got, want, abs(got - want) / abs(want))
        assert abs(got - want) <= 1e-4 * abs(want), (extra, got, want)
        assert _steps(pkg, M) == [3] * 3


def _selection_data(pkg):
    """random labels: validation loss turns upward once the model fits the train split"""
    cfg = dict(CONFIGS["plain"], splits=True)
    X, Y, S = _inputs(pkg, cfg, seed=17)
    return cfg, X, Y, S


# lr = 5e-2 overshoots on this data: the validation loss drops to 1.6157 at epoch 1, bounces to 1.674 and creeps back below
# its first minimum by epoch 11, so the minimum is the LAST epoch and patience = 2 would stop at epoch 3 with another best.  At
# 1e-2 the unconstrained run falls to 1.6068 at epoch 7 and turns upward (1.6090, 1.6141, ...): the learning rate used here.
SELECT_LR = 1e-2
SELECT_ADAM = (SELECT_LR,) + ADAM[1:]


@pytest.fixture(scope="module")
def recorded(pkg, ctx, graph):
    """the test's own bookkeeping of a twelve-epoch run under the selector (clean=False): host copies of the parameters
    before every step, split_metrics()["val"] after it"""
    cfg, X, Y, S = _selection_data(pkg)
    G = _model(pkg, graph, cfg, S)
    sel = pkg.model_selector(G, clean=False)
    copies, val = [], []
    for _ in range(12):
        copies.append({k: v.copy() for k, v in _state(pkg, G, ctx).items() if k[:2] not in ("m.", "v.")})
        out = sel.step(ctx, X, Y, *SELECT_ADAM)
        m = G.split_metrics()
        assert out == m["train"]
        val.append(m["val"])
    return dict(G=G, sel=sel, copies=copies, val=val)


def test_selector_agrees_with_the_tests_own_bookkeeping(pkg, ctx, recorded, tmp_path):
    G, sel, copies, val = (recorded[k] for k in ("G", "sel", "copies", "val"))
    losses = [v[0] for v in val]
    print("val losses", losses)
    first_min = int(np.argmin(losses))
    assert first_min < len(losses) - 1                          # precondition: the minimum is strictly before the last epoch
    assert sel.history == losses
    assert sel.best_epoch == first_min and sel.best_value == losses[first_min] and not sel.stop
    sel.save_best(ctx, str(tmp_path / "best.ckpt"))
    sel.restore(ctx)
    st = _state(pkg, G, ctx)
    for k, want in copies[first_min].items():
        np.testing.assert_array_equal(st[k], want, err_msg=k)
        assert not st["m." + k].any() and not st["v." + k].any()
    assert _steps(pkg, G) == [0] * 3
    file_cfg, tensors = pkg.datasets.read_checkpoint(str(tmp_path / "best.ckpt"))
    assert not file_cfg["optimizer"] and sorted(tensors) == sorted(copies[first_min])
    for k, want in copies[first_min].items():
        np.testing.assert_array_equal(tensors[k].view(np.uint32), want, err_msg=k)


def test_selector_patience_and_score(pkg, ctx, graph, recorded):
    cfg, X, Y, S = _selection_data(pkg)
    losses, scores = [v[0] for v in recorded["val"]], [v[1] for v in recorded["val"]]
    # patience = 2: the first epoch e with e - (first argmin of losses[:e + 1]) >= 2
    want_stop = next(e for e in range(len(losses)) if e - int(np.argmin(losses[:e + 1])) >= 2)
    G = _model(pkg, graph, cfg, S)
    sel = pkg.model_selector(G, patience=2, clean=False)
    ran = 0
    while not sel.stop and ran < 12:
        sel.step(ctx, X, Y, *SELECT_ADAM)
        ran += 1
    assert sel.stop and ran == want_stop + 1, (ran, want_stop, losses)
    np.testing.assert_allclose(sel.history, losses[:ran], rtol=LOSS_BAR)      # a second run of the same kernels
    assert sel.best_epoch == int(np.argmin(losses[:ran]))
    assert sel.best_epoch == recorded["sel"].best_epoch
    G = _model(pkg, graph, cfg, S)
    sel = pkg.model_selector(G, metric="score", clean=False)
    for _ in range(12):
        sel.step(ctx, X, Y, *SELECT_ADAM)
    assert sel.history == scores and sel.best_epoch == int(np.argmax(scores)) and sel.best_value == max(scores)


def test_selector_needs_splits_on_a_real_model(pkg, graph):
    G = pkg.gcn(_A(pkg, graph), SIZES)
    with pytest.raises(ValueError, match="set_splits"):
        pkg.model_selector(G)
    with pytest.raises(ValueError, match="metric"):
        pkg.model_selector(G, metric="auc")


def test_clean_selection_under_dropout(pkg, ctx, graph):
    """clean=True: history[e] is the validation loss of a plain forward on the post-update parameters, and the extra
    forward spends no dropout epoch"""
    cfg = CONFIGS["res-norm-dropout-splits"]
    X, Y, S = _inputs(pkg, cfg)
    G = _model(pkg, graph, cfg, S)
    T = _model(pkg, graph, cfg, S)                              # the test's twin: same seed, no selector
    sel = pkg.model_selector(G)
    assert sel.clean and not pkg.model_selector(G, clean=False).clean
    for e in range(4):
        sel.step(ctx, X, Y, *ADAM)
        T.train_step(ctx, X, Y, *ADAM)
        assert G.dropout_epoch == T.dropout_epoch == e + 1
        _same(_state(pkg, G, ctx), _state(pkg, T, ctx))          # the next training forward drew the next epoch's mask
        T.loss_layer(ctx, T(ctx, X), Y)
        want = T.split_metrics()["val"][0]
        assert T.dropout_epoch == e + 1
        print("clean val loss", e, sel.history[e], want)
        assert abs(sel.history[e] - want) <= LOSS_BAR * abs(want), (e, sel.history, want)
    dropped = [T.train_step(ctx, X, Y, *ADAM), T.split_metrics()["val"][0]][1]
    assert abs(dropped - sel.history[-1]) > 1e-3 * abs(dropped)  # and it is not the dropped forward's number


def test_predict_is_the_plain_forward(pkg, ctx, graph):
    for name in ("res-norm-dropout-splits", "bce-splits"):
        cfg = CONFIGS[name]
        X, Y, S = _inputs(pkg, cfg)
        G = _model(pkg, graph, cfg, S)
        G.train_step(ctx, X, Y, *ADAM)
        epoch = G.dropout_epoch
        pred = G.predict(ctx, X)
        logits = G(ctx, X)
        ctx.sync()
        logits = logits.numpy()
        assert pred.dtype == np.int32 and G.dropout_epoch == epoch
        if name == "bce-splits":
            assert pred.shape == logits.shape
            np.testing.assert_array_equal(pred, (logits > 0).astype(np.int32))
        else:
            assert pred.shape == (N, 1)
            np.testing.assert_array_equal(pred[:, 0], np.argmax(logits, axis=1))      # the first maximum wins in both
