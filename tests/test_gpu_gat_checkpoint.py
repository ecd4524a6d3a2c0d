"""save / load / predict and model_selector of gat on one GPU: a resumed run is the uninterrupted run bit for bit (both
variants, both dropouts, fused and per-tensor Adam on either side of the file), a load is in place, a refused load changes
nothing, a file without the optimiser section resets Adam, predict is the plain forward, the selector agrees with
split_metrics(), and the C++ command line refuses an attention model's file by name.

The engine is run-to-run deterministic and the masks are counter-based (test_gpu_gat_dropout.py), so parameters and
moments are compared as uint32 views, never with a tolerance.  n = 256 with about 8 entries per row, three empty rows and
one row of 80 entries in the matrix and in its transpose; sizes [16, 32, 32, 5] with heads [4, 2, 1]."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mg-gcn_amd", "bin", "mg_gcn")
ADAM = (1e-2, 0.9, 0.999, 5e-4, 1e-8)
N = 256
SIZES = [16, 32, 32, 5]
HEADS = [4, 2, 1]
SEED64 = 0xFEDCBA9876543210
LOSS_BAR = 2e-6                          # test_gpu_gcn.py:296: two runs of the same kernels


def graph_256():
    """(indptr, indices, data) of A: rows 3, 100 and 255 are empty and row 7 has 80 entries; columns 5, 130 and 200 never
    occur and column 11 occurs in 80 rows, so A.transpose() -- the matrix the forward walks -- has the same features"""
    rng = np.random.default_rng(2024)
    cols_ok = np.setdiff1d(np.arange(N), [5, 130, 200])
    long_col_rows = set(rng.choice(np.setdiff1d(np.arange(N), [3, 100, 255]), size=80, replace=False).tolist())
    rows = []
    for i in range(N):
        if i in (3, 100, 255):
            rows.append(np.zeros(0, dtype=np.int64))
            continue
        k = 80 if i == 7 else int(rng.integers(5, 12))
        c = set(rng.choice(cols_ok, size=k, replace=False).tolist()) - {11}
        if i in long_col_rows:
            c.add(11)
        rows.append(np.array(sorted(c), dtype=np.int64))
    indptr = np.zeros(N + 1, dtype=np.int32)
    indptr[1:] = np.cumsum([r.size for r in rows])
    indices = np.concatenate(rows).astype(np.int32)
    return indptr, indices, np.ones(indices.size, dtype=np.float32)


def inputs(loss="softmax", seed=3):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, SIZES[0]), dtype=np.float32)
    Y = (rng.random((N, SIZES[-1])) < 0.3).astype(np.int32) if loss == "bce" else rng.integers(0, SIZES[-1], size=(N, 1)).astype(np.int32)
    S = rng.integers(0, 3, size=N).astype(np.int32)
    return X, Y, S


CONFIGS = {
    "v1-both-dropouts": dict(variant="v1", dropout=0.5, attn_dropout=0.3),
    "v2-dropout": dict(variant="v2", dropout=0.5),
    "v1-bce": dict(variant="v1", dropout=0.5, attn_dropout=0.3, loss="bce"),
}


def state_bits(pkg, G):
    """name -> uint32 view of every parameter and every Adam moment (the caller has synchronised)"""
    out = {}
    for name, owner, p, m, v in pkg.checkpoint.model_params(G):
        out[name] = getattr(owner, p).numpy().view(np.uint32).copy()
        if getattr(owner, m) is not None:
            out["m." + name] = getattr(owner, m).numpy().view(np.uint32).copy()
            out["v." + name] = getattr(owner, v).numpy().view(np.uint32).copy()
    return out


def differences(a, b):
    return [k for k in sorted(set(a) | set(b)) if k not in a or k not in b or not np.array_equal(a[k], b[k])]


def host_state(G):
    """what load restores besides the tensors"""
    return (G.dropout_p, G.attn_dropout_p, G.dropout_seed, G.dropout_epoch)


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


@pytest.fixture(scope="module")
def graph():
    ip, ix, dv = graph_256()
    counts = np.diff(ip)
    back = np.bincount(ix, minlength=N)
    assert (counts == 0).sum() == 3 and counts.max() == 80 and (back == 0).sum() == 3 and back.max() == 80
    assert 7 <= counts.mean() <= 9
    return ip, ix, dv


def _A(pkg, graph):
    ip, ix, dv = graph
    return pkg.csr_matrix(ip.copy(), ix.copy(), dv.copy(), N)


def _gat(pkg, graph, seed=True, **kw):
    G = pkg.gat(_A(pkg, graph), SIZES, heads=HEADS, **kw)
    if seed:
        G.set_dropout(G.dropout_p, SEED64)
    return G


def _steps(pkg, G):
    return [o.step for o in pkg.checkpoint.model_owners(G)]


def _garbage(pkg, G):
    for _, owner, p, _, _ in pkg.checkpoint.model_params(G):
        t = getattr(owner, p)
        t.init(np.full(t.shape(), 123.0, dtype=np.float32))


def _same(a, b):
    assert not differences(a, b), differences(a, b)


def _dn(pkg, *arrays):
    return [pkg.dn_matrix.from_numpy(a) for a in arrays]


@pytest.fixture(scope="module")
def uninterrupted(pkg, ctx, graph, tmp_path_factory):
    """per configuration, once: A trains four epochs and saves; B trains two and saves"""
    base = tmp_path_factory.mktemp("gat_ckpt")
    made = {}

    def get(name):
        if name not in made:
            kw = CONFIGS[name]
            X, Y = _dn(pkg, *inputs(kw.get("loss", "softmax"))[:2])
            A = _gat(pkg, graph, **kw)
            la = [A.train_step(ctx, X, Y, *ADAM)[0] for _ in range(4)]
            B = _gat(pkg, graph, **kw)
            ctx.sync()
            initial = state_bits(pkg, B)
            for _ in range(2):
                B.train_step(ctx, X, Y, *ADAM)
            pa, pb = str(base / f"{name}_a4.ckpt"), str(base / f"{name}_b2.ckpt")
            A.save(ctx, pa)
            B.save(ctx, pb)
            made[name] = dict(A=A, B=B, la=la, pa=pa, pb=pb, initial=initial, X=X, Y=Y, sa=state_bits(pkg, A), sb=state_bits(pkg, B))
        return made[name]
    return get


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_resume_is_exact(pkg, ctx, graph, uninterrupted, tmp_path, name, fused):
    """C, a fresh model with neither dropout, its parameters overwritten with garbage, loads B's file (written by a fused
    model) and trains two epochs: it is A, which trained four"""
    kw, u = CONFIGS[name], uninterrupted(name)
    A, B, X, Y = u["A"], u["B"], u["X"], u["Y"]
    C = _gat(pkg, graph, seed=False, variant=kw["variant"], loss=kw.get("loss", "softmax"), fused=fused)
    _garbage(pkg, C)
    assert host_state(C) == (0.0, 0.0, 0, 0)
    C.load(ctx, u["pb"])
    assert host_state(C) == (0.5, kw.get("attn_dropout", 0.0), SEED64, 2)
    ctx.sync()
    _same(state_bits(pkg, C), u["sb"])
    assert _steps(pkg, C) == [2] * 6
    lc = [C.train_step(ctx, X, Y, *ADAM)[0] for _ in range(2)]
    ctx.sync()
    sc = state_bits(pkg, C)
    _same(sc, u["sa"])
    assert len(sc) == 27                                        # W, b, att and both moments of each, three layers
    assert _steps(pkg, C) == _steps(pkg, A) == [4] * 6
    assert host_state(C) == host_state(A) == (0.5, kw.get("attn_dropout", 0.0), SEED64, 4)
    print("losses", u["la"][2:], lc)
    for a, c in zip(u["la"][2:], lc):
        assert np.isfinite(a) and abs(a - c) <= LOSS_BAR * abs(a), (u["la"], lc)
    for k in u["initial"]:                                      # not vacuous: training moved every tensor
        assert (sc[k] != u["initial"][k]).any(), k
    pc = str(tmp_path / "c4.ckpt")
    C.save(ctx, pc)
    assert open(pc, "rb").read() == open(u["pa"], "rb").read()
    assert open(pc, "rb").read() != open(u["pb"], "rb").read()
    cfg, tensors = pkg.datasets.read_checkpoint(pc)
    assert cfg == {"model": "gat", "variant": kw["variant"], "sizes": SIZES, "heads": HEADS, "attn_slope": 0.2,
                   "attn_dropout": kw.get("attn_dropout", 0.0), "residual_layer": False, "norm": None,
                   "loss": kw.get("loss", "softmax"), "dropout": (0.5, SEED64, 4), "step": 4, "optimizer": True}
    for k, v in sc.items():
        np.testing.assert_array_equal(tensors[k].view(np.uint32), v, err_msg=k)


def test_load_is_in_place(pkg, ctx, graph, uninterrupted):
    """a model that has stepped (its fused Adam table holds raw pointers) loads a file and steps once: bitwise a fresh
    model that loaded the file and stepped once"""
    u = uninterrupted("v1-both-dropouts")
    X, Y = u["X"], u["Y"]
    M = _gat(pkg, graph, **CONFIGS["v1-both-dropouts"])
    M.set_dropout(0.25, 77, 9, attn=0.5)
    for _ in range(3):
        M.train_step(ctx, X, Y, *ADAM)
    table = M._adam
    addresses = [getattr(o, a).t.data_ptr() for _, o, p, m, v in pkg.checkpoint.model_params(M) for a in (p, m, v)]
    assert table is not None
    M.load(ctx, u["pb"])
    F = _gat(pkg, graph, seed=False, variant="v1")
    F.load(ctx, u["pb"])
    lm, lf = M.train_step(ctx, X, Y, *ADAM), F.train_step(ctx, X, Y, *ADAM)
    ctx.sync()
    _same(state_bits(pkg, M), state_bits(pkg, F))
    assert M._adam is table
    assert addresses == [getattr(o, a).t.data_ptr() for _, o, p, m, v in pkg.checkpoint.model_params(M) for a in (p, m, v)]
    assert _steps(pkg, M) == _steps(pkg, F) == [3] * 6 and host_state(M) == host_state(F) == (0.5, 0.3, SEED64, 3)
    assert abs(lm[0] - lf[0]) <= LOSS_BAR * abs(lf[0]) and lm[1] == lf[1]
    assert abs(lm[0] - u["la"][2]) <= LOSS_BAR * abs(lm[0])      # and it is the uninterrupted run's third epoch


def _host_file(pkg, path, **change):
    """a well-formed attention file of random tensors whose configuration differs from the model's in ``change``"""
    ds = pkg.datasets
    c = dict({"model": "gat", "variant": "v1", "sizes": SIZES, "heads": HEADS, "attn_slope": 0.2, "attn_dropout": 0.0,
              "loss": "softmax", "dropout": (0.5, 9, 9), "step": 4, "optimizer": True}, **change)
    rng = np.random.default_rng(0)
    names = ds.checkpoint_tensors(c["sizes"], False, None, model=c["model"], variant=c.get("variant"))
    ds.write_checkpoint(path, c, {k + nm: rng.standard_normal(shape, dtype=np.float32) for nm, shape in names for k in ("", "m.", "v.")})
    return path


def test_a_refused_load_changes_nothing(pkg, ctx, graph, uninterrupted, tmp_path):
    u = uninterrupted("v1-both-dropouts")
    G = _gat(pkg, graph, variant="v1")
    G.set_dropout(0.25, 5, 3, attn=0.125)
    G.train_step(ctx, u["X"], u["Y"], *ADAM)
    ctx.sync()
    before, host, steps = state_bits(pkg, G), host_state(G), _steps(pkg, G)
    assert host == (0.25, 0.125, 5, 4)
    others = {"model": dict(model="gcn", variant=None), "variant": dict(variant="v2"), "heads": dict(heads=[2, 2, 1]),
              "sizes": dict(sizes=[16, 32, 5], heads=[4, 1]), "loss": dict(loss="bce"), "attn_slope": dict(attn_slope=0.1)}
    messages = {"model": "model: file gcn, model gat", "variant": "variant: file v2, model v1",
                "heads": r"heads: file \[2, 2, 1\], model \[4, 2, 1\]", "sizes": r"sizes: file \[16, 32, 5\], model \[16, 32, 32, 5\]",
                "loss": "loss: file bce, model softmax", "attn_slope": "attn_slope: file 0.1, model 0.2"}
    for field, change in others.items():
        path = _host_file(pkg, str(tmp_path / f"{field}.ckpt"), **change)
        with pytest.raises(ValueError, match=messages[field]) as e:
            G.load(ctx, path)
        assert path in str(e.value)
        ctx.sync()
        _same(state_bits(pkg, G), before)
        assert host_state(G) == host and _steps(pkg, G) == steps
    # v1 into v2, and an attention file into gcn: the targets stay as they were built
    V2 = _gat(pkg, graph, variant="v2")
    K = pkg.gcn(_A(pkg, graph), SIZES)
    for M, message in ((V2, "variant: file v1, model v2"), (K, "model: file gat, model gcn")):
        ctx.sync()
        was, was_host = state_bits(pkg, M), (M.dropout_p, M.dropout_seed, M.dropout_epoch)
        with pytest.raises(ValueError, match=message) as e:
            M.load(ctx, u["pb"])
        assert u["pb"] in str(e.value)
        ctx.sync()
        _same(state_bits(pkg, M), was)
        assert (M.dropout_p, M.dropout_seed, M.dropout_epoch) == was_host == (0.0, SEED64 if M is V2 else 0, 0)
        assert _steps(pkg, M) == [0] * len(_steps(pkg, M))


def test_a_file_without_the_optimiser_section_resets_adam(pkg, ctx, graph, uninterrupted, tmp_path):
    u = uninterrupted("v2-dropout")
    X, Y = u["X"], u["Y"]
    path = str(tmp_path / "weights.ckpt")
    u["B"].save(ctx, path, optimizer=False)
    cfg, tensors = pkg.datasets.read_checkpoint(path)
    assert not cfg["optimizer"] and cfg["step"] == 0 and cfg["dropout"] == (0.5, SEED64, 2)
    assert sorted(tensors) == sorted(f"{k}{l}" for k in ("W", "b", "att") for l in range(3))
    for k, v in tensors.items():
        np.testing.assert_array_equal(v.view(np.uint32), u["sb"][k], err_msg=k)
    C = _gat(pkg, graph, variant="v2")
    C.train_step(ctx, X, Y, *ADAM)                              # moments exist and are not zero
    table = C._adam
    C.load(ctx, path)
    ctx.sync()
    st = state_bits(pkg, C)
    for k, v in st.items():
        if k[:2] in ("m.", "v."):
            assert not v.any(), k                               # +0.0 in every bit
        else:
            np.testing.assert_array_equal(v, u["sb"][k], err_msg=k)
    assert _steps(pkg, C) == [0] * 6
    D = _gat(pkg, graph, variant="v2", dropout=0.5, weights=[(tensors[f"W{l}"], tensors[f"b{l}"], tensors[f"att{l}"]) for l in range(3)])
    D.set_dropout(0.5, SEED64, 2)
    lc, ld = C.train_step(ctx, X, Y, *ADAM), D.train_step(ctx, X, Y, *ADAM)
    ctx.sync()
    _same(state_bits(pkg, C), state_bits(pkg, D))
    assert _steps(pkg, C) == [1] * 6 and C._adam is table
    assert abs(lc[0] - ld[0]) <= LOSS_BAR * abs(ld[0]) and lc[1] == ld[1]


@pytest.mark.parametrize("name", ["v1-both-dropouts", "v1-bce"])
def test_predict_is_the_plain_forward(pkg, ctx, uninterrupted, name):
    u = uninterrupted(name)
    G, X = u["B"], u["X"]
    epoch = G.dropout_epoch
    pred = G.predict(ctx, X)
    logits = G(ctx, X)
    ctx.sync()
    logits = logits.numpy()
    assert pred.dtype == np.int32 and G.dropout_epoch == epoch == 2 and np.isfinite(logits).all()
    if name == "v1-bce":
        assert pred.shape == logits.shape == (N, SIZES[-1])
        np.testing.assert_array_equal(pred, (logits > 0).astype(np.int32))
        assert 0 < pred.sum() < pred.size
    else:
        assert pred.shape == (N, 1)
        np.testing.assert_array_equal(pred[:, 0], np.argmax(logits, axis=1))      # the first maximum wins in both
        assert np.unique(pred).size > 1
    np.testing.assert_array_equal(pred, G.predict(ctx, X))


def test_model_selector_on_gat(pkg, ctx, graph, tmp_path):
    """only attention dropout: the default is the clean pass; history, best_epoch and stop against split_metrics() of a twin
    without a selector; restore and save_best against the test's own snapshot of the best epoch.  The score is a count of
    rows over a count of rows and is compared exactly; a loss is a float sum over workgroups and gets LOSS_BAR"""
    X, Y, S = inputs(seed=17)
    X, Y = _dn(pkg, X, Y)

    def model(**kw):
        G = _gat(pkg, graph, variant="v1", **kw)
        G.set_splits(S)
        return G
    G, T = model(attn_dropout=0.3), model(attn_dropout=0.3)
    sel = pkg.model_selector(G, metric="score", patience=3)
    assert sel.clean and not pkg.model_selector(G, clean=False).clean and not pkg.model_selector(model()).clean
    want, snapshots = [], []
    for e in range(8):
        got, twin = sel.step(ctx, X, Y, *ADAM), T.train_step(ctx, X, Y, *ADAM)
        assert abs(got[0] - twin[0]) <= LOSS_BAR * abs(twin[0]) and got[1] == twin[1]
        assert G.dropout_epoch == T.dropout_epoch == e + 1      # the clean pass spends no epoch
        T.loss_layer(ctx, T(ctx, X), Y)
        want.append(T.split_metrics()["val"])
        assert sel.history[e] == G.split_metrics()["val"][1]    # split_metrics() reports the clean pass
        ctx.sync()
        snapshots.append({k: v for k, v in state_bits(pkg, T).items() if k[:2] not in ("m.", "v.")})
        _same(state_bits(pkg, G), state_bits(pkg, T))
        best = int(np.argmax(sel.history))                      # the first best epoch wins a tie
        assert sel.best_epoch == best and sel.best_value == sel.history[best] and sel.stop == (e - best >= 3)
    print("clean val (loss, score)", want, "history", sel.history)
    assert sel.history == [w[1] for w in want]
    best = sel.best_epoch
    path = str(tmp_path / "best.ckpt")
    sel.save_best(ctx, path)
    sel.restore(ctx)
    st = state_bits(pkg, G)
    for k, v in snapshots[best].items():
        np.testing.assert_array_equal(st[k], v, err_msg=k)
        assert not st["m." + k].any() and not st["v." + k].any()
    assert _steps(pkg, G) == [0] * 6
    cfg, tensors = pkg.datasets.read_checkpoint(path)
    assert not cfg["optimizer"] and cfg["model"] == "gat" and sorted(tensors) == sorted(snapshots[best])
    fresh = model()
    fresh.load(ctx, path)
    assert host_state(fresh) == (0.0, 0.3, SEED64, 8)
    ctx.sync()
    _same({k: v for k, v in state_bits(pkg, fresh).items() if k[:2] not in ("m.", "v.")}, snapshots[best])
    ev = fresh.evaluate(ctx, X, Y, pkg.dn_matrix.from_numpy(S))
    print("best epoch", best, "score", sel.history[best], "evaluate of the loaded model", ev)
    assert abs(ev["val"] - sel.history[best]) <= 1e-6           # the same count of rows, divided in float64 and in float32
    for M in (fresh, G):                                        # the restored model is that model too
        M.loss_layer(ctx, M(ctx, X), Y)
        m = M.split_metrics()["val"]
        assert abs(m[0] - want[best][0]) <= LOSS_BAR * abs(m[0]) and m[1] == want[best][1]


def test_cli_refuses_an_attention_models_file(pkg, ctx, golden_dir, tmp_path):
    toy = os.path.join(golden_dir, "toyA")
    features = pkg.datasets.read_dense(os.path.join(toy, "features.bin"), "<f4").shape[1]
    classes = 1 + int(pkg.datasets.read_dense(os.path.join(toy, "labels.bin"), "<i4").max())
    G = pkg.gat(pkg.csr_matrix(os.path.join(toy, "graph.bin")), [features, 8, classes], heads=[2, 1])
    path = str(tmp_path / "gat.ckpt")
    G.save(ctx, path)
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MGGCN_")}
    for command in ("predict", "train"):
        r = subprocess.run([EXE, "-P", "1", command, toy, "1", "8"], cwd=str(tmp_path), env=dict(clean, MGGCN_LOAD=path),
                           capture_output=True, text=True, timeout=120)
        lines = [ln for ln in r.stderr.splitlines() if "model: file gat, model gcn" in ln]
        assert r.returncode != 0 and len(lines) == 1 and path in lines[0], (r.returncode, r.stderr)
        assert "[mggcn predict]" not in r.stderr and not os.path.exists(str(tmp_path / "predictions.bin"))
