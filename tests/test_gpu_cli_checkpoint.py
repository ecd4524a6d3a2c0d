"""Checkpoints, model selection and `predict` of the mg_gcn command line, and the file across the two languages: a resumed
CLI run writes the uninterrupted run's file byte for byte, its epoch column and weight dumps continue, Python's file loads
into the CLI and the CLI's into Python, MGGCN_SAVE_BEST / MGGCN_PATIENCE follow the "[mggcn splits]" lines of the same
run, and `mg_gcn predict` writes what gcn.predict returns."""
import filecmp
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mg-gcn_amd", "bin", "mg_gcn")
ADAM = (1e-2, 0.9, 0.999, 5e-4, 1e-8)        # main.cpp's hyper-parameters
N, F, C = 1024, 24, 5
HIDDEN = [16, 16]
SIZES = [F] + HIDDEN + [C]
TOL = 1e-4                                    # test_gpu_host_cpp.py::test_cli_matches_oracle


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


@pytest.fixture(scope="module")
def data(pkg, tmp_path_factory):
    """random labels and a random three-way split (the data of test_gpu_checkpoint.py's selector tests), on disk"""
    ip, ix, dv = pkg.datasets.synth_powerlaw_csr(N, 20 * N, 900)
    rng = np.random.default_rng(17)
    X = rng.standard_normal((N, F), dtype=np.float32)
    Y = rng.integers(0, C, size=(N, 1)).astype(np.int32)
    Y[0, 0] = C - 1                                              # num_labels = 1 + max(Y)
    S = rng.integers(0, 3, size=N).astype(np.int32)
    Yb = (rng.random((N, C)) < 0.3).astype(np.int32)
    base = tmp_path_factory.mktemp("cli_ckpt")
    d, db = str(base / "permuted" / "synth"), str(base / "permuted" / "synthbce")
    pkg.datasets.write_dataset(d, ip, ix, dv, X, Y, S)
    pkg.datasets.write_dataset(db, ip, ix, dv, X, Yb, S)
    return dict(graph=(ip, ix, dv), X=X, Y=Y, Yb=Yb, S=S, dir=d, dir_bce=db)


def _cli(args, cwd, command="train", dirname=None, **env):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MGGCN_")}
    r = subprocess.run([EXE] + args + [command, dirname, str(len(HIDDEN))] + [str(h) for h in HIDDEN], cwd=str(cwd),
                       env=dict(clean, **{k: str(v) for k, v in env.items()}), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def _epochs(stderr):
    """[(epoch, loss, score)] of the epoch lines"""
    out = []
    for ln in stderr.splitlines():
        t = ln.split()
        if len(t) == 4 and re.fullmatch(r"\d+", t[0]):
            out.append((int(t[0]), float(t[1]), float(t[2])))
    return out


def _model(pkg, data, **kw):
    ip, ix, dv = data["graph"]
    return pkg.gcn(pkg.csr_matrix(ip, ix, dv.copy(), N), SIZES, **kw)


def _bits(tensors):
    return {k: np.ascontiguousarray(v).view(np.uint32) for k, v in tensors.items()}


@pytest.mark.parametrize("form", ["one-gpu", "P2-R1", "one-gpu-dropout-norm-splits"])
def test_cli_resume_writes_the_uninterrupted_runs_file(pkg, data, tmp_path, form):
    args = {"P2-R1": ["-P", "2", "-R", "1"]}.get(form, ["-P", "1"])
    env = {"P2-R1": dict(MGGCN_OVERSUBSCRIBE=1),
           "one-gpu-dropout-norm-splits": dict(MGGCN_DROPOUT=0.5, MGGCN_DROPOUT_SEED=0xFEDCBA9876543210, MGGCN_LAYER_NORM=1,
                                               MGGCN_TRAIN_SET=0)}.get(form, {})
    a, b, c, dumps = (str(tmp_path / x) for x in ("a.ckpt", "b.ckpt", "c.ckpt", "dumps"))
    ra = _cli(args + ["-E", "4"], tmp_path, dirname=data["dir"], MGGCN_SAVE=a, **env)
    _cli(args + ["-E", "2"], tmp_path, dirname=data["dir"], MGGCN_SAVE=b, **env)
    rc = _cli(args + ["-E", "2"], tmp_path, dirname=data["dir"], MGGCN_LOAD=b, MGGCN_SAVE=c, MGGCN_DUMP_WEIGHTS=dumps, **env)
    assert filecmp.cmp(a, c, shallow=False)
    assert not filecmp.cmp(a, b, shallow=False)
    assert [e[0] for e in _epochs(ra.stderr)] == [0, 1, 2, 3] and [e[0] for e in _epochs(rc.stderr)] == [2, 3]
    for (_, la, sa), (_, lc, sc) in zip(_epochs(ra.stderr)[2:], _epochs(rc.stderr)):
        assert abs(la - lc) <= 2e-6 * abs(la) + 1e-6 * abs(la), (la, lc)      # six printed digits of the same sum
    if form == "one-gpu-dropout-norm-splits":
        assert [ln.split()[2] for ln in rc.stderr.splitlines() if ln.startswith("[mggcn splits]")] == ["2", "3"]
    cfg, tensors = pkg.datasets.read_checkpoint(b)
    assert cfg["step"] == 2 and cfg["optimizer"]
    assert cfg["dropout"] == ((0.5, 0xFEDCBA9876543210, 2) if form == "one-gpu-dropout-norm-splits" else (0.0, 0, 0))
    assert cfg["sizes"] == SIZES[:-1] + [6 if form == "P2-R1" else C]            # -R 1 pads the classes to a multiple of P
    names = ["W", "b"] + (["gamma", "beta"] if form == "one-gpu-dropout-norm-splits" else [])
    for l in range(len(SIZES) - 1):
        for nm in names:
            if nm in ("gamma", "beta") and l == len(SIZES) - 2:
                continue
            dumped = pkg.datasets.read_dense(os.path.join(dumps, f"e2_{nm}{l}.bin"), "<f4")
            np.testing.assert_array_equal(dumped.view(np.uint32), tensors[f"{nm}{l}"].view(np.uint32), err_msg=f"{nm}{l}")
    assert sorted(os.listdir(dumps))[0].startswith("e2_")


def test_padded_classes_are_refused_by_name(pkg, data, tmp_path):
    """-R 1 pads the last width to a multiple of P: a -P 1 file (5 classes) does not load into -P 2 -R 1 (6)"""
    f = str(tmp_path / "one.ckpt")
    _cli(["-P", "1", "-E", "1"], tmp_path, dirname=data["dir"], MGGCN_SAVE=f)
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MGGCN_")}
    r = subprocess.run([EXE, "-P", "2", "-R", "1", "-E", "1", "train", data["dir"], "2", "16", "16"], cwd=str(tmp_path),
                       env=dict(clean, MGGCN_OVERSUBSCRIBE="1", MGGCN_LOAD=f), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "sizes: file [24, 16, 16, 5], model [24, 16, 16, 6]" in r.stderr, r.stderr
    assert not _epochs(r.stderr)                                                  # before training starts


def test_the_file_crosses_the_languages(pkg, ctx, data, tmp_path):
    py, cli = str(tmp_path / "py.ckpt"), str(tmp_path / "cli.ckpt")
    X, Y = pkg.dn_matrix.from_numpy(data["X"]), pkg.dn_matrix.from_numpy(data["Y"])
    G = _model(pkg, data)
    for _ in range(2):
        G.train_step(ctx, X, Y, *ADAM)
    G.save(ctx, py)
    want = G.train_forward(ctx, X, Y)[0]
    r = _cli(["-P", "1", "-E", "1"], tmp_path, dirname=data["dir"], MGGCN_LOAD=py, MGGCN_SAVE=cli)
    (e, loss, _), = _epochs(r.stderr)
    print("python next loss", want, "cli", loss)
    assert e == 2 and abs(loss - want) <= TOL * abs(want), (loss, want)
    cfg, tensors = pkg.datasets.read_checkpoint(cli)
    assert cfg["step"] == 3 and cfg["optimizer"] and cfg["sizes"] == SIZES
    H = _model(pkg, data)
    H.load(ctx, cli)
    ctx.sync()
    got = {}
    for name, owner, p, m, v in pkg.checkpoint.model_params(H):
        got[name], got["m." + name], got["v." + name] = (getattr(owner, a).numpy() for a in (p, m, v))
    assert sorted(got) == sorted(tensors)
    for k, v in _bits(tensors).items():
        np.testing.assert_array_equal(_bits(got)[k], v, err_msg=k)
    assert [o.step for o in pkg.checkpoint.model_owners(H)] == [3] * 3


def test_cli_selection_follows_its_own_split_lines(pkg, ctx, data, tmp_path):
    f, epochs = str(tmp_path / "best.ckpt"), 60
    r = _cli(["-P", "1", "-E", str(epochs)], tmp_path, dirname=data["dir"], MGGCN_TRAIN_SET=0, MGGCN_SAVE_BEST=f, MGGCN_PATIENCE=2)
    val, best = [], []
    for ln in r.stderr.splitlines():
        t = ln.split()
        if ln.startswith("[mggcn splits]"):
            val.append((int(t[2]), float(t[t.index("val") + 1]), float(t[t.index("val") + 2])))
        elif ln.startswith("[mggcn best]"):
            best.append((int(t[2]), float(t[3]), float(t[4])))
    print("val", val, "best", best)
    assert [v[0] for v in val] == list(range(len(val)))
    improving, low, since, stop = [], None, 0, None
    for e, loss, score in val:
        if low is None or loss < low:
            improving.append((e, loss, score))
            low, since = loss, 0
        else:
            since += 1
        if since >= 2:
            stop = e
            break
    assert best == improving
    assert stop is not None and stop < epochs - 1                       # the run did turn upward before -E ran out
    assert val[-1][0] == stop and [e[0] for e in _epochs(r.stderr)] == list(range(stop + 1))
    cfg, tensors = pkg.datasets.read_checkpoint(f)
    assert not cfg["optimizer"] and cfg["step"] == 0 and sorted(tensors) == sorted(f"{k}{l}" for k in "Wb" for l in range(3))
    G = _model(pkg, data)
    G.set_splits(data["S"])
    G.load(ctx, f)
    X, Y = pkg.dn_matrix.from_numpy(data["X"]), pkg.dn_matrix.from_numpy(data["Y"])
    G.loss_layer(ctx, G(ctx, X), Y)
    got = G.split_metrics()["val"][0]
    print("best line", best[-1], "python plain forward", got)
    assert abs(got - best[-1][1]) <= TOL * abs(got)


def test_cli_predict_softmax(pkg, oracle, ctx, data, tmp_path):
    f, out = str(tmp_path / "m.ckpt"), str(tmp_path / "pred.bin")
    X, Y, S = (pkg.dn_matrix.from_numpy(data[k]) for k in ("X", "Y", "S"))
    G = _model(pkg, data)
    for _ in range(3):
        G.train_step(ctx, X, Y, *ADAM)
    G.save(ctx, f)
    cfg, tensors = pkg.datasets.read_checkpoint(f)
    # near-ties between the two host layers' kernel choices: measured on the CPU oracle's logits for the file's weights
    ip, ix, dv = data["graph"]
    O = oracle.Gcn(oracle.Csr(ip, ix, dv.copy(), N), SIZES)
    for l, layer in enumerate(O.layers):
        layer.lin.W, layer.lin.b = tensors[f"W{l}"].copy(), tensors[f"b{l}"].copy()
    logits = O.forward(data["X"])
    top = np.sort(logits, axis=1)
    keep = (top[:, -1] - top[:, -2]) >= 1e-5 * np.abs(logits).max()
    assert (~keep).mean() <= 0.01, (~keep).sum()
    r = _cli(["-P", "1"], tmp_path, "predict", data["dir"], MGGCN_LOAD=f, MGGCN_PREDICTIONS=out)
    H = _model(pkg, data)
    H.load(ctx, f)
    want = H.predict(ctx, X)
    got = pkg.datasets.read_dense(out, "<i4")
    assert got.shape == want.shape == (N, 1) and want.dtype == np.int32
    np.testing.assert_array_equal(got[keep], want[keep])
    np.testing.assert_array_equal(want[keep][:, 0], np.argmax(logits, axis=1)[keep])
    line, = [ln for ln in r.stderr.splitlines() if ln.startswith("[mggcn predict]")]
    t = line.split()
    assert t[2::2] == ["all", "train", "val", "test"] and not _epochs(r.stderr)
    ev = H.evaluate(ctx, X, Y, S)
    for name in ("all", "train", "val", "test"):
        rows = N if name == "all" else int((data["S"] == ("train", "val", "test").index(name)).sum())
        assert abs(float(t[t.index(name) + 1]) - ev[name]) <= 3.0 / rows, (name, line, ev)
    assert abs(float(t[3]) - ev["all"]) <= 3.0 / N
    assert not os.path.exists(str(tmp_path / "csvs"))                   # predict times nothing
    # without MGGCN_PREDICTIONS the file is predictions.bin in the working directory
    _cli(["-P", "1"], tmp_path, "predict", data["dir"], MGGCN_LOAD=f)
    assert filecmp.cmp(out, str(tmp_path / "predictions.bin"), shallow=False)


def test_cli_predict_bce(pkg, ctx, data, tmp_path):
    f, out = str(tmp_path / "m.ckpt"), str(tmp_path / "pred.bin")
    X, Y, S = pkg.dn_matrix.from_numpy(data["X"]), pkg.dn_matrix.from_numpy(data["Yb"]), pkg.dn_matrix.from_numpy(data["S"])
    G = _model(pkg, data, loss="bce")
    for _ in range(3):
        G.train_step(ctx, X, Y, *ADAM)
    G.save(ctx, f)
    logits = G(ctx, X)
    ctx.sync()
    logits = logits.numpy()
    keep = np.abs(logits) >= 1e-5 * np.abs(logits).max()
    assert (~keep).mean() <= 0.01
    r = _cli(["-P", "1"], tmp_path, "predict", data["dir_bce"], MGGCN_LOAD=f, MGGCN_PREDICTIONS=out, MGGCN_LOSS="bce")
    got = pkg.datasets.read_dense(out, "<i4")
    assert got.shape == (N, C) and set(np.unique(got)) <= {0, 1}
    np.testing.assert_array_equal(got[keep], (logits > 0).astype(np.int32)[keep])
    np.testing.assert_array_equal(G.predict(ctx, X)[keep], got[keep])
    line, = [ln for ln in r.stderr.splitlines() if ln.startswith("[mggcn predict]")]
    t = line.split()
    ev = G.evaluate(ctx, X, Y, S)
    for name in ("all", "train", "val", "test"):
        assert abs(float(t[t.index(name) + 1]) - ev[name]) <= 1e-5, (name, line, ev)      # six printed digits of the same ratio
    # a softmax model does not take the multi-label file
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MGGCN_")}
    bad = subprocess.run([EXE, "-P", "1", "predict", data["dir_bce"], "2", "16", "16"], cwd=str(tmp_path),
                         env=dict(clean, MGGCN_LOAD=f), capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "[mggcn predict]" not in bad.stderr
