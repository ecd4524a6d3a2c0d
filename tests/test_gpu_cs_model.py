"""correct_and_smooth (mg-gcn_amd/smoothing.py) on the device against the fp64 restatement of cs_ref.py: the whole pipeline on
a 600-vertex power-law graph and its symmetric twin, the planted-partition case of test_cs_cpu.py, and predict() behind a
trained gcn and gat.

The bar on G's absolute error is eight times the fp32 twin's worst on the same input, computed here (cs_ref.model_case):
the device's SpMM adds in another order than the twin's.  Predictions must equal the reference's on every row whose top-two
margin in the reference exceeds twice the bar; test_cs_cpu.py checks that those are at least 99 % of the rows and that no
row's autoscale quotient sits on the switch at 1000, and the same conditions are asserted again here."""
import numpy as np
import pytest

import cs_ref as ref
from gat_ref import ADAM

pytestmark = pytest.mark.gpu

N = ref.MODEL_N


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _csr(pkg, graph):
    ip, ix, dv = graph
    return pkg.csr_matrix(ip.copy(), ix.copy(), dv.copy(), ip.shape[0] - 1)


def _device_pred(pkg, ctx, G):
    P = pkg.dn_matrix(G.n(), 1, dtype=np.int32)
    pkg.ops.max_row_indices(ctx, G, P)
    ctx.sync()
    return P.numpy().reshape(-1)


def _check_against(c, G, pred, what):
    """G within the bar of the reference, the predictions equal wherever the reference's margin decides them"""
    want = c["want"]
    err = float(np.abs(G.astype(np.float64) - want["G"]).max())
    twin = c["bar"] / 8.0
    decided = ref.decided_rows(want["G"], c["bar"])
    print(f"[cs] {what}: |G - fp64| {err:.3e} (twin {twin:.3e}, bar {c['bar']:.3e}); undecided rows {int((~decided).sum())}")
    assert (~decided).mean() <= 0.01, what
    assert err <= c["bar"], (what, err, c["bar"])
    np.testing.assert_array_equal(pred[decided], want["pred"][decided], err_msg=what)


@pytest.mark.parametrize("autoscale", [True, False])
@pytest.mark.parametrize("L1,L2", ref.MODEL_LAYERS)
@pytest.mark.parametrize("C", ref.MODEL_CLASSES)
@pytest.mark.parametrize("kind", ref.MODEL_KINDS)
def test_whole_pipeline(pkg, ctx, kind, C, L1, L2, autoscale):
    c = ref.model_case(pkg.datasets, kind, C, L1, L2, autoscale)
    if autoscale:
        assert ref.threshold_clear(c["want"]["quotient"]), "a row's quotient sits on the switch at 1000: choose another seed"
    cs = pkg.correct_and_smooth(_csr(pkg, c["graph"]), C, L1, 0.8, L2, 0.8, autoscale=autoscale, scale=0.9)
    logits = pkg.dn_matrix.from_numpy(c["logits"])
    Y, S = c["Y"], pkg.dn_matrix.from_numpy(c["S"].reshape(-1, 1))          # one as a host array, one on the device
    G = cs(ctx, logits, Y, S)
    pred = _device_pred(pkg, ctx, G)
    got = G.numpy().copy()
    what = f"{kind} C={C} L=({L1},{L2}) autoscale={autoscale}"
    _check_against(c, got, pred, what)
    np.testing.assert_array_equal(logits.numpy(), c["logits"])              # only read
    # the two halves on their own: Z within the same kind of bar, and smooth(correct()) is the same bits as the call
    Z = cs.correct(ctx, logits, Y, S)
    ctx.sync()
    z = Z.numpy().copy()
    zbar = 8.0 * float(np.abs(c["twin"]["Z"].astype(np.float64) - c["want"]["Z"]).max())
    zerr = float(np.abs(z.astype(np.float64) - c["want"]["Z"]).max())
    print(f"[cs] {what}: |Z - fp64| {zerr:.3e} (bar {zbar:.3e})")
    assert zerr <= zbar, (what, zerr, zbar)
    G2 = cs.smooth(ctx, Z, Y, S)
    ctx.sync()
    np.testing.assert_array_equal(_bits(G2.numpy()), _bits(got), err_msg=what)
    if L2 == 0:                                     # G = G0: Z with the labels written over the training rows
        train = c["S"] == 0
        np.testing.assert_array_equal(got[train], ref.onehot(c["Y"], C, np.float32)[train])
        np.testing.assert_array_equal(_bits(got[~train]), _bits(z[~train]))


def test_planted_partition(pkg, ctx):
    c = ref.planted_case()
    dn = pkg.datasets.sym_normalize(c["ip"], c["ix"], c["dv"])
    p = c["params"]
    args = ((c["ip"], c["ix"], dn), c["logits"], c["Y"], c["S"], 0, p["L1"], p["a1"], p["L2"], p["a2"], p["autoscale"], p["scale"])
    want, twin = ref.pipeline(*args), ref.pipeline(*args, dtype=np.float32)
    case = dict(want=want, bar=8.0 * float(np.abs(twin["G"] - want["G"]).max()))
    assert ref.threshold_clear(want["quotient"])
    cs = pkg.correct_and_smooth(_csr(pkg, (c["ip"], c["ix"], dn)), c["C"], p["L1"], p["a1"], p["L2"], p["a2"],
                                autoscale=p["autoscale"], scale=p["scale"])
    G = cs(ctx, pkg.dn_matrix.from_numpy(c["logits"]), c["Y"], c["S"])
    pred = _device_pred(pkg, ctx, G)
    _check_against(case, G.numpy(), pred, "planted partition")
    test = c["S"] == 2
    base, after = (c["logits"].argmax(axis=1) == c["Y"])[test].mean(), (pred == c["Y"])[test].mean()
    print(f"[cs] planted partition on the device: test accuracy {base:.4f} -> {after:.4f}")
    assert after >= base


# ---- behind a trained model ----------------------------------------------------------------------------------------------------------
F = 16


def _model_data(pkg, C):
    inp = ref.model_inputs(C)
    rng = np.random.default_rng(5)
    X = (ref.onehot(inp["Y"], C, np.float32) @ rng.standard_normal((C, F)).astype(np.float32)
         + 1.5 * rng.standard_normal((N, F)).astype(np.float32))
    return ref.model_graph(pkg.datasets, "sym"), X.astype(np.float32), inp["Y"].reshape(-1, 1), inp["S"]


def _make(pkg, which, graph, C):
    ip, ix, dv = graph
    A = pkg.csr_matrix(ip.copy(), ix.copy(), np.ones_like(dv), N)             # the models normalise their own copy
    return pkg.gcn(A, [F, 16, C]) if which == "gcn" else pkg.gat(A, [F, 16, C], heads=2)


def _weights(model):
    return [getattr(o, row[1]).numpy().copy() for layer in model.layers() for o in layer.params() for row in o.params_table]


@pytest.mark.parametrize("which", ["gcn", "gat"])
def test_predict_behind_a_trained_model(pkg, ctx, which):
    C = 7
    graph, X, Y, S = _model_data(pkg, C)
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    model = _make(pkg, which, graph, C)
    model.set_splits(S)
    for _ in range(5):
        model.train_step(ctx, Xd, Yd, *ADAM)
    cs = pkg.correct_and_smooth(_csr(pkg, graph), C, 20, 0.8, 20, 0.8)
    yp = cs.predict(ctx, model, Xd, Y, S)
    assert yp.dtype == np.int32 and yp.shape == (N, 1)
    logits = model(ctx, Xd)
    ctx.sync()
    logits = logits.numpy().copy()
    args = (graph, logits, Y, S, 0, 20, 0.8, 20, 0.8, True, 1.0)
    want, twin = ref.pipeline(*args), ref.pipeline(*args, dtype=np.float32)
    c = dict(want=want, bar=8.0 * float(np.abs(twin["G"] - want["G"]).max()))
    assert ref.threshold_clear(want["quotient"]), "a row's quotient sits on the switch at 1000"
    G = cs(ctx, pkg.dn_matrix.from_numpy(logits), Y, S)
    ctx.sync()
    _check_against(c, G.numpy(), yp.reshape(-1), f"predict behind {which}")
    again = cs.predict(ctx, model, Xd, Y, S)
    np.testing.assert_array_equal(yp, again)                                  # a second predict: the same bits
    test = S == 2
    print(f"[cs] {which}: test accuracy {(logits.argmax(axis=1) == Y.reshape(-1))[test].mean():.4f} -> "
          f"{(yp.reshape(-1) == Y.reshape(-1))[test].mean():.4f} after correct and smooth")


@pytest.mark.parametrize("which", ["gcn", "gat"])
def test_training_is_untouched_by_a_live_correct_and_smooth(pkg, ctx, which):
    """the models' own train_step gives the same bits with and without a correct_and_smooth object alive and running
    between the epochs (it shares the stream and its reduction scratch, nothing else)"""
    C = 7
    graph, X, Y, S = _model_data(pkg, C)
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    logits = pkg.dn_matrix.from_numpy(ref.model_inputs(C)["logits"])
    runs = []
    for with_cs in (False, True):
        model = _make(pkg, which, graph, C)
        model.set_splits(S)
        cs = pkg.correct_and_smooth(_csr(pkg, graph), C, 2, 0.8, 2, 0.8) if with_cs else None
        losses = []
        for _ in range(3):
            losses.append(model.train_step(ctx, Xd, Yd, *ADAM))
            if cs is not None:
                cs(ctx, logits, Y, S)
        runs.append((losses, _weights(model)))
    (la, wa), (lb, wb) = runs
    assert la == lb
    assert len(wa) == len(wb) and len(wa) >= 4
    for a, b in zip(wa, wb):
        np.testing.assert_array_equal(_bits(a), _bits(b))


def test_timers_are_registered(pkg, ctx):
    c = ref.model_case(pkg.datasets, "sym", 7, 3, 3, True)
    cs = pkg.correct_and_smooth(_csr(pkg, c["graph"]), 7, 3, 0.8, 3, 0.8)
    cs(ctx, pkg.dn_matrix.from_numpy(c["logits"]), c["Y"], c["S"])
    ctx.sync()
    for name in ("cs-residual", "cs-correct", "cs-scale", "cs-smooth", "cs-spmm", "cs-step"):
        assert name in ctx.timers and ctx.measure(name) >= 0.0, name
