"""Correct and Smooth without a GPU: the host restatement (cs_ref.py) is pinned independently of the code -- a closed form
and the direction of the algorithm --, datasets.sym_normalize against dense numpy, every option check of
correct_and_smooth and of the three ops wrappers before any device work, and the conditions the GPU tests' inputs must
meet (the autoscale threshold is clear, the undecided rows are few) where they can be checked: here."""
import numpy as np
import pytest

import cs_ref as ref


class shape_only:
    def __init__(self, n, m): self.n_, self.m_ = n, m
    def n(self): return self.n_
    def m(self): return self.m_
    def shape(self): return (self.n_, self.m_)


def _small_graph(pkg, n=40, seed=5):
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    upper = np.triu(rng.random((n, n)) < 0.15, 1)
    adj = sp.csr_matrix((upper | upper.T).astype(np.float32) * (0.5 + rng.random((n, n)).astype(np.float32)))
    adj = ((adj + adj.T) * 0.5).tocsr()                     # symmetric values, not only a symmetric pattern
    adj.sort_indices()
    ip, ix = adj.indptr.astype(np.uint32), adj.indices.astype(np.uint32)
    return ip, ix, adj.data.astype(np.float32)


def _dense(ip, ix, dv, n):
    out = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(ip.astype(np.int64)))
    np.add.at(out, (rows, ix.astype(np.int64)), dv.astype(np.float64))
    return out


def test_unclamped_iteration_reaches_the_closed_form(pkg):
    """X <- a A X + (1 - a) E0 from X = E0 converges to (1 - a)(I - a A)^-1 E0 when the spectral radius of a A is below
    one: A = D^-1/2 W D^-1/2 of a symmetric W has eigenvalues in [-1, 1], a = 0.8, and after 300 iterations the distance
    is at most 0.8^300 ~ 8e-30 of the start -- the 1e-10 asked for is far above that and far above fp64 rounding"""
    n, a = 40, 0.8
    ip, ix, dv = _small_graph(pkg, n)
    dn = pkg.datasets.sym_normalize(ip, ix, dv)
    A = _dense(ip, ix, dn, n)
    assert np.abs(np.linalg.eigvalsh((A + A.T) / 2)).max() <= 1 + 1e-6 and np.abs(A - A.T).max() <= 1e-7
    E0 = np.random.default_rng(1).standard_normal((n, 3))
    got = ref.propagate(ip, ix, dn, E0, 300, a, 1 - a, -ref.INF, ref.INF)
    want = (1 - a) * np.linalg.solve(np.eye(n) - a * A, E0)
    assert np.abs(got - want).max() <= 1e-10


def test_correct_and_smooth_does_not_lose_accuracy_on_a_planted_partition(pkg):
    c = ref.planted_case()
    test = c["S"] == 2
    base = float((c["logits"].argmax(axis=1) == c["Y"])[test].mean())
    assert 0.5 <= base <= 0.8, base
    dn = pkg.datasets.sym_normalize(c["ip"], c["ix"], c["dv"])
    p = c["params"]
    out = ref.pipeline((c["ip"], c["ix"], dn), c["logits"], c["Y"], c["S"], 0, p["L1"], p["a1"], p["L2"], p["a2"],
                       p["autoscale"], p["scale"])
    after = float((out["pred"] == c["Y"])[test].mean())
    print(f"planted partition: test accuracy {base:.4f} -> {after:.4f}")
    assert after >= base, (base, after)
    assert (out["pred"] == c["Y"])[c["S"] == 0].all()       # the training rows carry their labels through the smoothing


def test_sym_normalize_against_dense_numpy(pkg):
    n = 9
    rng = np.random.default_rng(2)
    W = (rng.random((n, n)) < 0.4) * (0.25 + rng.random((n, n)))
    W[4, :] = 0.0                                           # a row without entries: degree zero
    W[:, 4] = np.where(np.arange(n) % 2 == 0, 0.5, 0.0)      # ... that other rows still point to
    W[4, 4] = 0.0
    import scipy.sparse as sp
    M = sp.csr_matrix(W.astype(np.float32))
    before = (M.indptr.copy(), M.indices.copy(), M.data.copy())
    got = pkg.datasets.sym_normalize(M.indptr, M.indices, M.data)
    assert got.dtype == np.float32 and got.shape == M.data.shape
    for a, b in zip(before, (M.indptr, M.indices, M.data)):
        np.testing.assert_array_equal(a, b)
    Wd = M.toarray().astype(np.float64)
    d = Wd.sum(axis=1)
    r = np.zeros(n)
    r[d > 0] = 1.0 / np.sqrt(d[d > 0])
    want = sp.csr_matrix((got, M.indices, M.indptr), shape=(n, n)).toarray()
    np.testing.assert_allclose(want, r[:, None] * Wd * r[None, :], rtol=1e-6, atol=0)
    assert d[4] == 0 and np.all(want[:, 4] == 0) and np.all(want[4] == 0)
    assert pkg.datasets.sym_normalize([0], [], []).shape == (0,)
    with pytest.raises(ValueError):
        pkg.datasets.sym_normalize([0, 1], [3], [1.0])      # not square


def _cs(pkg, n=6, C=3, **kw):
    A = pkg.csr_matrix(np.arange(n + 1), np.arange(n), np.ones(n, dtype=np.float32), n)
    args = dict(num_correction_layers=2, correction_alpha=0.8, num_smoothing_layers=2, smoothing_alpha=0.7)
    args.update(kw)
    return pkg.correct_and_smooth(A, C, **args)


def test_exported(pkg):
    assert "correct_and_smooth" in pkg.__all__ and pkg.correct_and_smooth is pkg.smoothing.correct_and_smooth
    cs = _cs(pkg, num_correction_layers=0, num_smoothing_layers=0)      # zero layers are valid
    assert (cs.num_correction_layers, cs.num_smoothing_layers, cs.autoscale, cs.scale) == (0, 0, True, 1.0)


@pytest.mark.parametrize("kw,name", [
    (dict(correction_alpha=0.0), "correction_alpha"), (dict(correction_alpha=1.5), "correction_alpha"),
    (dict(smoothing_alpha=-0.1), "smoothing_alpha"), (dict(smoothing_alpha=float("nan")), "smoothing_alpha"),
    (dict(num_correction_layers=-1), "num_correction_layers"), (dict(num_smoothing_layers=-3), "num_smoothing_layers"),
    (dict(num_smoothing_layers=2.5), "num_smoothing_layers"), (dict(scale=float("inf")), "scale")])
def test_constructor_refuses(pkg, kw, name):
    with pytest.raises(ValueError, match=name):
        _cs(pkg, **kw)


@pytest.mark.parametrize("C", [0, 1025, -4])
def test_constructor_refuses_class_counts(pkg, C):
    with pytest.raises(ValueError, match="n_classes"):
        _cs(pkg, C=C)


def test_constructor_refuses_a_matrix_that_is_not_square(pkg):
    A = pkg.csr_matrix([0, 1, 2], [0, 2], [1.0, 1.0], 3)
    with pytest.raises(ValueError, match="A must be square"):
        pkg.correct_and_smooth(A, 3, 1, 0.5, 1, 0.5)


def test_calls_refuse_before_any_device_work(pkg):
    """ctx = None: anything that touched the device would fail with AttributeError, not ValueError"""
    cs = _cs(pkg)
    Y, S = np.array([0, 1, 2, 0, 1, 2]), np.array([0, 0, 1, 2, 2, 7])
    for call in (cs.correct, cs.__call__, cs.smooth):
        with pytest.raises(ValueError, match="6 x 3"):
            call(None, shape_only(6, 4), Y, S)                          # a wrong shape
        with pytest.raises(ValueError, match="6 x 3"):
            call(None, shape_only(5, 3), Y, S)
        with pytest.raises(ValueError, match="Y: the label 3"):
            call(None, shape_only(6, 3), np.array([0, 3, 2, 0, 1, 2]), S)      # out of range on a training row
        with pytest.raises(ValueError, match="Y: the label -1"):
            call(None, shape_only(6, 3), np.array([-1, 1, 2, 0, 1, 2]), S)
        with pytest.raises(ValueError, match="no vertex belongs to set 0"):
            call(None, shape_only(6, 3), Y, np.array([1, 1, 1, 2, 2, 7]))
        with pytest.raises(ValueError, match="train_set"):
            call(None, shape_only(6, 3), Y, S, train_set=3)
        with pytest.raises(ValueError, match="Y must be 6 integers"):
            call(None, shape_only(6, 3), Y[:5], S)
        with pytest.raises(ValueError, match="S / train_set"):
            call(None, shape_only(6, 3), Y, S.astype(np.float32))
    # an out-of-range label on a row that does not train is never looked at: the call gets past the checks to the device
    with pytest.raises(AttributeError):
        cs.correct(None, shape_only(6, 3), np.array([0, 1, 99, 0, 1, 2]), S)


def test_predict_refuses_a_multi_label_model(pkg):
    class model:
        loss, _out_width = "bce", 3
    cs = _cs(pkg)
    with pytest.raises(ValueError, match="model.*bce"):
        cs.predict(None, model(), None, np.zeros(6, dtype=int), np.zeros(6, dtype=int))
    model.loss, model._out_width = "softmax", 4
    with pytest.raises(ValueError, match="model"):
        cs.predict(None, model(), None, np.zeros(6, dtype=int), np.zeros(6, dtype=int))


@pytest.mark.parametrize("m", [0, 1025])
def test_wrappers_refuse_bad_shapes_before_the_library(pkg, m):
    """the library's own precondition prints and exits the process: ops raises first, with shapes alone"""
    ops, a, b = pkg.ops, shape_only(3, m), shape_only(3, 8)
    with pytest.raises(ValueError):
        ops.cs_residual(None, a, shape_only(3, 1), shape_only(3, 1), 0, a, a, None)
    with pytest.raises(ValueError):
        ops.cs_step(None, a, a, None, 0.5, 0.5, 0.0, 1.0)
    with pytest.raises(ValueError):
        ops.cs_correct(None, a, a, None, None, 0, None, 1.0, 1.0, 0)
    with pytest.raises(ValueError):
        ops.cs_residual(None, b, shape_only(3, 1), shape_only(3, 1), 0, shape_only(4, 8), b, None)     # a shape mismatch
    with pytest.raises(ValueError):
        ops.cs_step(None, b, shape_only(3, 9), None, 0.5, 0.5, 0.0, 1.0)
    with pytest.raises(ValueError):
        ops.cs_correct(None, b, shape_only(2, 8), None, None, 0, None, 1.0, 1.0, 0)


def test_the_twin_rounds_where_the_kernels_round():
    """the fp32 twin of the step on operands of at most 12 significant bits equals the exact value rounded once"""
    rng = np.random.default_rng(3)
    q = lambda x: (np.round(np.ldexp(np.frexp(x)[0], 12)) * np.ldexp(1.0, np.frexp(x)[1] - 12)).astype(np.float32)
    T, R = q(rng.standard_normal((50, 7))), q(rng.standard_normal((50, 7)))
    al, be = float(q(np.array(0.8))), float(q(np.array(0.2)))
    got = ref.step(T, R, None, al, be, -ref.INF, ref.INF, dtype=np.float32)
    want = (al * T.astype(np.float64) + be * R.astype(np.float64)).astype(np.float32)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("kind", ref.MODEL_KINDS)
@pytest.mark.parametrize("C", ref.MODEL_CLASSES)
def test_inputs_of_the_gpu_model_tests_are_well_conditioned(pkg, kind, C):
    """what test_gpu_cs_model.py assumes about its inputs, checked where it can be: no row's autoscale quotient lies within
    a relative 1e-3 of the switch at 1000, and at most 1 % of the rows have a top-two margin within twice the bar"""
    for L1, L2 in ref.MODEL_LAYERS:
        for autoscale in (True, False):
            c = ref.model_case(pkg.datasets, kind, C, L1, L2, autoscale)
            assert c["bar"] > 0 and c["bar"] <= 1e-4, c["bar"]
            if autoscale:
                assert ref.threshold_clear(c["want"]["quotient"]), (kind, C, L1, L2)
            decided = ref.decided_rows(c["want"]["G"], c["bar"])
            assert (~decided).mean() <= 0.01, (kind, C, L1, L2, autoscale, float((~decided).mean()))
            np.testing.assert_array_equal(c["twin"]["pred"][decided], c["want"]["pred"][decided])


def test_planted_case_is_well_conditioned_for_the_gpu_test(pkg):
    c = ref.planted_case()
    dn = pkg.datasets.sym_normalize(c["ip"], c["ix"], c["dv"])
    p = c["params"]
    args = ((c["ip"], c["ix"], dn), c["logits"], c["Y"], c["S"], 0, p["L1"], p["a1"], p["L2"], p["a2"], p["autoscale"], p["scale"])
    want, twin = ref.pipeline(*args), ref.pipeline(*args, dtype=np.float32)
    bar = 8.0 * float(np.abs(twin["G"] - want["G"]).max())
    assert ref.threshold_clear(want["quotient"])
    assert (~ref.decided_rows(want["G"], bar)).mean() <= 0.01
