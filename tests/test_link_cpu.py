"""The link head without a GPU: every refusal of link_predictor and of the ops wrappers (None stands in for the context:
each raises before any device call), the exported symbols, and the sanity of the numpy restatement itself."""
import inspect
import types

import numpy as np
import pytest

import link_ref as ref


class fake:
    """quacks like a device tensor of the given shape at `ptr`: nothing is ever dereferenced"""

    def __init__(self, ptr, *shape, floating=False):
        self.ptr, self.shape = ptr, shape
        self.is_cuda, self.dtype = True, types.SimpleNamespace(is_floating_point=floating)

    def data_ptr(self): return self.ptr
    def numel(self): return int(np.prod(self.shape))
    def element_size(self): return 4
    def is_contiguous(self): return True
    def dim(self): return len(self.shape)
    def stride(self, i): return self.shape[1] if i == 0 else 1


def _model(pkg, n=10, d=8, cls=None):
    m = object.__new__(cls or pkg.gcn)
    m.A, m._out_width = types.SimpleNamespace(n=lambda: n), d
    return m


def _P(pkg, n=10, indptr0=0, nnz=3):
    ip = np.full(n + 1, indptr0 + nnz, dtype=np.uint32)
    ip[0] = indptr0
    return pkg.csr_matrix(ip, np.zeros(nnz, np.uint32), np.ones(nnz, np.float32), n)


@pytest.mark.parametrize("case,word", [("dist", "model"), ("wide", "model"), ("rect", "P"), ("rows", "P"), ("indptr0", "indptr"),
                                       ("empty", "P"), ("column", "column"), ("ratio0", "neg_ratio"), ("ratio_f", "neg_ratio"),
                                       ("huge", "neg_ratio"), ("pairs", "pairs")])
def test_link_predictor_refuses(pkg, case, word):
    model, P, kw = _model(pkg), _P(pkg), {}
    if case == "dist":
        model = _model(pkg, cls=pkg.dist_gcn)
    elif case == "wide":
        model = _model(pkg, d=1025)
    elif case == "rect":
        P = pkg.csr_matrix(P.indptr, P.indices, P.data, 11)
    elif case == "rows":
        P = _P(pkg, n=9)
    elif case == "indptr0":
        P = _P(pkg, indptr0=2)
    elif case == "empty":
        P = _P(pkg, nnz=0)
    elif case == "column":
        P.indices[1] = 10
    elif case in ("ratio0", "ratio_f", "huge"):
        kw = dict(neg_ratio={"ratio0": 0, "ratio_f": 1.0, "huge": (1 << 31) // 3 + 1}[case])
    with pytest.raises(ValueError, match=word):
        head = pkg.link_predictor(model, P, **kw)
        head.score(None, None, np.array([[0, 10]]))           # only the "pairs" case gets here


def test_ops_refuse_before_the_library(pkg):
    ops, u32 = pkg.ops, lambda ptr, k: fake(ptr, k)
    H, G = fake(1 << 20, 10, 8, floating=True), fake(2 << 20, 10, 8, floating=True)
    bad = [
        lambda: ops.link_neg_draw(None, 10, u32(64, 11), 3, 10, 0, 0, 0, u32(4096, 3), u32(8192, 3)),          # R == 0
        lambda: ops.link_neg_draw(None, 10, u32(64, 11), 1 << 30, 10, 2, 0, 0, u32(4096, 3), u32(8192, 3)),    # M R >= 2^31
        lambda: ops.link_neg_draw(None, 10, u32(64, 11), 3, 1 << 31, 1, 0, 0, u32(4096, 3), u32(8192, 3)),     # n >= 2^31
        lambda: ops.link_neg_draw(None, 10, u32(64, 11), 3, 10, 1, 0, 0, u32(4096, 3), u32(4100, 3)),          # overlap
        lambda: ops.link_bounds(None, u32(4096, 8), 8, 10, u32(4100, 11)),
        lambda: ops.link_dot_loss(None, 10, 10, u32(64, 11), u32(512, 3), 3, fake(1 << 20, 10, 1025, floating=True),
                                  fake(2 << 20, 10, 1025, floating=True), True, 1.0),                         # d > 1024
        lambda: ops.link_dot_loss(None, 10, 10, u32(64, 11), u32(512, 3), 3, H, fake((1 << 20) + 64, 10, 8, floating=True), True, 1.0),
        lambda: ops.link_dot_loss(None, 10, 10, u32(64, 11), u32(512, 3), 3, H, G, True, 1.0, row_loss=fake(4 << 20, 20, floating=True)),
        lambda: ops.link_dot_loss(None, 10, 10, u32(64, 11), u32(512, 3), 1 << 30, H, G, True, 1.0, neg_ratio=2),
        lambda: ops.edge_dot(None, u32(64, 5), u32(128, 5), 5, fake(1 << 20, 10, 0, floating=True), fake(4096, 5, floating=True)),
        lambda: ops.edge_dot(None, u32(64, 5), u32(128, 5), 5, H, fake(64, 5, floating=True)),                 # out on src
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {i} was not refused")


def test_exported_with_the_documented_signatures(pkg):
    assert "link_predictor" in pkg.__all__ and pkg.link_predictor is pkg.link.link_predictor
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(pkg.link_predictor.__init__) == ["self", "model", "P", "neg_ratio", "seed"]
    assert sig(pkg.link_predictor.train_step) == ["self", "ctx", "X", "lr", "beta1", "beta2", "weight_decay", "eps"]
    assert sig(pkg.link_predictor.set_negatives) == ["self", "ratio", "seed", "epoch"]
    assert sig(pkg.link_predictor.score) == ["self", "ctx", "X", "pairs"]
    assert sig(pkg.link_predictor.evaluate) == ["self", "ctx", "X", "pos_pairs", "neg_pairs"]
    for name in ("link_neg_draw_u32", "link_bounds_u32", "link_dot_loss_f32", "link_sums_f32", "edge_dot_f32"):
        assert hasattr(pkg._lib.load(), "mggcn_" + name)
    assert pkg.ops.LINK_DOMAIN == ref.LINK_DOMAIN == 0xE0000000


def test_the_reference_draws_uniform_tails_in_range():
    indptr = np.array([0, 50_000, 100_000], dtype=np.uint32)
    for n in (37, 1_000_003):
        tails, heads = ref.negatives(indptr, n, 1, seed=9, epoch=2)
        assert tails.shape == (100_000, 1) and tails.max() < n and heads.tolist() == [0] * 50_000 + [1] * 50_000
    u = tails.reshape(-1) / float(n)                  # uniform: standard deviation sqrt(1 / 12)
    assert abs(u.mean() - 0.5) <= 5 * np.sqrt(1 / 12 / u.size), u.mean()
    assert (ref.negatives(indptr, n, 1, 9, 3)[0] != tails).any()


def test_the_reference_gradient_is_the_derivative_of_its_loss():
    n, d, R = 80, 5, 2
    indptr, indices = ref.pattern(n, 4)
    H = np.random.default_rng(0).standard_normal((n, d))
    G = ref.loss_grad(indptr, indices, H.astype(np.float32), R, 3, 1)["G"]
    H = H.astype(np.float32).astype(np.float64)
    D, eps = np.random.default_rng(1).standard_normal((n, d)), 1e-6
    num = (ref.loss_only(indptr, indices, H + eps * D, R, 3, 1) - ref.loss_only(indptr, indices, H - eps * D, R, 3, 1)) / (2 * eps)
    assert abs(num - (G * D).sum()) <= 1e-6 * abs(num), (num, (G * D).sum())
