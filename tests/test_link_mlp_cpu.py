"""The MLP link head without a GPU: every refusal of mlp_link_predictor (each raises before any device call), the exported
symbols, and the numpy restatement's gradients against a central difference of its own loss."""
import inspect

import numpy as np
import pytest

import link_mlp_ref as ref
import link_ref
from test_link_cpu import _model, _P


@pytest.mark.parametrize("case,word", [("d", "model"), ("d_odd", "model"), ("hidden0", "hidden"), ("hidden_odd", "hidden"),
                                       ("hidden_big", "hidden"), ("hidden_f", "hidden"), ("w_len", "weights"), ("w_shape", "W1"),
                                       ("w_b2", "b2"), ("w_nan", "non-finite"), ("ratio", "neg_ratio"), ("dist", "model")])
def test_mlp_link_predictor_refuses(pkg, case, word):
    d, good = 32, lambda hd: [np.zeros(s, np.float32) for s in ((32, hd), (1, hd), (1, hd), (1, 1))]
    model, kw = _model(pkg, d={"d": 8, "d_odd": 48}.get(case, d)), {}
    if case.startswith("hidden"):
        kw = dict(hidden={"hidden0": 0, "hidden_odd": 48, "hidden_big": 160, "hidden_f": 64.0}[case])
    elif case == "w_len":
        kw = dict(hidden=64, weights=good(64)[:3])
    elif case == "w_shape":
        kw = dict(hidden=64, weights=good(32))
    elif case == "w_b2":
        kw = dict(hidden=64, weights=good(64)[:3] + [np.zeros((1, 2), np.float32)])
    elif case == "w_nan":
        kw = dict(hidden=64, weights=good(64))
        kw["weights"][2][0, 5] = np.inf
    elif case == "ratio":
        kw = dict(neg_ratio=0)
    elif case == "dist":
        model = _model(pkg, d=d, cls=pkg.dist_gcn)
    with pytest.raises(ValueError, match=word):
        pkg.mlp_link_predictor(model, _P(pkg), **kw)


def test_exported_with_the_documented_signatures(pkg):
    assert "mlp_link_predictor" in pkg.__all__ and issubclass(pkg.mlp_link_predictor, pkg.link_predictor)
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(pkg.mlp_link_predictor.__init__) == ["self", "model", "P", "hidden", "neg_ratio", "seed", "weights"]
    assert sig(pkg.link_predictor.__init__) == ["self", "model", "P", "neg_ratio", "seed"]
    assert sig(pkg.mlp_link_predictor.train_step) == sig(pkg.link_predictor.train_step)
    for name in ("link_mlp_loss_f32", "link_mlp_pairs_f32", "link_mlp_partial_floats"):
        assert hasattr(pkg._lib.load(), "mggcn_" + name)
    assert pkg._lib.load().mggcn_link_mlp_partial_floats(96, 64) == pkg.ops.link_mlp_partial_floats(96, 64)
    with pytest.raises(ValueError, match="hd"):          # the ops refuse before the library: None stands in for the context
        from test_link_cpu import fake
        f = lambda *s: fake(1 << 20, *s, floating=True)
        pkg.ops.link_mlp_pairs(None, f(10, 32), (f(32, 48), f(48), f(48), f(1)), pairs=(fake(64, 5), fake(128, 5), 5), out=f(5))


def test_the_reference_gradients_are_the_derivative_of_its_loss():
    n, d, hd, R = 50, 32, 64, 2
    indptr, indices = link_ref.pattern(n, 4)
    H, params = ref.inputs(n, d, hd, 0)
    pairs = ref.pairs_of(indptr, indices, n, R, 3, 1)
    want = ref.loss_grad(H, params, *pairs)
    ref.check(want, ref.loss_grad(H, params, *pairs, dt=np.float32))
    rng, eps = np.random.default_rng(1), 1e-6
    point = [H.astype(np.float64)] + [p.astype(np.float64) for p in params]
    dirs = [rng.standard_normal(p.shape) for p in point]
    at = lambda sign: ref.loss_only(point[0] + sign * eps * dirs[0], [p + sign * eps * D for p, D in zip(point[1:], dirs[1:])], *pairs)
    num = (at(1) - at(-1)) / (2 * eps)
    ana = sum((want[k] * D).sum() for k, D in zip(("G",) + ref.NAMES, dirs))
    assert abs(num - ana) <= 1e-6 * abs(num), (num, ana)
