"""The exact fan-out without a device: the refusals, the restated sample's properties, exact_inverse_factors by hand."""
from importlib import import_module

import numpy as np
import pytest

import edge_sample_ref as ref
import edge_select_ref as sel
from gat_ref import transpose_pattern

def _tiny(pkg, n=8):
    return pkg.csr_matrix(np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32), np.ones(n, dtype=np.float32), n)


MODELS = [("gat", dict(heads=2)), ("sage", dict(aggr="max")), ("sage", dict(aggr="mean", edge_rescale="row")),
          ("gcn", dict(edge_rescale="inverse"))]


@pytest.mark.parametrize("cls,kw", MODELS, ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v.values())))
def test_refusals_name_the_argument_and_store_nothing(pkg, cls, kw):
    A, model, inverse = _tiny(pkg), getattr(pkg, cls), kw.get("edge_rescale") == "inverse"
    G = model.__new__(model)                                        # a model object without a device
    G._sample_matrices = (A, A)
    for k, v in kw.items():
        setattr(G, k, v)
    bad = [dict(fanout=4, exact=1), dict(fanout=4, exact="yes"), dict(exact=True), dict(keep=0.5, exact=True),
           *([dict(fanout=4, keep=0.5, exact=True)] if inverse else [])]       # no closed-form factor for DropEdge-then-k
    for b in bad:
        ctor = {dict(keep="edge_keep", exact="fanout_exact").get(k, k): v for k, v in b.items()}
        with pytest.raises(TypeError if cls == "gat" else ValueError, match="exact"):
            model(A, [4, 8, 3], **kw, **ctor)                        # gat's constructor does not take the switch
        with pytest.raises(ValueError, match="exact"):
            G.set_sampling(seed=5, epoch=2, **b)
        assert (G.sample_fanout, G.sample_keep, G.sample_exact, G.sample_epoch, G.sampler) == (None, 1.0, False, 0, None)
    G.set_sampling(fanout=4, keep=1.0 if inverse else 0.5, seed=5, epoch=3, exact=True)
    assert G.sample_exact and G.sampler.exact and G.sampler.thr_host is None and (G.sampler.inv_host is not None) == inverse
    G.set_sampling(fanout=6)                                        # None keeps the model's setting
    assert G.sample_exact and G.sampler.exact and G.sample_fanout == 6
    G.set_sampling()                                                # off is not refused; the setting rests
    assert G.sampler is None and G.sample_exact
    G.set_sampling(fanout=6, exact=False)
    assert not G.sampler.exact and G.sampler.thr_host.dtype == np.uint32
    with pytest.raises(ValueError, match="exact"):
        pkg.edge_sampler(A, A, None, 0.5, exact=True)


def test_the_restated_sample_is_an_exact_fan_out_and_transposes(pkg):
    K = 10
    ip, ix = sel.graph(K, pkg.ops.EDGE_SELECT_REG_ENTRIES)
    thr = sel.select(ip, ix, K, 1.0, seed=sel.SEED, epoch=sel.EPOCH)
    dst, src, rows = ref.pairs(ip, ix, 0)
    kept = ref.keep_mask(ip, ix, thr, seed=sel.SEED, epoch=sel.EPOCH)
    others = np.bincount(rows[kept & (dst != src)].astype(np.int64), minlength=sel.N_ROWS)
    m = np.bincount(rows[dst != src].astype(np.int64), minlength=sel.N_ROWS)
    assert (others <= K).all() and (kept | (dst != src)).all()      # at most k others, every self entry
    simple = np.array([np.unique(ix[ip[r]:ip[r + 1]]).size == ip[r + 1] - ip[r] for r in range(sel.N_ROWS)])
    assert simple.sum() > 150 and (~simple).sum() > 50
    np.testing.assert_array_equal(others[simple], np.minimum(K, m)[simple])     # also: this seed has no 32-bit tie
    assert others[sel.STRADDLE] == K - 1 and m[sel.STRADDLE] > K     # the duplicate at the boundary: fewer, never more
    half = sel.select(ip, ix, K, 0.5, seed=sel.SEED, epoch=sel.EPOCH)
    assert (half <= thr).all() and (half <= sel.t_keep(0.5)).all() and (half < thr).any()
    # F's and F^T's samples are transposes of each other, entry for entry
    sample = lambda p, x, t: ref.sample(p, x, thr, t, seed=sel.SEED, epoch=sel.EPOCH)[1:]
    for got, want in zip(sample(*transpose_pattern(ip, ix, sel.N_COLS), 1), transpose_pattern(*sample(ip, ix, 0), sel.N_COLS)):
        np.testing.assert_array_equal(got, want)


def test_exact_inverse_factors(pkg):
    es = import_module(pkg.__name__ + ".edge_sample")
    # row 0: itself and 5 others; row 1: 2 others, one of them twice (m = 3); row 2: only itself; row 3: empty
    ip = np.array([0, 6, 9, 10, 10], dtype=np.uint32)
    ix = np.array([3, 0, 1, 2, 3, 1, 0, 0, 2, 2], dtype=np.uint32)
    for k, want in ((2, [2.5, 1.5, 1.0, 1.0]), (3, [5.0 / 3.0, 1.0, 1.0, 1.0]), (10 ** 6, [1.0] * 4)):
        got = es.exact_inverse_factors(ip, ix, k)
        np.testing.assert_array_equal(got, np.array(want, dtype=np.float64).astype(np.float32))
        np.testing.assert_array_equal(got, sel.exact_inverse_factors(ip, ix, k))
