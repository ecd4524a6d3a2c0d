"""link_predictor.rank without a GPU: the tie rule by hand, every refusal (None stands in for the context: each raises before
any device call), and the new entries in the library, PROTOTYPES and ops."""
import numpy as np
import pytest

import link_rank_ref as ref
from test_link_cpu import _P, _model

ENTRIES = ("mggcn_link_rank_dot_f32", "mggcn_link_rank_mlp_f32", "mggcn_link_rank_mlp_bf16", "mggcn_link_rank_sorted_u32")


@pytest.mark.parametrize("metrics", ["ref", "package"])
def test_the_tie_rule_by_hand(pkg, metrics):
    f = ref.metrics if metrics == "ref" else pkg.link.rank_metrics
    for s_neg in ([[2.0, 1.0, 1.0, 0.0]], [2.0, 1.0, 1.0, 0.0]):         # own negatives, then the same list shared
        g, e = ref.counts([1.0], np.array(s_neg, dtype=np.float32))
        assert (g.tolist(), e.tolist()) == ([1], [2])
    mrr, hits = f(g, e, (2, 3, 4), False)                                # rank 1 + 1 + 2 / 2 = 3
    assert mrr == 1.0 / 3.0 and hits == {2: 0.0, 3: 1.0, 4: 1.0}
    mrr, hits = f(g, e, (3, 4, 5), True)                                 # greater + equal = 3: not above the 3rd largest
    assert mrr == 1.0 / 3.0 and hits == {3: 0.0, 4: 1.0, 5: 1.0}        # k = 5 > m_neg = 4: 1.0 by itself
    assert ref.counts([-0.0], np.array([0.0, -0.0], dtype=np.float32))[1].tolist() == [2]


@pytest.mark.parametrize("word,kw", [
    ("neg_pairs and neg_tails", dict()),
    ("neg_pairs and neg_tails", dict(neg_pairs=[[0, 1]], neg_tails=[[1], [2]])),
    ("pos_pairs", dict(pos_pairs=[0, 1], neg_pairs=[[0, 1]])),                                      # shape
    ("pos_pairs", dict(pos_pairs=[[0.0, 1.0]], neg_pairs=[[0, 1]])),                                # dtype
    ("pos_pairs", dict(pos_pairs=[[0, 10]], neg_pairs=[[0, 1]])),                                   # vertex
    ("pos_pairs", dict(pos_pairs=np.zeros((0, 2), np.int64), neg_pairs=[[0, 1]])),                  # m == 0
    ("neg_pairs", dict(neg_pairs=[[0, 1, 2]])),
    ("neg_pairs", dict(neg_pairs=[[0, -1]])),
    ("neg_pairs", dict(neg_pairs=np.broadcast_to(np.zeros((1, 2), np.int32), ((1 << 31) - 2, 2)))),  # m + m_neg >= 2^31
    ("neg_tails", dict(neg_tails=[[1, 2, 3]])),                                                     # one row for two positives
    ("neg_tails", dict(neg_tails=[[1.0], [2.0]])),
    ("neg_tails", dict(neg_tails=[[1], [10]])),
    ("neg_tails", dict(neg_tails=np.broadcast_to(np.zeros((1, 1), np.int32), (2, 1 << 30)))),       # m K >= 2^31
    ("ks", dict(neg_tails=[[1], [2]], ks=5)),
    ("ks", dict(neg_tails=[[1], [2]], ks=(1, 0))),
    ("ks", dict(neg_tails=[[1], [2]], ks=(1, 2.0))),
])
@pytest.mark.parametrize("head", ["dot", "mlp"])
def test_rank_refuses_before_any_device_work(pkg, head, word, kw):
    if head == "dot":
        h = pkg.link_predictor(_model(pkg), _P(pkg))
    else:
        h = object.__new__(pkg.mlp_link_predictor)                      # its constructor allocates; rank checks first
        h.n = 10
    kw = {"pos_pairs": [[0, 1], [2, 3]], **kw}
    with pytest.raises(ValueError, match=word):
        h.rank(None, None, **kw)


def test_the_entries_are_declared_loaded_and_wrapped(pkg):
    lib = pkg._lib.load()
    assert all(name in pkg._lib.PROTOTYPES and hasattr(lib, name) for name in ENTRIES)
    assert all(callable(getattr(pkg.ops, name)) for name in ("link_rank_dot", "link_rank_mlp", "link_rank_mlp_bf16", "link_rank_sorted"))
    assert pkg.mlp_link_predictor.rank is pkg.link_predictor.rank
