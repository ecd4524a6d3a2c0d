"""The ranking kernels of the link head on the device (csrc/link_rank.hip): every count is an exact integer, so every check is
integer equality -- the dot kernel against float64 on embeddings whose products are exact, the MLP kernels against counts taken
from the pair kernels' own scores (held to float64 in test_gpu_link_mlp*.py), the sorted kernel against numpy, and
link_predictor.rank against counts taken from score() of the same pairs."""
import numpy as np
import pytest

import link_mlp_ref
import link_rank_ref as ref
from test_gpu_link import _dev, _window
from test_gpu_link_mlp_bf16 import _images

pytestmark = pytest.mark.gpu

N, M = 50, 9                                             # nine positives: three workgroups, the last with one live wave


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


def _lists(K, seed, twins=None):
    """src, dst [M] and tails [M x K] below N with tails[:, 0] the positive's own tail: a planted tie in every row; with
    ``twins`` = (a, b), two vertices whose rows of H are identical, tail b wherever a is the positive's tail"""
    rng = np.random.default_rng(seed)
    src, dst, tails = rng.integers(0, N, M), rng.integers(0, N, M), rng.integers(0, N, (M, K))
    tails[:, 0] = dst
    if twins is not None and K > 1:
        dst[:3] = twins[0]
        tails[:3, 0], tails[:3, K - 1] = twins[0], twins[1]
        tails[:3, 1:K - 1] = rng.integers(10, 30, (3, max(K - 2, 0)))       # the near twins of test_rank_mlp_*: scores an ulp apart
    return tuple(a.astype(np.uint32) for a in (src, dst, tails))


def _counts(pkg, ctx, op, lists, *operands):
    import torch
    src, dst, tails = lists
    out = torch.full((2 * M + 2,), -1, dtype=torch.int32, device="cuda")
    ctx.sync()
    op(ctx, _dev(src), _dev(dst), M, _dev(tails.reshape(-1)), tails.shape[1], *operands, out)
    ctx.sync()
    got = out.cpu().numpy()
    assert got[2 * M:].tolist() == [-1, -1]              # nothing beyond the last positive
    return got[:2 * M].reshape(M, 2).astype(np.int64)


@pytest.mark.parametrize("K", (1, 33, 70, 257))          # 70: one chunk of 64 and 6 more
@pytest.mark.parametrize("d,misaligned", [(4, False), (41, False), (128, False), (1024, False), (128, True)])
def test_rank_dot_counts_exactly(pkg, ctx, d, K, misaligned):
    src, dst, tails = lists = _lists(K, d + K)
    H = np.random.default_rng(d).integers(-2, 3, size=(N, d)).astype(np.float32)       # every dot product exact in fp32
    got = _counts(pkg, ctx, pkg.ops.link_rank_dot, lists, _window(N, d, misaligned, H))
    H64 = H.astype(np.float64)
    g, e = ref.counts((H64[src] * H64[dst]).sum(1), np.einsum("ic,ikc->ik", H64[src], H64[tails]))
    assert (e >= 1).all()
    assert (got[:, 0].tolist(), got[:, 1].tolist()) == (g.tolist(), e.tolist())


@pytest.mark.parametrize("K", (1, 31, 32, 33, 70))
@pytest.mark.parametrize("d,hd", [(32, 32), (96, 64), (128, 128)])
@pytest.mark.parametrize("dtype", ("f32", "bf16"))
def test_rank_mlp_counts_what_the_pair_kernel_scores(pkg, ctx, dtype, d, hd, K):
    import torch
    lists = src, dst, tails = _lists(K, d + hd + K, twins=(3, 7))
    H = np.random.default_rng(d + hd).standard_normal((N, d)).astype(np.float32)
    H[7] = H[3]
    H[10:30] = H[3] * (1 + np.arange(-10, 10, dtype=np.float32)[:, None] * 2.0 ** -23)   # a few ulps off: the last bit of a score decides
    params = tuple(_dev(p) for p in link_mlp_ref.inputs(N, d, hd, 5)[1])
    Hd = _window(N, d, False, H)
    if dtype == "bf16":
        Hd, image = _images(pkg, ctx, Hd, params[0])
        params = (image,) + params[1:]
    pairs_op, rank_op = ((pkg.ops.link_mlp_pairs, pkg.ops.link_rank_mlp) if dtype == "f32" else
                         (pkg.ops.link_mlp_pairs_bf16, pkg.ops.link_rank_mlp_bf16))
    u = np.repeat(src, 1 + K)                            # the same M (1 + K) pairs, flat: the positive, then its negatives
    v = np.concatenate([dst[:, None], tails], axis=1).reshape(-1)
    out = torch.empty(u.size, device="cuda")
    ctx.sync()
    pairs_op(ctx, Hd, params, pairs=(_dev(u), _dev(v), u.size), out=out)
    ctx.sync()
    s = out.cpu().numpy().reshape(M, 1 + K)
    g, e = ref.counts(s[:, 0], s[:, 1:])
    assert (e >= 1).all() and (K == 1 or (e[:3] >= 2).all())
    got = _counts(pkg, ctx, rank_op, lists, Hd, params)
    assert (got[:, 0].tolist(), got[:, 1].tolist()) == (g.tolist(), e.tolist())


@pytest.mark.parametrize("m", (1, 70))
@pytest.mark.parametrize("m_neg", (1, 5, 300, 5000))     # 5000: past one sort tile
def test_rank_sorted_counts_exactly(pkg, ctx, m, m_neg):
    import torch
    values = np.array([0.0, -0.0, -1.5, -1.5, 2.0, 1e-30, -3.0, 7.25], dtype=np.float32)
    rng = np.random.default_rng(m + m_neg)
    s_pos, s_neg = values[rng.integers(0, values.size, m)], values[rng.integers(0, values.size, m_neg)]
    keys, vals, ka, va = (torch.empty(m_neg, dtype=torch.int32, device="cuda") for _ in range(4))
    work = torch.empty(pkg.ops.radix_sort_work_bytes(1, m_neg) // 8 + 1, dtype=torch.int64, device="cuda")
    out = torch.full((2 * m,), -1, dtype=torch.int32, device="cuda")
    neg, zeros = _dev(s_neg.reshape(-1, 1)), torch.zeros((m_neg, 1), dtype=torch.int32, device="cuda")
    ctx.sync()
    pkg.ops.roc_auc_keys(ctx, neg, zeros, None, 0, 1, keys, vals)
    pkg.ops.radix_sort_pairs(ctx, 1, m_neg, keys, vals, ka, va, work)
    pkg.ops.link_rank_sorted(ctx, _dev(s_pos), m, keys, m_neg, out)
    ctx.sync()
    g, e = ref.counts(s_pos, s_neg)
    got = out.cpu().numpy().reshape(m, 2)
    assert (got[:, 0].tolist(), got[:, 1].tolist()) == (g.tolist(), e.tolist())


@pytest.mark.parametrize("mode", ("tails", "shared"))
@pytest.mark.parametrize("head", ("dot", "mlp", "bf16"))
def test_rank_is_what_one_counts_from_score(pkg, ctx, head, mode):
    n, sizes, ks = 70, [6, 8, 32], (1, 3, 10, 50)
    ip, ix, dv = pkg.datasets.synth_uniform_csr(n, 5, seed=2)
    X = pkg.dn_matrix.from_numpy(np.random.default_rng(3).standard_normal((n, sizes[0])).astype(np.float32))
    csr = lambda: pkg.csr_matrix(ip.copy(), ix.copy(), dv.copy(), n)
    model = pkg.gcn(csr(), sizes, dropout=0.5)
    h = (pkg.link_predictor(model, csr()) if head == "dot" else
         pkg.mlp_link_predictor(model, csr(), hidden=64, decoder_dtype="f32" if head == "mlp" else "bf16"))
    rng = np.random.default_rng(4)
    pos, tails, neg = rng.integers(0, n, (M, 2)), rng.integers(0, n, (M, 40)), rng.integers(0, n, (45, 2))
    tails[:, 0], neg[0] = pos[:, 1], pos[0]              # a tie in every row; the first positive is in the shared list
    h.rank(ctx, X, pos, neg_pairs=neg)                   # a first call: the bf16 head's images exist from here on
    before = (h.epoch, model.dropout_epoch)
    kw = dict(neg_tails=tails) if mode == "tails" else dict(neg_pairs=neg)
    a, b = (h.rank(ctx, X, pos, ks=ks, **kw) for _ in range(2))
    assert before == (h.epoch, model.dropout_epoch) and "link-rank" in ctx.timers
    assert all(a[k].dtype == np.uint32 and a[k].tolist() == b[k].tolist() for k in ("greater", "equal"))
    assert (a["mrr"], a["hits"]) == (b["mrr"], b["hits"])
    s_pos = h.score(ctx, X, pos).numpy().reshape(-1)
    if mode == "tails":
        flat = np.stack([np.repeat(pos[:, 0], 40), tails.reshape(-1)], axis=1)
        g, e = ref.counts(s_pos, h.score(ctx, X, flat).numpy().reshape(M, 40))
    else:
        g, e = ref.counts(s_pos, h.score(ctx, X, neg).numpy().reshape(-1))
    assert (e >= 1).all() if mode == "tails" else e[0] >= 1
    assert (a["greater"].tolist(), a["equal"].tolist()) == (g.tolist(), e.tolist())
    assert (a["mrr"], a["hits"]) == ref.metrics(g, e, ks, mode == "shared")
