"""The link head on the device against tests/link_ref.py: (a) draw -> sort -> bounds as exact integers, (b) the loss kernel's
three launches and the sums against float64, (c) edge_dot, (d) link_predictor.train_step against the same step driven by hand,
(e) a gcn encoder learns a planted partition.  The float bar is the project's rule as gatdot_ref.bar_rule states it, on
gat_ref's row-scaled measure: gat_ref.ROW_TOL where the float32 twin's worst distance from the float64 restatement over the
cases below stays within ROW_TOL / 8, eight times the twin's worst otherwise."""
import functools

import numpy as np
import pytest

import link_ref as ref
from gat_ref import rowdist
from gatdot_ref import bar_rule

pytestmark = pytest.mark.gpu

SEED, EPOCH = 0x1234_5678_9ABC, 7
PATTERNS = {"n300": (300, 1, None), "n37": (37, 3, None), "n40": (40, 3, 3000)}        # (n, R, M): see link_ref.pattern
WIDTHS = (1, 7, 64, 128, 132, 1023, 1024)       # (1,1,4) x2, (4,1,4) x3, (1,16,1), (4,4,1); d = 128 misaligned is (1,4,2)
CASES = [(p, d, False) for p in PATTERNS for d in WIDTHS] + [(p, 128, True) for p in PATTERNS]


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _window(n, d, misaligned, values=None):
    """an [n x d] fp32 device window: contiguous, or with an odd leading dimension on a base 4 bytes off (NaN around it)"""
    import torch
    ld, off = (d + 3, 1) if misaligned else (d, 0)
    buf = torch.full((off + n * ld,), float("nan"), device="cuda")
    w = buf[off:].view(n, ld)[:, :d]
    if values is not None:
        w.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)))
    return w


@functools.lru_cache(maxsize=None)
def graph(name):
    n, R, M = PATTERNS[name]
    return (n, R) + ref.pattern(n, 11, M)


@functools.lru_cache(maxsize=None)
def case(name, d, with_G0=False):
    n, R, indptr, indices = graph(name)
    H = ref.embeddings(indptr, indices, n, d, R, SEED, EPOCH)
    G0 = np.random.default_rng(d).standard_normal((n, d)).astype(np.float32) if with_G0 else None
    want, twin = (ref.loss_grad(indptr, indices, H, R, SEED, EPOCH, G0, dt) for dt in (np.float64, np.float32))
    assert np.abs(want["scores"]).min() > 1e-3 and twin["hits"] == want["hits"]        # the count cannot hide behind a score at 0
    assert want["scores"].min() < -20 and want["scores"].max() > 20                    # both branches, a saturated sigma
    return dict(H=H, G0=G0, want=want, twin=twin)


def _sum_err(got, want):
    return max(abs(g - w) / w for g, w in zip(got, want["sums"]))


@functools.lru_cache(maxsize=None)
def bars():
    worst = dict(G=0.0, sums=0.0)
    for name, d, _ in CASES:
        c = case(name, d)
        worst["G"] = max(worst["G"], rowdist(c["twin"]["G"], c["want"]["G"], c["want"]["scale"]).max())
        worst["sums"] = max(worst["sums"], _sum_err(c["twin"]["sums"], c["want"]))
    out = {k: bar_rule(v) for k, v in worst.items()}
    print("[link] the twin's worst:", {k: f"{v:.3e}" for k, v in worst.items()}, "bars:", {k: f"{v:.3e}" for k, v in out.items()})
    assert all(v > 0 for v in out.values())
    return out


def _transpose_on_device(pkg, ctx, g, epoch, seed=SEED):
    """draw -> sort -> bounds through ops on the graph g = (n, R, indptr, indices); returns the host copies (keys and vals as
    drawn, sorted, nt_indptr) and the tensors"""
    import torch
    n, R, indptr, indices = g
    M = int(indptr[-1])
    keys, vals, ka, va = [torch.empty(M * R, dtype=torch.int32, device="cuda") for _ in range(4)]
    work = torch.empty(pkg.ops.radix_sort_work_bytes(1, M * R) // 8 + 1, dtype=torch.int64, device="cuda")
    nt, ip = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda"), _dev(indptr)
    ctx.sync()                                           # torch filled and uploaded on its own stream
    pkg.ops.link_neg_draw(ctx, n, ip, M, n, R, seed, epoch, keys, vals)
    ctx.sync()
    drawn = [t.cpu().numpy().view(np.uint32).copy() for t in (keys, vals)]
    pkg.ops.radix_sort_pairs(ctx, 1, M * R, keys, vals, ka, va, work, 0, max(1, (n - 1).bit_length()))
    pkg.ops.link_bounds(ctx, keys, M * R, n, nt)
    ctx.sync()
    return drawn + [t.cpu().numpy().view(np.uint32) for t in (keys, vals, nt)], (keys, vals, nt)


@pytest.mark.parametrize("name", PATTERNS)
def test_draw_sort_bounds(pkg, ctx, name):
    n, R, indptr, indices = graph(name)
    tails, heads = ref.negatives(indptr, n, R, SEED, EPOCH)
    (k0, v0, ks, vs, nt), _ = _transpose_on_device(pkg, ctx, graph(name), EPOCH)
    np.testing.assert_array_equal(k0, tails.reshape(-1))
    np.testing.assert_array_equal(v0, np.repeat(heads, R))
    for got, want in zip((ks, vs, nt), ref.negative_transpose(tails, heads, n)):
        np.testing.assert_array_equal(got, want)
    again, _ = _transpose_on_device(pkg, ctx, graph(name), EPOCH)
    other, _ = _transpose_on_device(pkg, ctx, graph(name), EPOCH + 1)
    assert all((a == b).all() for a, b in zip(again, (k0, v0, ks, vs, nt))) and (other[0] != k0).any()


def _host(M):
    return M.numpy() if hasattr(M, "buffer") else M.contiguous().cpu().numpy()


def _head_by_hand(pkg, ctx, g, seed, epoch, H, G, beta_first, rows):
    """the head through ops alone: draw, sort, bounds, the three launches in their order (P^T from numpy), the sums;
    returns G, the two loss sums and the correct count"""
    n, R, indptr, indices = g
    M = int(indptr[-1])
    t_ip, t_ix = ref.transpose_pattern(indptr, indices, n)
    _, (keys, vals, nt) = _transpose_on_device(pkg, ctx, g, epoch, seed)
    loss, (ip, ix, tip, tix) = pkg.ops.link_dot_loss, [_dev(a) for a in (indptr, indices, t_ip, t_ix)]
    ctx.sync()                                           # the uploads and fills of torch's stream are done
    loss(ctx, n, n, ip, ix, M, H, G, True, 1.0 / M, R, 1.0 / (M * R), seed, epoch, beta_first, *rows[:2])
    loss(ctx, n, n, tip, tix, M, H, G, True, 1.0 / M, beta=1.0)
    loss(ctx, n, n, nt, vals, M * R, H, G, False, 1.0 / (M * R), beta=1.0)
    pkg.ops.link_sums(ctx, rows[0], rows[1], n, rows[2])
    ctx.sync()
    words = rows[2].cpu().numpy()
    return _host(G), (float(words[0]), float(words[1])), int(words.view(np.uint32)[2])


def _rows(n):
    import torch
    return (torch.empty(2 * n, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(3, device="cuda"))


def _three_launches(pkg, ctx, name, H, G, beta_first, rows):
    return _head_by_hand(pkg, ctx, graph(name), SEED, EPOCH, H, G, beta_first, rows)


@pytest.mark.parametrize("name,d,misaligned", CASES)
def test_dot_loss_and_sums(pkg, ctx, name, d, misaligned):
    n, c, bar = graph(name)[0], case(name, d), bars()
    H = _window(n, d, misaligned, c["H"])
    runs = []
    for _ in range(2):                                   # beta = 0 never reads G: it starts as NaN
        rows = _rows(n)
        runs.append(_three_launches(pkg, ctx, name, H, _window(n, d, misaligned), 0.0, rows))
    (G, sums, hits), (G2, sums2, hits2) = runs
    assert G.view(np.uint32).tolist() == G2.view(np.uint32).tolist() and (sums, hits) == (sums2, hits2)    # the same bits
    dG, ds = rowdist(G, c["want"]["G"], c["want"]["scale"]).max(), _sum_err(sums, c["want"])
    print(f"[link] {name} d={d} misaligned={misaligned}: G {dG / bar['G']:.3f} of its bar, sums {ds / bar['sums']:.3f}")
    assert hits == c["want"]["hits"]
    assert dG <= bar["G"] and ds <= bar["sums"], (dG, ds, bar)
    if d == 128:                                         # beta = 1 onto a non-zero G
        c1 = case(name, d, True)
        G1 = _three_launches(pkg, ctx, name, H, _window(n, d, misaligned, c1["G0"]), 1.0, rows)[0]
        assert rowdist(G1, c1["want"]["G"], c1["want"]["scale"]).max() <= bar["G"]


@pytest.mark.parametrize("m", (1, 63, 4097))
@pytest.mark.parametrize("d,misaligned", [(64, False), (7, False), (64, True)])
def test_edge_dot(pkg, ctx, m, d, misaligned):
    import torch
    rng = np.random.default_rng(m + d)
    H = rng.standard_normal((50, d)).astype(np.float32)
    src, dst = (rng.integers(0, 50, size=m).astype(np.uint32) for _ in range(2))
    A, B = H[src].astype(np.float64), H[dst].astype(np.float64)
    want, scale = (A * B).sum(axis=1), np.abs(A * B).sum(axis=1)
    twin = (H[src] * H[dst]).cumsum(axis=1)[:, -1]
    bar = bar_rule(rowdist(twin, want[:, None], scale[:, None]).max())
    out = torch.full((m + 1,), 7.0, device="cuda")
    operands = (_dev(src), _dev(dst), m, _window(50, d, misaligned, H), out)
    ctx.sync()
    pkg.ops.edge_dot(ctx, *operands)
    ctx.sync()
    got = out.cpu().numpy()
    assert got[m] == 7.0
    assert rowdist(got[:m], want[:, None], scale[:, None]).max() <= bar


def _params(model):
    return [t.numpy().view(np.uint32) for layer in model.layers() for p in layer.params() for t in (p.W, p.b)]


@pytest.mark.parametrize("kind", ("gcn", "sage"))
def test_train_step_is_the_public_pieces(pkg, ctx, kind):
    n, sizes, adam = 200, [6, 8, 4], (1e-2, 0.9, 0.999, 5e-4, 1e-8)
    ip, ix, dv = pkg.datasets.synth_uniform_csr(n, 5, seed=2)
    X = pkg.dn_matrix.from_numpy(np.random.default_rng(3).standard_normal((n, sizes[0])).astype(np.float32))
    make = lambda w: (pkg.gcn if kind == "gcn" else pkg.sage)(pkg.csr_matrix(ip.copy(), ix.copy(), dv.copy(), n), sizes, weights=w)
    first = make(None)
    lins = [[p for p in layer.params()] for layer in first.layers()]
    weights = [tuple(a.numpy() for p in ps for a in (p.W, p.b)) for ps in lins]
    models = [make(weights), make(weights)]
    head = pkg.link_predictor(models[0], pkg.csr_matrix(ip.copy(), ix.copy(), dv.copy(), n), neg_ratio=2, seed=SEED)
    g, M, R, G, rows = (n, 2, ip, ix), int(ip[-1]), 2, pkg.dn_matrix(n, sizes[-1]), _rows(n)
    for step in range(3):
        loss, acc = head.train_step(ctx, X, *adam)
        H = models[1](ctx, X, training=True)             # the second model: nothing of link.py from here on
        ctx.sync()
        want = ref.loss_grad(ip, ix, H.numpy(), R, SEED, step)
        got_G, sums, hits = _head_by_hand(pkg, ctx, g, SEED, step, H, G, 0.0, rows)
        assert rowdist(got_G, want["G"], want["scale"]).max() <= bars()["G"], step
        assert (sums[0] / M + sums[1] / (M * R), hits / (M * (1 + R))) == (loss, acc)
        assert abs(loss - want["loss"]) <= bars()["sums"] * want["loss"] and hits == want["hits"], (step, loss, want["loss"])
        back = G
        for layer in reversed(models[1].layers()):
            back = layer.backward(ctx, back)
        models[1].adam_update(ctx, *adam)
        ctx.sync()
        assert all((a == b).all() for a, b in zip(_params(models[0]), _params(models[1]))), step
    assert head.epoch == 3 and {"link-draw", "link-sort", "link-bounds", "link-loss"} <= set(ctx.timers)


def test_a_gcn_encoder_learns_a_planted_partition(pkg, ctx):
    """cs_ref's planted partition of 1000 vertices, 500 edges held out, 500 uniform non-edges, random features, 60 steps of
    link_predictor(gcn(A, [16, 32, 16]), P_train) with A = P_train, at the learning rate of the other model tests.  The bars:
    five standard errors over a chance-level AUC, 0.5 + 5 sqrt((P + N + 1) / (12 P N)) = 0.5913 at P = N = 500, and the AUC of the
    raw scores X X^T in float64.
    One thing is not cs_ref's default: C = 40 communities of 25 instead of 5 of 200 (the same expected 8 neighbours inside and 3
    outside).  Random features carry no community, so what tells a held-out edge from a non-edge is that its endpoints'
    two-hop neighbourhoods share vertices; in a community of 200 they share too few for 16 dimensions and 60 steps (DESIGN.md
    3.15 has the figures)."""
    import cs_ref
    g = cs_ref.planted_case(n=1000, C=40)
    n, rng = g["n"], np.random.default_rng(5)
    rows = np.repeat(np.arange(n), np.diff(g["ip"].astype(np.int64)))
    upper = np.flatnonzero(rows < g["ix"])
    held = rng.choice(upper, size=500, replace=False)
    pos = np.stack([rows[held], g["ix"][held]], axis=1).astype(np.int64)
    dense = np.zeros((n, n), dtype=bool)
    dense[rows, g["ix"]] = True
    cand = rng.integers(0, n, size=(4000, 2))
    neg = cand[(~dense[cand[:, 0], cand[:, 1]]) & (cand[:, 0] != cand[:, 1])][:500]
    dense[pos[:, 0], pos[:, 1]] = dense[pos[:, 1], pos[:, 0]] = False                   # train on what is left, both directions
    import scipy.sparse as sp
    train = sp.csr_matrix(dense.astype(np.float32))
    csr = lambda: pkg.csr_matrix(train.indptr.astype(np.uint32), train.indices.astype(np.uint32), train.data.copy(), n)
    Xh = rng.standard_normal((n, 16)).astype(np.float32)
    head = pkg.link_predictor(pkg.gcn(csr(), [16, 32, 16]), csr())
    X = pkg.dn_matrix.from_numpy(Xh)
    losses = [head.train_step(ctx, X, 1e-2, 0.9, 0.999, 0.0, 1e-8)[0] for _ in range(60)]
    res = head.evaluate(ctx, X, pos, neg)
    import auc_ref
    raw = (Xh.astype(np.float64)[np.r_[pos[:, 0], neg[:, 0]]] * Xh.astype(np.float64)[np.r_[pos[:, 1], neg[:, 1]]]).sum(axis=1)
    y = np.r_[np.ones(500, np.int32), np.zeros(500, np.int32)]
    raw_auc = auc_ref.auc_of(*auc_ref.stats(raw.astype(np.float32).reshape(-1, 1), y.reshape(-1, 1))[0][4])
    chance = 0.5 + 5 * np.sqrt((500 + 500 + 1) / (12 * 500 * 500))
    print(f"[link] loss {losses[0]:.4f} -> {losses[-1]:.4f}, auc {res['auc']:.4f} (raw X X^T {raw_auc:.4f}, bar {chance:.4f})")
    assert len(neg) == 500 and losses[-1] < losses[0]
    assert res["auc"] > chance and res["auc"] > raw_auc
