"""The MLP link decoder on the device against tests/link_mlp_ref.py: (a) the three link_mlp_loss launches, the sums and the
link_mlp_pairs gradients of a step against float64, (b) link_mlp_pairs on explicit lists, (c) mlp_link_predictor.train_step
against the same step driven by hand.  The float bars are gatdot_ref.bar_rule of the float32 twin's worst distance from float64
over the cases below: gat_ref's row-scaled measure for G, the relative error (scaled by the tensor's largest magnitude) for
the sums and the parameter gradients."""
import functools
import sys

import numpy as np
import pytest

import link_mlp_ref as ref
import link_ref
from gat_ref import rowdist
from gatdot_ref import bar_rule
from test_gpu_link import _dev, _host, _rows, _transpose_on_device, _window

pytestmark = pytest.mark.gpu

SEED, EPOCH = 0x1234_5678_9ABC, 7
SHAPES = ((32, 32), (96, 64), (128, 128), (32, 128))
CASES = [(p, d, hd, "") for p in ("edges", "n40") for d, hd in SHAPES] + [("edges", 96, 64, "G0"), ("n40", 32, 128, "misaligned")]


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


@functools.lru_cache(maxsize=None)
def graph(name):
    """(n, R, indptr, indices): rows of exactly 0, 1, 31, 32, 33, 64 and 65 entries (the tile and chunk edges) with a
    duplicated pair, then rows of 0 .. 4; or link_ref's pattern whose last row spans several chunks"""
    if name == "n40":
        return (40, 3) + link_ref.pattern(40, 11, 3000)
    n, rng = 70, np.random.default_rng(5)
    lens = rng.integers(0, 5, size=n)
    lens[:7] = (0, 1, 31, 32, 33, 64, 65)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    indices = rng.integers(0, n, size=int(indptr[-1])).astype(np.uint32)
    indices[int(indptr[2]) + 1] = indices[int(indptr[2])]
    return n, 2, indptr, indices


@functools.lru_cache(maxsize=None)
def case(name, d, hd, with_G0=False):
    n, R, indptr, indices = graph(name)
    pairs = ref.pairs_of(indptr, indices, n, R, SEED, EPOCH)
    H, params = ref.inputs(n, d, hd, 100 * d + hd, *pairs[:2])
    G0 = np.random.default_rng(d).standard_normal((n, d)).astype(np.float32) if with_G0 else None
    want, twin = (ref.loss_grad(H, params, *pairs, G0=G0, dt=dt) for dt in (np.float64, np.float32))
    ref.check(want, twin)
    return dict(H=H, params=params, G0=G0, want=want, twin=twin)


def _errors(got, want):
    """the three measures of a result dict(G, sums, W1, b1, w2, b2) against the float64 one"""
    return dict(G=float(rowdist(got["G"], want["G"], want["scale"]).max()),
                sums=max(abs(g - w) / w for g, w in zip(got["sums"], want["sums"])),
                params=max(ref.relerr(got[k], want[k]) for k in ref.NAMES))


@functools.lru_cache(maxsize=None)
def bars():
    worst = dict(G=0.0, sums=0.0, params=0.0, scores=0.0)
    for name, d, hd, _ in CASES:
        c = case(name, d, hd)
        worst = {**{k: max(worst[k], v) for k, v in _errors(c["twin"], c["want"]).items()},
                 "scores": max(worst["scores"], ref.relerr(c["twin"]["scores"], c["want"]["scores"]))}
    out = {k: bar_rule(v) for k, v in worst.items()}
    print("[link mlp] the twin's worst:", {k: f"{v:.3e}" for k, v in worst.items()}, "bars:", {k: f"{v:.3e}" for k, v in out.items()})
    return out


def _step_by_hand(pkg, ctx, g, seed, epoch, H, params, G, beta_first, rows, grads, partials):
    """a step through ops alone: draw, sort, bounds, the three launches in their order (P^T from numpy), the pairs launch, the
    sums; returns dict(G, sums, hits, W1, b1, w2, b2) on the host"""
    n, R, indptr, indices = g
    M = int(indptr[-1])
    t_ip, t_ix = link_ref.transpose_pattern(indptr, indices, n)
    heads = np.repeat(np.arange(n, dtype=np.uint32), np.diff(indptr.astype(np.int64)))
    _, (keys, vals, nt) = _transpose_on_device(pkg, ctx, g, epoch, seed)
    loss, (ip, ix, tip, tix, hd_) = pkg.ops.link_mlp_loss, [_dev(a) for a in (indptr, indices, t_ip, t_ix, heads)]
    ctx.sync()                                           # the uploads and fills of torch's stream are done
    loss(ctx, n, n, ip, ix, M, H, params, G, True, 1.0 / M, R, 1.0 / (M * R), seed, epoch, beta_first, *rows[:2])
    loss(ctx, n, n, tip, tix, M, H, params, G, True, 1.0 / M, beta=1.0)
    loss(ctx, n, n, nt, vals, M * R, H, params, G, False, 1.0 / (M * R), beta=1.0)
    pkg.ops.link_mlp_pairs(ctx, H, params, train=(hd_, ix, M, R, n, seed, epoch), weight=1.0 / M, neg_weight=1.0 / (M * R),
                           grads=grads, partials=partials)
    pkg.ops.link_sums(ctx, rows[0], rows[1], n, rows[2])
    ctx.sync()
    words, flat = rows[2].cpu().numpy(), grads.cpu().numpy()
    d, hd = (params[0].t if hasattr(params[0], "N_") else params[0]).shape
    cuts = np.cumsum([0, d * hd, hd, hd, 1])
    return dict(G=_host(G), sums=(float(words[0]), float(words[1])), hits=int(words.view(np.uint32)[2]),
                **{k: flat[lo:hi].copy() for k, lo, hi in zip(ref.NAMES, cuts[:-1], cuts[1:])})


def _work(pkg, d, hd):
    import torch
    return (torch.full((pkg.ops.link_mlp_grad_floats(d, hd),), float("nan"), device="cuda"),
            torch.full((pkg.ops.link_mlp_partial_floats(d, hd),), float("nan"), device="cuda"))


@pytest.mark.parametrize("name,d,hd,kind", CASES)
def test_mlp_loss_pairs_and_sums(pkg, ctx, name, d, hd, kind):
    g, c, bar, mis = graph(name), case(name, d, hd, kind == "G0"), bars(), kind == "misaligned"
    n = g[0]
    H, params = _window(n, d, mis, c["H"]), tuple(_dev(p) for p in c["params"])
    runs = []
    for _ in range(2):                                   # beta = 0 never reads G: it starts as NaN
        G = _window(n, d, mis, c["G0"])
        runs.append(_step_by_hand(pkg, ctx, g, SEED, EPOCH, H, params, G, 1.0 if kind == "G0" else 0.0, _rows(n), *_work(pkg, d, hd)))
    a, b = runs
    assert all(np.asarray(a[k]).view(np.uint32).tolist() == np.asarray(b[k]).view(np.uint32).tolist() for k in ("G",) + ref.NAMES)
    assert (a["sums"], a["hits"]) == (b["sums"], b["hits"])                                     # the same bits
    err = _errors(a, c["want"])
    print(f"[link mlp] {name} d={d} hd={hd} {kind}:", {k: f"{v / bar[k]:.3f} of its bar" for k, v in err.items()})
    assert a["hits"] == c["want"]["hits"]
    assert all(err[k] <= bar[k] for k in err), (err, bar)


@pytest.mark.parametrize("m", (1, 32, 33, 1000))
@pytest.mark.parametrize("d,hd,misaligned", [(96, 64, False), (128, 128, True)])
def test_mlp_pairs_scores_an_explicit_list(pkg, ctx, m, d, hd, misaligned):
    import torch
    n, rng = 50, np.random.default_rng(m + d)
    src, dst = (rng.integers(0, n, size=m).astype(np.uint32) for _ in range(2))
    H, params = ref.inputs(n, d, hd, 7, src.astype(np.int64), dst.astype(np.int64))
    want, twin = (ref.forward(H, params, src.astype(np.int64), dst.astype(np.int64), dt)[3] for dt in (np.float64, np.float32))
    bar = bar_rule(max(ref.relerr(twin, want), bars()["scores"]))
    out = torch.full((m + 40,), float("nan"), device="cuda")
    operands = (_window(n, d, misaligned, H), tuple(_dev(p) for p in params))
    pairs = (_dev(src), _dev(dst), m)
    ctx.sync()
    pkg.ops.link_mlp_pairs(ctx, *operands, pairs=pairs, out=out)
    ctx.sync()
    got = out.cpu().numpy()
    assert np.isnan(got[m:]).all()                       # the tile beyond the list wrote nothing
    assert ref.relerr(got[:m], want) <= bar


def _bits(tensors):
    return [np.asarray(t.numpy()).view(np.uint32).copy() for t in tensors]


@pytest.mark.parametrize("fused", (False, True))
def test_train_step_is_the_public_pieces(pkg, ctx, fused):
    n, sizes, hd, adam = 200, [6, 8, 32], 64, (1e-2, 0.9, 0.999, 5e-4, 1e-8)
    ip, ix, dv = pkg.datasets.synth_uniform_csr(n, 5, seed=2)
    X = pkg.dn_matrix.from_numpy(np.random.default_rng(3).standard_normal((n, sizes[0])).astype(np.float32))
    csr = lambda: pkg.csr_matrix(ip.copy(), ix.copy(), dv.copy(), n)
    make = lambda w: pkg.gcn(csr(), sizes, weights=w, fused=fused)
    first = make(None)
    weights = [tuple(a.numpy() for p in layer.params() for a in (p.W, p.b)) for layer in first.layers()]
    encoder_bits = lambda model: _bits(t for layer in model.layers() for p in layer.params() for t in (p.W, p.b))
    models = [make(weights), make(weights)]
    head = pkg.mlp_link_predictor(models[0], csr(), hidden=hd, neg_ratio=2, seed=SEED)
    start = head.weights()
    # the hand-driven side: a bare param_owner over copies of the head's tensors, nothing of link.py
    owner = sys.modules[pkg.__name__ + ".gcn"].param_owner()
    owner.params_table, owner.adam_fused = pkg.mlp_link_predictor.params_table, fused
    grads, partials = _work(pkg, sizes[-1], hd)
    cuts = np.cumsum([0, sizes[-1] * hd, hd, hd, 1])
    for (_, p, gname, mname, vname, _), w, lo, hi in zip(owner.params_table, start, cuts[:-1], cuts[1:]):
        setattr(owner, p, pkg.dn_matrix.from_numpy(w))
        setattr(owner, gname, pkg.dn_matrix(w.shape, buffer=grads[lo:hi]))
        setattr(owner, mname, None)
        setattr(owner, vname, None)
    by_hand = tuple(getattr(owner, p) for p in ref.NAMES)
    g, G, rows, losses, after = (n, 2, ip, ix), pkg.dn_matrix(n, sizes[-1]), _rows(n), [], []
    for step in range(3):
        losses.append(head.train_step(ctx, X, *adam))
        after.append((encoder_bits(models[0]), _bits(head.params())))
        H = models[1](ctx, X, training=True)
        got = _step_by_hand(pkg, ctx, g, SEED, step, H, by_hand, G, 0.0, rows, grads, partials)
        M = int(ip[-1])
        assert (got["sums"][0] / M + got["sums"][1] / (M * 2), got["hits"] / (M * 3)) == losses[-1]
        back = G
        for layer in reversed(models[1].layers()):
            back = layer.backward(ctx, back)
        models[1].adam_update(ctx, *adam)
        owner.adam_update(ctx, *adam)
        ctx.sync()
        assert all((a == b).all() for a, b in zip(after[-1][0], encoder_bits(models[1]))), step
        assert all((a == b).all() for a, b in zip(after[-1][1], _bits(by_hand))), step
    assert all((a != b.view(np.uint32)).any() for a, b in zip(after[-1][1], start)) and losses[-1][0] < losses[0][0]
    assert head.epoch == 3 and {"link-loss", "link-wgrad"} <= set(ctx.timers)
    # a replayed step: restored weights, the first step's negatives
    again = pkg.mlp_link_predictor(make(weights), csr(), hidden=hd, neg_ratio=2, seed=SEED + 1, weights=start)
    again.set_negatives(seed=SEED, epoch=0)
    assert again.train_step(ctx, X, *adam) == losses[0]
    assert all((a == b).all() for a, b in zip(after[0][0] + after[0][1], encoder_bits(again.model) + _bits(again.params())))
