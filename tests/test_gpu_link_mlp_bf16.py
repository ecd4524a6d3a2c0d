"""The bf16 MLP link decoder on the device against tests/link_mlp_bf16_ref.py, as test_gpu_link_mlp.py tests the fp32 one: a
step through the bf16 ops on its graphs and shapes and on both input families, explicit lists, train_step against the step
driven by hand.  Bars: gatdot_ref.bar_rule of the float32 twin's worst distance from float64 over the cases below, in the fp32
test's measures; on the family that is exact in bf16 the forward also meets the fp32 test's own bars."""
import functools
import sys

import numpy as np
import pytest

import link_mlp_bf16_ref as ref
import link_mlp_ref
import link_ref
import test_gpu_link_mlp as f32
from gatdot_ref import bar_rule
from test_gpu_link import _dev, _host, _rows, _transpose_on_device, _window

pytestmark = pytest.mark.gpu

SEED, EPOCH = f32.SEED, f32.EPOCH
CASES = [c + (fam,) for fam in ("exact", "rounding") for c in f32.CASES]


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


@functools.lru_cache(maxsize=None)
def case(name, d, hd, fam, with_G0=False):
    n, R, indptr, indices = f32.graph(name)
    pairs = link_mlp_ref.pairs_of(indptr, indices, n, R, SEED, EPOCH)
    make = link_mlp_ref.inputs if fam == "exact" else ref.rounding_inputs
    H, params = make(n, d, hd, 100 * d + hd, *pairs[:2])
    G0 = np.random.default_rng(d).standard_normal((n, d)).astype(np.float32) if with_G0 else None
    want, twin = (ref.loss_grad(H, params, *pairs, G0=G0, dt=dt) for dt in (np.float64, np.float32))
    ref.check(want, twin)
    if fam == "exact":                                   # nothing of the forward is rounded: the fp32 decoder's z
        assert (want["z"] == link_mlp_ref.forward(H, params, *pairs[:2])[1]).all()
    return dict(H=H, params=params, G0=G0, want=want, twin=twin)


@functools.lru_cache(maxsize=None)
def bars():
    worst = dict(G=0.0, sums=0.0, params=0.0, scores=0.0)
    for name, d, hd, _, fam in CASES:
        c = case(name, d, hd, fam)
        worst = {**{k: max(worst[k], v) for k, v in f32._errors(c["twin"], c["want"]).items()},
                 "scores": max(worst["scores"], link_mlp_ref.relerr(c["twin"]["scores"], c["want"]["scores"]))}
    out = {k: bar_rule(v) for k, v in worst.items()}
    print("[link mlp bf16] the twin's worst:", {k: f"{v:.3e}" for k, v in worst.items()}, "bars:", {k: f"{v:.3e}" for k, v in out.items()})
    return out


def _images(pkg, ctx, H, W1):
    import torch
    n, d = (H.n(), H.m()) if hasattr(H, "N_") else H.shape
    dd, hd = (W1.n(), W1.m()) if hasattr(W1, "N_") else W1.shape
    Hb = torch.empty((n, d), dtype=torch.bfloat16, device="cuda")
    image = torch.empty(pkg.ops.link_mlp_image_halves(dd, hd), dtype=torch.bfloat16, device="cuda")
    ctx.sync()
    pkg.ops.convert_bf16(ctx, H, Hb)
    pkg.ops.link_mlp_pack_bf16(ctx, W1, image)
    return Hb, image


def _step_by_hand(pkg, ctx, g, seed, epoch, H, params, G, beta_first, rows, grads, partials):
    """test_gpu_link_mlp._step_by_hand with the bf16 ops: pack, draw, sort, bounds, the three launches, the pairs launch, the sums"""
    n, R, indptr, indices = g
    M = int(indptr[-1])
    t_ip, t_ix = link_ref.transpose_pattern(indptr, indices, n)
    heads = np.repeat(np.arange(n, dtype=np.uint32), np.diff(indptr.astype(np.int64)))
    _, (keys, vals, nt) = _transpose_on_device(pkg, ctx, g, epoch, seed)
    loss, (ip, ix, tip, tix, hd_) = pkg.ops.link_mlp_loss_bf16, [_dev(a) for a in (indptr, indices, t_ip, t_ix, heads)]
    Hb, image = _images(pkg, ctx, H, params[0])
    packed = (image,) + tuple(params[1:])
    loss(ctx, n, n, ip, ix, M, Hb, packed, G, True, 1.0 / M, R, 1.0 / (M * R), seed, epoch, beta_first, *rows[:2])
    loss(ctx, n, n, tip, tix, M, Hb, packed, G, True, 1.0 / M, beta=1.0)
    loss(ctx, n, n, nt, vals, M * R, Hb, packed, G, False, 1.0 / (M * R), beta=1.0)
    pkg.ops.link_mlp_pairs_bf16(ctx, Hb, packed, train=(hd_, ix, M, R, n, seed, epoch), weight=1.0 / M, neg_weight=1.0 / (M * R),
                                grads=grads, partials=partials)
    pkg.ops.link_sums(ctx, rows[0], rows[1], n, rows[2])
    ctx.sync()
    words, flat = rows[2].cpu().numpy(), grads.cpu().numpy()
    d, hd = (params[0].t if hasattr(params[0], "N_") else params[0]).shape
    cuts = np.cumsum([0, d * hd, hd, hd, 1])
    return dict(G=_host(G), sums=(float(words[0]), float(words[1])), hits=int(words.view(np.uint32)[2]),
                **{k: flat[lo:hi].copy() for k, lo, hi in zip(ref.NAMES, cuts[:-1], cuts[1:])})


@pytest.mark.parametrize("name,d,hd,kind,fam", CASES)
def test_bf16_loss_pairs_and_sums(pkg, ctx, name, d, hd, kind, fam):
    g, c, bar, mis = f32.graph(name), case(name, d, hd, fam, kind == "G0"), bars(), kind == "misaligned"
    n, runs = g[0], []
    H, params = _window(n, d, mis, c["H"]), tuple(_dev(p) for p in c["params"])
    for _ in range(2):                                   # beta = 0 never reads G: it starts as NaN
        G = _window(n, d, mis, c["G0"])
        runs.append(_step_by_hand(pkg, ctx, g, SEED, EPOCH, H, params, G, 1.0 if kind == "G0" else 0.0, _rows(n), *f32._work(pkg, d, hd)))
    a, b = runs                                          # the same bits
    assert all(np.asarray(a[k]).view(np.uint32).tolist() == np.asarray(b[k]).view(np.uint32).tolist() for k in ("G",) + ref.NAMES)
    assert (a["sums"], a["hits"]) == (b["sums"], b["hits"]) and a["hits"] == c["want"]["hits"]
    err = f32._errors(a, c["want"])
    print(f"[link mlp bf16] {name} d={d} hd={hd} {kind} {fam}:", {k: f"{v / bar[k]:.3f} of its bar" for k, v in err.items()})
    assert all(err[k] <= bar[k] for k in err), (err, bar)
    if fam == "exact":                                   # the forward is the fp32 decoder's: its own bar for the sums
        assert err["sums"] <= f32.bars()["sums"], (err, f32.bars())


@pytest.mark.parametrize("fam", ("exact", "rounding"))
@pytest.mark.parametrize("m", (1, 32, 33, 1000))
@pytest.mark.parametrize("d,hd", [(96, 64), (128, 128)])
def test_bf16_pairs_scores_an_explicit_list(pkg, ctx, m, d, hd, fam):
    import torch
    n, rng = 50, np.random.default_rng(m + d)
    src, dst = (rng.integers(0, n, size=m).astype(np.int64) for _ in range(2))
    H, params = (link_mlp_ref.inputs if fam == "exact" else ref.rounding_inputs)(n, d, hd, 7, src, dst)
    want, twin = (ref.forward(H, params, src, dst, dt)[3] for dt in (np.float64, np.float32))
    bar = bar_rule(max(link_mlp_ref.relerr(twin, want), (f32.bars() if fam == "exact" else bars())["scores"]))
    out = torch.full((m + 40,), float("nan"), device="cuda")
    W1 = _dev(params[0])
    Hb, image = _images(pkg, ctx, _window(n, d, d == 128, H), W1)
    pairs = (_dev(src.astype(np.uint32)), _dev(dst.astype(np.uint32)), m)
    ctx.sync()
    pkg.ops.link_mlp_pairs_bf16(ctx, Hb, (image,) + tuple(_dev(p) for p in params[1:]), pairs=pairs, out=out)
    ctx.sync()
    got = out.cpu().numpy()
    assert np.isnan(got[m:]).all()                       # the tile beyond the list wrote nothing
    assert link_mlp_ref.relerr(got[:m], want) <= bar


@pytest.mark.parametrize("fused", (False, True))
def test_bf16_train_step_is_the_public_pieces(pkg, ctx, fused):
    n, sizes, hd, adam = 200, [6, 8, 32], 64, (1e-2, 0.9, 0.999, 5e-4, 1e-8)
    ip, ix, dv = pkg.datasets.synth_uniform_csr(n, 5, seed=2)
    X = pkg.dn_matrix.from_numpy(np.random.default_rng(3).standard_normal((n, sizes[0])).astype(np.float32))
    csr = lambda: pkg.csr_matrix(ip.copy(), ix.copy(), dv.copy(), n)
    first = pkg.gcn(csr(), sizes, fused=fused)
    weights = [tuple(a.numpy() for p in layer.params() for a in (p.W, p.b)) for layer in first.layers()]
    models = [pkg.gcn(csr(), sizes, weights=weights, fused=fused) for _ in range(2)]
    head = pkg.mlp_link_predictor(models[0], csr(), hidden=hd, neg_ratio=2, seed=SEED, decoder_dtype="bf16")
    start = head.weights()
    owner = sys.modules[pkg.__name__ + ".gcn"].param_owner()    # the hand-driven side: copies of the head's tensors
    owner.params_table, owner.adam_fused = pkg.mlp_link_predictor.params_table, fused
    grads, partials = f32._work(pkg, sizes[-1], hd)
    cuts = np.cumsum([0, sizes[-1] * hd, hd, hd, 1])
    for (_, p, gname, mname, vname, _), w, lo, hi in zip(owner.params_table, start, cuts[:-1], cuts[1:]):
        vars(owner).update({p: pkg.dn_matrix.from_numpy(w), gname: pkg.dn_matrix(w.shape, buffer=grads[lo:hi]), mname: None, vname: None})
    by_hand = tuple(getattr(owner, p) for p in ref.NAMES)
    g, G, rows, losses, M = (n, 2, ip, ix), pkg.dn_matrix(n, sizes[-1]), _rows(n), [], int(ip[-1])
    for step in range(3):
        losses.append(head.train_step(ctx, X, *adam))
        H = models[1](ctx, X, training=True)
        got = _step_by_hand(pkg, ctx, g, SEED, step, H, by_hand, G, 0.0, rows, grads, partials)
        assert (got["sums"][0] / M + got["sums"][1] / (M * 2), got["hits"] / (M * 3)) == losses[-1]
        back = G
        for layer in reversed(models[1].layers()):
            back = layer.backward(ctx, back)
        models[1].adam_update(ctx, *adam)
        owner.adam_update(ctx, *adam)
        ctx.sync()
        for a, b in zip(head.params(), by_hand):
            assert (a.numpy().view(np.uint32) == b.numpy().view(np.uint32)).all(), step
        for la, lb in zip(models[0].layers(), models[1].layers()):
            assert all((ta.numpy() == tb.numpy()).all() for pa, pb in zip(la.params(), lb.params()) for ta, tb in ((pa.W, pb.W), (pa.b, pb.b))), step
    assert losses[-1][0] < losses[0][0] and (head.W1.numpy() != start[0]).any()
    assert {"link-loss", "link-wgrad", "link-pack"} <= set(ctx.timers) and all(str(p.t.dtype) == "torch.float32" for p in head.params())
    import torch                                         # score: the bf16 decoder on the model's H
    pairs = np.random.default_rng(9).integers(0, n, size=(77, 2))
    scores = head.score(ctx, X, pairs).numpy().reshape(-1)
    Hb, image = _images(pkg, ctx, models[0](ctx, X), head.W1)
    out = torch.empty(77, device="cuda")
    pkg.ops.link_mlp_pairs_bf16(ctx, Hb, (image, head.b1, head.w2, head.b2),
                                pairs=(_dev(pairs[:, 0].astype(np.uint32)), _dev(pairs[:, 1].astype(np.uint32)), 77), out=out)
    ctx.sync()
    assert (scores.view(np.uint32) == out.cpu().numpy().view(np.uint32)).all()
