"""The MLP link decoder's contract (include/mggcn.h, "link prediction, MLP decoder") restated in numpy over the flat list of a
step's pairs: scores, the two loss sums, hits, G = dL/dH and the four parameter gradients -- float64 is the reference, float32
the twin whose distance from it sets the bar (gatdot_ref.bar_rule).  The draw is link_ref's.

The leaky ReLU has a kink, so inputs() keeps every pre-activation away from it: H in multiples of 1/4 within [-2, 2], W1 in
multiples of 1/8 within [-1, 1] and b1 in odd multiples of 1/256 make every z an odd multiple of 1/256 below 2^10 -- exact in
fp32 in any summation order, the same side of 0 in every precision."""
import numpy as np

import link_ref

SLOPE = 0.01
NAMES = ("W1", "b1", "w2", "b2")


def inputs(n, d, hd, seed, us=None, vs=None):
    """(H [n x d], (W1 [d x hd], b1 [1 x hd], w2 [1 x hd], b2 [1 x 1])) as float32, from the first generator seed (``seed``,
    seed + 1, ...) at which no score of the pairs (us, vs) lies within 2e-3 of 0 (link_ref.embeddings' rule)"""
    for s in range(seed, seed + 64):
        rng = np.random.default_rng(s)
        H = rng.integers(-8, 9, size=(n, d)) / 4.0
        W1 = rng.integers(-8, 9, size=(d, hd)) / 8.0
        b1 = (2 * rng.integers(-64, 64, size=(1, hd)) + 1) / 256.0
        w2 = rng.standard_normal((1, hd)) / np.sqrt(hd * d)
        b2 = rng.standard_normal((1, 1)) * 0.1
        H, params = H.astype(np.float32), tuple(a.astype(np.float32) for a in (W1, b1, w2, b2))
        if us is None or np.abs(forward(H, params, us, vs)[3]).min() > 2e-3:
            return H, params
    raise AssertionError("no seed keeps the scores away from 0")


def pairs_of(indptr, indices, n, R, seed, epoch):
    """(us, vs, positive, weight) of a step: the M positives, then the M R negatives in order of p R + r"""
    tails, heads = link_ref.negatives(indptr, n, R, seed, epoch)
    M = heads.size
    us = np.concatenate([heads, np.repeat(heads, R)]).astype(np.int64)
    vs = np.concatenate([np.asarray(indices), tails.reshape(-1)]).astype(np.int64)
    return us, vs, np.arange(us.size) < M, np.where(np.arange(us.size) < M, 1.0 / M, 1.0 / (M * R))


def forward(H, params, us, vs, dt=np.float64):
    """(x, z, a, s) of the pairs in ``dt``"""
    H, (W1, b1, w2, b2) = np.asarray(H, dtype=np.float32).astype(dt), [np.asarray(p, dtype=np.float32).astype(dt) for p in params]
    x = H[us] * H[vs]
    z = x @ W1 + b1
    a = np.where(z > 0, z, dt(SLOPE) * z)
    return x, z, a, a @ w2[0] + b2[0, 0]


def loss_grad(H, params, us, vs, positive, weight, G0=None, dt=np.float64):
    """dict(scores, sums, hits, G, scale, W1, b1, w2, b2): the weighted loss of the pairs and its gradients.  scale: per
    element of G the sum of the magnitudes of its terms (gat_ref.rowdist's yardstick)."""
    Hd, w2 = np.asarray(H, dtype=np.float32).astype(dt), np.asarray(params[2], dtype=np.float32).astype(dt)
    W1 = np.asarray(params[0], dtype=np.float32).astype(dt)
    x, z, a, s = forward(H, params, us, vs, dt)
    g, loss, hit = np.empty_like(s), np.empty_like(s), np.empty(s.size, dtype=bool)
    for label in (True, False):
        k = positive == label
        g[k], loss[k], hit[k] = link_ref.pair(s[k], label, weight[k].astype(dt), dt)
    dz = g[:, None] * w2 * np.where(z > 0, dt(1), dt(SLOPE))
    dx = dz @ W1.T
    G = np.zeros_like(Hd) if G0 is None else np.asarray(G0, dtype=np.float32).astype(dt)
    scale = np.abs(G).astype(np.float64)
    for ends, other in ((us, vs), (vs, us)):            # the walk over P (and the negatives), then the transposes
        np.add.at(G, ends, dx * Hd[other])
        np.add.at(scale, ends, np.abs((dx * Hd[other]).astype(np.float64)))
    return dict(scores=s.astype(np.float64), z=z, sums=(float(loss[positive].sum()), float(loss[~positive].sum())),
                hits=int(hit.sum()), G=G, scale=scale, W1=x.T @ dz, b1=dz.sum(axis=0)[None, :],
                w2=(g[:, None] * a).sum(axis=0)[None, :], b2=g.sum().reshape(1, 1))


def loss_only(H, params, us, vs, positive, weight):
    """the float64 loss of float64 operands (the central difference)"""
    x = H[us] * H[vs]
    z = x @ params[0] + params[1]
    s = np.where(z > 0, z, SLOPE * z) @ params[2][0] + params[3][0, 0]
    return float((np.where(positive, link_ref.softplus(-s), link_ref.softplus(s)) * weight).sum())


def check(want, twin):
    """what a case must show before anything is compared with it"""
    z, s = want["z"], want["scores"]
    assert np.abs(z).min() >= 1 / 256 and (twin["z"] == z).all()                # away from the kink, exact in fp32
    assert (z > 0).any() and (z < 0).any()                                      # hidden units on both sides of 0
    assert ((z > 0).any(axis=0) & (z < 0).any(axis=0)).any()                    # a unit changes side between pairs
    assert np.abs(s).min() > 1e-3 and twin["hits"] == want["hits"]              # the count cannot hide behind a score at 0
    assert s.min() < 0 < s.max()


def relerr(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64).reshape(want.shape) - want).max() / np.abs(want).max())
