"""The bf16 MLP link decoder's contract (include/mggcn.h, "MLP decoder, bf16 operands") in numpy over the flat list of a step's
pairs, the roundings where the contract names them.  float64 is the reference, float32 with the same roundings the twin whose
distance sets the bars (gatdot_ref.bar_rule): it meets a dz on a rounding midpoint that goes the other way as the device does.
Input families: link_mlp_ref.inputs (all exact in bf16: the fp32 decoder's z) and rounding_inputs (every rounding bites)."""
import numpy as np

import link_mlp_ref as base
import link_ref
from bf16_ref import round_bf16

SLOPE, NAMES = base.SLOPE, base.NAMES


def rb(a, dt):                                           # bf16(a) as ``dt``: through fp32, round to nearest even
    return round_bf16(np.asarray(a).astype(np.float32)).astype(dt)


def forward(H, params, us, vs, dt=np.float64):
    """(x, z, a, s) of the pairs in ``dt``"""
    W1, b1, w2, b2 = [np.asarray(p, dtype=np.float32) for p in params]
    Hb = rb(H, dt)
    x = rb(Hb[us] * Hb[vs], dt)
    z = x @ rb(W1, dt) + b1.astype(dt)
    a = np.where(z > 0, z, dt(SLOPE) * z)
    return x, z, a, a @ w2.astype(dt)[0] + b2.astype(dt)[0, 0]


def loss_grad(H, params, us, vs, positive, weight, G0=None, dt=np.float64):
    """link_mlp_ref.loss_grad's dict for the bf16 decoder"""
    Hb, W1b, w2 = rb(H, dt), rb(params[0], dt), np.asarray(params[2], dtype=np.float32).astype(dt)
    x, z, a, s = forward(H, params, us, vs, dt)
    g, loss, hit = np.empty_like(s), np.empty_like(s), np.empty(s.size, dtype=bool)
    for label in (True, False):
        k = positive == label
        g[k], loss[k], hit[k] = link_ref.pair(s[k], label, weight[k].astype(dt), dt)
    dz_full = g[:, None] * w2 * np.where(z > 0, dt(1), dt(SLOPE))
    dz = rb(dz_full, dt)
    dx = dz @ W1b.T
    G = np.zeros_like(Hb) if G0 is None else np.asarray(G0, dtype=np.float32).astype(dt)
    scale = np.abs(G).astype(np.float64)
    for ends, other in ((us, vs), (vs, us)):            # the walk over P (and the negatives), then the transposes
        np.add.at(G, ends, dx * Hb[other])
        np.add.at(scale, ends, np.abs((dx * Hb[other]).astype(np.float64)))
    return dict(scores=s.astype(np.float64), z=z, sums=(float(loss[positive].sum()), float(loss[~positive].sum())),
                hits=int(hit.sum()), G=G, scale=scale, W1=x.T @ dz, b1=dz_full.sum(axis=0)[None, :],
                w2=(g[:, None] * a).sum(axis=0)[None, :], b2=g.sum().reshape(1, 1))


def rounding_inputs(n, d, hd, seed, us, vs):
    """(H, params) as float32: |Hb| = k / 128 (k in [128, 255]) times 1/2 or 1 and W1b in eighths are bf16 values, the operands
    handed over are Hb (1 +- 2^-12) and W1b (1 +- 2^-12) -- exact in fp32, rounding back to their parents, the lower ones only to
    nearest.  With b1 in odd multiples of 2^-13 every z is an odd multiple of 2^-13: exact in fp32 in any order, never 0."""
    for s in range(seed, seed + 64):
        rng = np.random.default_rng(s)
        Hb = rng.integers(128, 256, size=(n, d)) / 128.0 * rng.choice([0.5, 1.0], size=(n, d)) * rng.choice([-1.0, 1.0], size=(n, d))
        W1b = rng.integers(-8, 9, size=(d, hd)) / 8.0
        b1 = (2 * rng.integers(-64, 64, size=(1, hd)) + 1) / 8192.0
        w2 = rng.standard_normal((1, hd)) / np.sqrt(hd * d)
        b2 = rng.standard_normal((1, 1)) * 0.1
        H = (Hb * (1 + rng.choice([-1.0, 1.0], size=Hb.shape) / 4096)).astype(np.float32)
        W1 = (W1b * (1 + rng.choice([-1.0, 1.0], size=W1b.shape) / 4096)).astype(np.float32)
        params = (W1,) + tuple(a.astype(np.float32) for a in (b1, w2, b2))
        if np.abs(forward(H, params, us, vs)[3]).min() > 2e-3:
            assert (round_bf16(H) == Hb).all() and (round_bf16(W1) == W1b).all() and (H != Hb).all()
            return H, params
    raise AssertionError("no seed keeps the scores away from 0")


def check(want, twin):
    """link_mlp_ref.check's conditions with the kink margin of the family at hand: z never 0 and the same in both precisions"""
    z, s = want["z"], want["scores"]
    assert np.abs(z).min() >= 2.0 ** -13 and (twin["z"] == z).all()             # exact in fp32, the same side of the kink
    assert (z > 0).any() and (z < 0).any()                                      # hidden units on both sides of 0
    assert ((z > 0).any(axis=0) & (z < 0).any(axis=0)).any()                    # a unit changes side between pairs
    assert np.abs(s).min() > 1e-3 and twin["hits"] == want["hits"] and s.min() < 0 < s.max()    # no score hides at 0
