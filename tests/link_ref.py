"""The link head's contract (include/mggcn.h, "link prediction") restated in numpy: the negatives from dropout_ref's Philox,
their transpose by a stable argsort and searchsorted, and loss, per-pair scalar and gradient looped pair by pair in the
documented order -- float64 is the reference, float32 the twin whose distance from it sets the bar (eight times the twin's
worst, never above gat_ref.ROW_TOL: the project's rule)."""
import numpy as np

import dropout_ref

LINK_DOMAIN = 0xE0000000
SPECIAL_ROWS = (0, 1, 63, 64, 65, 130)


def negatives(indptr, n, R, seed, epoch):
    """(tails [M x R], heads [M]): negative (p, r) is (heads[p], tails[p, r])"""
    ip = np.asarray(indptr).astype(np.int64)
    M = int(ip[-1])
    heads = np.repeat(np.arange(ip.size - 1, dtype=np.uint32), np.diff(ip))
    p = np.arange(M, dtype=np.uint64)[:, None]
    r = np.arange(R, dtype=np.uint64)[None, :]
    key = (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    w = dropout_ref.philox4x32_10((p, r >> np.uint64(2), LINK_DOMAIN, int(epoch) & 0xFFFFFFFF), key)
    word = np.choose((r & np.uint64(3)).astype(np.int64) + np.zeros((M, 1), dtype=np.int64), [np.asarray(x, dtype=np.uint64) for x in w])
    return ((word * np.uint64(n)) >> np.uint64(32)).astype(np.uint32).reshape(M, R), heads


def negative_transpose(tails, heads, n):
    """(sorted keys, sorted values, nt_indptr): the draw in order of p R + r, sorted stably on the tail"""
    keys = tails.reshape(-1)
    vals = np.repeat(heads, tails.shape[1])
    order = np.argsort(keys, kind="stable")
    return keys[order], vals[order], np.searchsorted(keys[order], np.arange(n + 1), side="left").astype(np.uint32)


def transpose_pattern(indptr, indices, n):
    """P^T with every row's entries in the order of their source rows"""
    ip = np.asarray(indptr).astype(np.int64)
    rows = np.repeat(np.arange(ip.size - 1), np.diff(ip))
    order = np.argsort(np.asarray(indices), kind="stable")
    return (np.searchsorted(np.asarray(indices)[order], np.arange(n + 1), side="left").astype(np.uint32),
            rows[order].astype(np.uint32))


def softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def pair(s, positive, w, dt):
    """(g, loss term, hit) of an array of scores: sigma(s) - 1 formed as -sigma(-s)"""
    e = np.exp(-np.abs(s))
    big, small = dt(1) / (dt(1) + e), e / (dt(1) + e)
    if positive:
        return -np.where(s >= 0, small, big) * w, softplus(-s), s > 0
    return np.where(s >= 0, big, small) * w, softplus(s), ~(s > 0)


def loss_grad(indptr, indices, H, R, seed, epoch, G0=None, dtype=np.float64):
    """dict(loss, hits, G, scale, sums, scores): the three walks in their order, each row's pairs in entry order (walk (a):
    per chunk of 64 entries the positives, then the negatives r = 0 .. R - 1).  G = G0-free sum (G0 None) or the third walk's
    result onto beta = 1 of the second, and so on; with G0 the FIRST walk adds onto it too (the kernel test's beta = 1).
    scale: per element the sum of the magnitudes of its terms (the row-scaled measure's yardstick)."""
    dt = dtype
    H = np.asarray(H, dtype=np.float32).astype(dt)
    n, M = H.shape[0], int(indptr[-1])
    tails, heads = negatives(indptr, n, R, seed, epoch)
    _, nt_vals, nt_ip = negative_transpose(tails, heads, n)
    t_ip, t_ix = transpose_pattern(indptr, indices, n)
    w_pos, w_neg = dt(1.0 / M), dt(1.0 / (M * R))
    G = np.zeros_like(H) if G0 is None else np.asarray(G0, dtype=np.float32).astype(dt)
    scale = np.abs(G).astype(np.float64)
    sums, hits, scores = [dt(0), dt(0)], 0, []

    def walk(x, ys, positive, w, acc, count):
        """acc and the sums take the pairs one after the other (cumsum adds in sequence, in dt)"""
        nonlocal hits
        ys = np.asarray(ys, dtype=np.int64)
        if not ys.size:
            return acc
        s = (H[ys] * H[x]).astype(dt).cumsum(axis=1)[:, -1]
        g, l, hit = pair(s, positive, w, dt)
        terms = g.astype(dt)[:, None] * H[ys]
        scale[x] += np.abs(terms.astype(np.float64)).sum(axis=0)
        if count:
            k = 0 if positive else 1
            sums[k] = np.concatenate([[sums[k]], l.astype(dt)]).cumsum()[-1]
            hits += int(hit.sum())
            scores.extend(s.astype(np.float64).tolist())
        return np.vstack([acc[None, :], terms]).cumsum(axis=0)[-1]

    for launch in range(3):
        for x in range(n):
            acc = np.zeros(H.shape[1], dtype=dt)
            if launch == 0:
                beg, end = int(indptr[x]), int(indptr[x + 1])
                for base in range(beg, end, 64):
                    top = min(base + 64, end)
                    acc = walk(x, indices[base:top], True, w_pos, acc, True)
                    for r in range(R):
                        acc = walk(x, tails[base:top, r], False, w_neg, acc, True)
            elif launch == 1:
                acc = walk(x, t_ix[int(t_ip[x]):int(t_ip[x + 1])], True, w_pos, acc, False)
            else:
                acc = walk(x, nt_vals[int(nt_ip[x]):int(nt_ip[x + 1])], False, w_neg, acc, False)
            G[x] = G[x] + acc
    loss = float(sums[0]) / M + float(sums[1]) / (M * R)
    return dict(loss=loss, hits=hits, G=G, scale=scale, sums=(float(sums[0]), float(sums[1])), scores=np.array(scores))


def loss_only(indptr, indices, H, R, seed, epoch):
    """the float64 loss, vectorised (the central difference of the reference's own sanity check)"""
    H = np.asarray(H, dtype=np.float64)
    tails, heads = negatives(indptr, H.shape[0], R, seed, epoch)
    s_pos = np.einsum("ij,ij->i", H[heads], H[np.asarray(indices)])
    s_neg = np.einsum("irj,irj->ir", np.repeat(H[heads][:, None, :], R, axis=1), H[tails])
    return softplus(-s_pos).mean() + softplus(s_neg).mean()


def pattern(n, seed, M=None):
    """(indptr, indices) of an n x n pattern: rows 0 .. 5 of SPECIAL_ROWS entries (where n allows: at most n per row is NOT
    required, duplicates are pairs of their own), every other row of 0 .. 4; with ``M`` the last row takes what is missing"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 5, size=n)
    lens[:len(SPECIAL_ROWS)] = SPECIAL_ROWS
    if M is not None:
        lens[-1] += M - int(lens.sum())
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    return indptr, rng.integers(0, n, size=int(indptr[-1])).astype(np.uint32)


def embeddings(indptr, indices, n, d, R, seed, epoch, spread=10.0):
    """H [n x d] fp32 whose scores have a standard deviation of about ``spread`` (both softplus branches, a saturated sigma),
    from the first generator seed at which no score of a pair of the step lies within 1e-3 of 0"""
    tails, heads = negatives(indptr, n, R, seed, epoch)
    us = np.concatenate([heads, np.repeat(heads, R)])
    vs = np.concatenate([np.asarray(indices), tails.reshape(-1)])
    for s in range(64):
        H = (np.random.default_rng(1000 * d + s).standard_normal((n, d)) * np.sqrt(spread / np.sqrt(d))).astype(np.float32)
        S = H.astype(np.float64) @ H.astype(np.float64).T
        if np.abs(S[us, vs]).min() > 2e-3:
            return H
    raise AssertionError("no seed keeps the scores away from 0")
