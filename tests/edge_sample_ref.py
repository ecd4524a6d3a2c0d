"""The per-epoch edge sample on the host, for the edge-sampling tests: the contract of mggcn_edge_sample_*_u32
(include/mggcn.h) restated in numpy from its definition alone.

Destination i has the threshold t_i = min(floor(q_i 2^32), 2^32 - 1), q_i = keep min(1, fanout / deg_i) in float64; entry
(destination i, source j), both global vertex numbers, is kept in training forward e iff i == j, or t_i == 0xFFFFFFFF, or
word 0 of Philox4x32-10(counter = (j, i, 0xC0000000, e), key = (seed & 0xffffffff, seed >> 32)) is below t_i.  The Philox is
dropout_ref's, the host transpose gat_ref's."""
import math

import numpy as np

from dropout_ref import philox4x32_10
from gat_ref import transpose_pattern

DOMAIN = 0xC0000000
FULL = 0xFFFFFFFF


def thresholds(indptr, fanout, keep):
    """one Python float64 expression per row (no vectorised shortcut: this is the definition)"""
    ip = [int(x) for x in indptr]
    out = np.empty(len(ip) - 1, dtype=np.uint32)
    for r in range(len(ip) - 1):
        deg = ip[r + 1] - ip[r]
        q = float(keep) * (1.0 if fanout is None or deg == 0 else min(1.0, float(fanout) / float(deg)))
        out[r] = min(int(math.floor(q * 4294967296.0)), FULL)
    return out


def pairs(indptr, indices, transposed, row0=0, col0=0):
    """(destination, source, the local index the threshold is read at) of every entry, as uint64 arrays"""
    rows = np.repeat(np.arange(indptr.size - 1, dtype=np.uint64), np.diff(indptr.astype(np.int64)))
    cols = indices[: rows.size].astype(np.uint64)
    r, c = (rows + np.uint64(row0)) & np.uint64(FULL), (cols + np.uint64(col0)) & np.uint64(FULL)
    return (c, r, cols) if transposed else (r, c, rows)


def counters(dst, src, epoch):
    """the Philox counter of every pair"""
    return (src, dst, np.full(dst.shape, DOMAIN, dtype=np.uint64), np.full(dst.shape, int(epoch) & FULL, dtype=np.uint64))


def words(dst, src, seed, epoch):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    if dst.size == 0:
        return np.zeros(0, dtype=np.uint32)
    return philox4x32_10(counters(dst, src, epoch), (seed & FULL, seed >> 32))[0]


def keep_mask(indptr, indices, thr, transposed=0, row0=0, col0=0, seed=0, epoch=0, self_loops=True):
    """True for every entry the sample keeps; ``self_loops=False``: the rule without its first clause (the rate test)"""
    dst, src, at = pairs(indptr, indices, transposed, row0, col0)
    t = np.asarray(thr, dtype=np.uint32)[at.astype(np.int64)]
    kept = (t == np.uint32(FULL)) | (words(dst, src, seed, epoch) < t)
    return kept | (dst == src) if self_loops else kept


def sample(indptr, indices, thr, transposed=0, row0=0, col0=0, seed=0, epoch=0):
    """(counts, indptr, indices) of the sampled pattern: the kept entries of every row in their original order"""
    kept = keep_mask(indptr, indices, thr, transposed, row0, col0, seed, epoch)
    rows = np.repeat(np.arange(indptr.size - 1), np.diff(indptr.astype(np.int64)))
    counts = np.bincount(rows[kept], minlength=indptr.size - 1).astype(np.uint32)
    out_indptr = np.zeros(indptr.size, dtype=np.uint32)
    out_indptr[1:] = np.cumsum(counts.astype(np.uint64)).astype(np.uint32)
    return counts, out_indptr, np.ascontiguousarray(indices[: rows.size][kept], dtype=np.uint32)


def sample_pair(indptr, indices, fanout, keep, seed=0, epoch=0):
    """the sample of a square forward matrix F and of transpose_pattern(F): ((indptr, indices) of F's, of F^T's)"""
    n = indptr.size - 1
    thr = thresholds(indptr, fanout, keep)
    t_indptr, t_indices = transpose_pattern(indptr, indices, n)
    _, ip, ix = sample(indptr, indices, thr, 0, seed=seed, epoch=epoch)
    _, tip, tix = sample(t_indptr, t_indices, thr, 1, seed=seed, epoch=epoch)
    return (ip, ix), (tip, tix)
