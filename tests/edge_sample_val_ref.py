"""The edge sample WITH VALUES and the row-split plan rule on the host, for the edge_rescale tests: the contracts of
mggcn_edge_sample_rowscale_f32 / _compact_val_f32 and of the device plan builder (include/mggcn.h), restated in numpy from
their definitions alone, and float64 forwards of gcn and sage(aggr="mean") over a restated sample.

The keep bit is edge_sample_ref's.  "row": a kept entry of destination i is multiplied by r_i = S_i / S'_i (row sum over kept
row sum; 0 where S'_i == 0).  "inverse": a kept entry with i != j is multiplied by fp32(2^32 / t_i) (1 for t_i == 0xFFFFFFFF,
0 for t_i == 0)."""
import numpy as np

import edge_sample_ref as ref

FULL = 0xFFFFFFFF
NO_SLOT = 0xFFFFFFFF


def inverse_factors(thr):
    """one Python float64 division per destination, rounded to fp32 once"""
    out = np.empty(len(thr), dtype=np.float32)
    for i, t in enumerate(int(x) for x in thr):
        out[i] = 1.0 if t == FULL else 0.0 if t == 0 else np.float32(4294967296.0 / float(t))
    return out


def row_factors(indptr, indices, values, thr, row0=0, col0=0, seed=0, epoch=0):
    """(r64, kept-whole mask, keeps-nothing mask, row length) of a forward matrix: r in float64 from float64 sums"""
    kept = ref.keep_mask(indptr, indices, thr, 0, row0, col0, seed, epoch)
    n = indptr.size - 1
    rows = np.repeat(np.arange(n), np.diff(indptr.astype(np.int64)))
    v = values[: rows.size].astype(np.float64)
    S = np.bincount(rows, weights=v, minlength=n)
    Sk = np.bincount(rows[kept], weights=v[kept], minlength=n)
    length = np.diff(indptr.astype(np.int64))
    n_kept = np.bincount(rows[kept], minlength=n)
    r = np.divide(S, Sk, out=np.zeros(n), where=Sk != 0)
    return r, (n_kept == length) & (Sk != 0), Sk == 0, length


def sample_val(indptr, indices, values, thr, transposed, scale, scale_self, row0=0, col0=0, seed=0, epoch=0):
    """(counts, indptr, indices, values) of the sample with values: value * scale[destination local index] in fp32, a self-loop
    (global destination == global source) left alone when ``scale_self`` is false; scale None: no factor"""
    kept = ref.keep_mask(indptr, indices, thr, transposed, row0, col0, seed, epoch)
    counts, out_ip, out_ix = ref.sample(indptr, indices, thr, transposed, row0, col0, seed, epoch)
    dst, src, at = ref.pairs(indptr, indices, transposed, row0, col0)
    v = values[: kept.size].astype(np.float32)
    if scale is not None:
        f = np.asarray(scale, dtype=np.float32)[at.astype(np.int64)]
        scaled = v * f                                           # one fp32 multiply
        v = scaled if scale_self else np.where(dst == src, v, scaled)
    return counts, out_ip, out_ix, np.ascontiguousarray(v[kept], dtype=np.float32)


def transpose_values(indptr, indices, values, n_src):
    """gat_ref.transpose_pattern with the values carried along: (t_indptr, t_indices, t_values) -- entries sorted by (column,
    row), equal pairs in their original order"""
    from gat_ref import transpose_pattern
    n = indptr.size - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr.astype(np.int64)))
    order = np.argsort(indices[: rows.size].astype(np.int64) * n + rows, kind="stable")
    tp, tx = transpose_pattern(indptr, indices, n_src)
    assert (tx == rows[order]).all()
    return tp, tx, np.ascontiguousarray(np.asarray(values)[: rows.size][order])


def triples(indptr, indices, values, transposed):
    """the sorted (destination, source, value bits) of a CSR with values"""
    dst, src, _ = ref.pairs(indptr, indices, transposed)
    bits = np.asarray(values, dtype=np.float32).view(np.uint32).astype(np.uint64)
    t = np.stack([dst, src, bits], axis=1)
    return t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))]


# ---- the row-split rule ----------------------------------------------------------------------------------------------------------
def row_cost(length, split):
    """(items, slots, split rows) of one row"""
    if length <= split + split // 2:
        return 1, 0, 0
    parts = (length + split - 1) // split
    return parts, parts, 1


def capacity(indptr, split):
    tot = [0, 0, 0]
    for length in np.diff(np.asarray(indptr).astype(np.int64)):
        for k, c in enumerate(row_cost(int(length), split)):
            tot[k] += c
    return tuple(tot)


def rowsplit_tables(indptr, split):
    """rowsplit_build's items BEFORE its sort, i.e. in row order: (items [k x 4], split rows [s x 4], (items, slots, split rows))"""
    items, rows, slots = [], [], 0
    ip = [int(x) for x in indptr]
    for r in range(len(ip) - 1):
        b, e = ip[r], ip[r + 1]
        length = e - b
        if length <= split + split // 2:
            items.append((r, b, e, NO_SLOT))
            continue
        parts = (length + split - 1) // split
        rows.append((r, slots, parts, 0))
        for k in range(parts):
            items.append((r, b + length * k // parts, b + length * (k + 1) // parts, slots))
            slots += 1
    return (np.array(items, dtype=np.uint32).reshape(-1, 4), np.array(rows, dtype=np.uint32).reshape(-1, 4),
            (len(items), slots, len(rows)))


# ---- float64 forwards over a restated sample --------------------------------------------------------------------------------------
def _dense(csr, n):
    ip, ix, v = csr
    M = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(ip.astype(np.int64)))
    np.add.at(M, (rows, ix[: rows.size].astype(np.int64)), np.asarray(v, dtype=np.float64)[: rows.size])
    return M


def _lrelu(x, slope=0.01):
    return np.maximum(x, slope * x)


def _xent(Z, Y):
    Z = Z - Z.max(axis=1, keepdims=True)
    logp = Z - np.log(np.exp(Z).sum(axis=1, keepdims=True))
    return float(-logp[np.arange(Z.shape[0]), np.asarray(Y).reshape(-1)].mean())


def gcn_loss(F, n, X, Y, weights, round_operand=None):
    """softmax cross-entropy of gcn's forward over the forward matrix F = (indptr, indices, values): GEMM first where out <= in
    (the bias is aggregated with the product), aggregation first otherwise; leaky ReLU on every layer but the last.
    ``round_operand``: what the aggregation does to its dense operand (bf16 rounding), None: nothing"""
    M, H = _dense(F, n), np.asarray(X, dtype=np.float64)
    rnd = round_operand or (lambda a: a)
    for li, (W, b) in enumerate(weights):
        W, b = np.asarray(W, dtype=np.float64), np.asarray(b, dtype=np.float64).reshape(1, -1)
        H = M @ rnd(H @ W + b) if W.shape[1] <= W.shape[0] else (M @ rnd(H)) @ W + b
        if li + 1 < len(weights):
            H = _lrelu(H)
    return _xent(H, Y)


def sage_mean_loss(F, n, X, Y, weights, round_operand=None):
    """the same for sage(aggr="mean"): Y = (F H) W_l + b_l + H W_r + b_r"""
    M, H = _dense(F, n), np.asarray(X, dtype=np.float64)
    rnd = round_operand or (lambda a: a)
    for li, (W_l, b_l, W_r, b_r) in enumerate(weights):
        W_l, b_l, W_r, b_r = (np.asarray(a, dtype=np.float64) for a in (W_l, b_l, W_r, b_r))
        H = (M @ rnd(H)) @ W_l + b_l.reshape(1, -1) + H @ W_r + b_r.reshape(1, -1)
        if li + 1 < len(weights):
            H = _lrelu(H)
    return _xent(H, Y)


def bf16_round(a):
    """round to nearest even to bf16, back in float64"""
    u = np.asarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return u.astype(np.uint32).view(np.float32).astype(np.float64)
