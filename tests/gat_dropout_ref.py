"""Attention dropout on the host, for the GAT dropout tests: the mask of the mggcn_gat_*_drop_f32 entry points
(include/mggcn.h) restated in numpy from dropout_ref.philox4x32_10, the contract of those entry points in fp64 with an fp32
twin -- gat_ref.attention with q = keep ? scale : 0 on the terms that carry it --, the cases both test files share, the
mutations the bar is held against, and the reference model with both dropouts.

Entry (global destination i, global source j, head k) is kept iff word k & 3 of
    Philox4x32-10(counter = (j, i, 0x80000000 | (k >> 2), stream), key = (seed & 0xffffffff, seed >> 32))
is >= floor(p * 2^32); i = dst0 + local row of F, j = src0 + local column.  With q_ijk = keep ? fp32(1 / (1 - p)) : 0:
    lse, alpha                   those of gat_ref (the softmax runs over ALL entries of the row)
    out[i, head k] = sum_j (alpha q) Z[j, head k]
    D[i, k] = G[i, head k] . out[i, head k];  dalpha = G[i, head k] . Z[j, head k]
    ds = alpha (q dalpha - D[i, k]) lrelu'(x)
    G_Z[j, head k] = sum_i (alpha q) G[i, head k] + ds_dst[j, k] att[0, head k] + ds_src[j, k] att[1, head k]
"""
import numpy as np

import dropout_ref
import gat_ref as ref
from gat_ref import _segmax, _segsum

DROP_NAMES = ("out", "lse", "D", "ds_dst", "ds_src", "G_Z")     # what the three _drop entry points write
TOP = 0x80000000


# ---- the mask ------------------------------------------------------------------------------------------------------------------------
def words(i, j, K, seed, stream, swap=False, head0=False):
    """uint32 [len(i) x K]: the word of every (entry, head) from global destinations ``i`` and global sources ``j``.  The two
    flags are mutations for the CPU tests: ``swap`` puts (i, j) into the counter, ``head0`` uses head 0's word for every head"""
    i, j = np.asarray(i, dtype=np.uint64), np.asarray(j, dtype=np.uint64)
    assert i.shape == j.shape and (i < 2 ** 32).all() and (j < 2 ** 32).all()
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = (seed & 0xFFFFFFFF, seed >> 32)
    c0, c1 = (i, j) if swap else (j, i)
    out = np.empty((i.size, K), dtype=np.uint32)
    for blk in range((K + 3) // 4):
        w = dropout_ref.philox4x32_10((c0, c1, TOP | blk, int(stream) & 0xFFFFFFFF), key)
        for k in range(4 * blk, min(K, 4 * blk + 4)):
            out[:, k] = w[k & 3]
    if head0:
        out[:] = out[:, :1]
    return out


def entry_words(indptr, indices, K, seed, stream, dst0=0, src0=0, **mut):
    rows = np.repeat(np.arange(indptr.size - 1, dtype=np.uint64), np.diff(indptr.astype(np.int64)))
    return words(rows + np.uint64(dst0), indices.astype(np.uint64) + np.uint64(src0), K, seed, stream, **mut)


def keep_mask(indptr, indices, K, p, seed, stream, dst0=0, src0=0, **mut):
    """bool [nnz x K] in F's entry order: True where the (entry, head) is KEPT"""
    return entry_words(indptr, indices, K, seed, stream, dst0, src0, **mut) >= np.uint32(dropout_ref.params(p)[0])


def drop_tuple(p, seed, stream, dst0=0, src0=0):
    """the (threshold, scale, seed, stream, dst0, src0) of ops.gat_forward(drop=) and of the C ABI's trailing arguments"""
    threshold, scale = dropout_ref.params(p)
    return (threshold, float(scale), int(seed), int(stream), int(dst0), int(src0))


# ---- the formulas, in one precision --------------------------------------------------------------------------------------------------
def attention(indptr, indices, Z, att, K, keep, scale, G=None, Z_dst=None, slope=ref.SLOPE, dtype=np.float64, s_dst=None,
              s_src=None, lse=None, D=None, scales=False, softmax_over_kept=False):
    """gat_ref.attention with attention dropout: ``keep`` bool [nnz x K] in F's entry order, ``scale`` = fp32(1 / (1 - p)).
    The same injectable s_dst, s_src, lse and D, and with ``scales`` the magnitude the terms of every output add up to,
    computed with alpha q where the terms carry q.  ``softmax_over_kept`` is a mutation for the CPU tests: the dropped
    entries leave the softmax sum too (renormalised dropout), which is NOT the contract."""
    T = dtype
    n, n_src, d = indptr.size - 1, Z.shape[0], Z.shape[1]
    dh = d // K
    square = Z_dst is None
    Z3 = np.asarray(Z, dtype=T).reshape(n_src, K, dh)
    Zd3 = Z3 if square else np.asarray(Z_dst, dtype=T).reshape(n, K, dh)
    a3 = np.asarray(att, dtype=T).reshape(2, K, dh)
    rows = np.repeat(np.arange(n), np.diff(indptr.astype(np.int64)))
    cols = indices.astype(np.int64)
    q = np.where(np.asarray(keep, dtype=bool), T(scale), T(0)).astype(T)
    assert q.shape == (cols.size, K)
    r = {}
    s_dst = (Zd3 * a3[0]).sum(axis=2, dtype=T) if s_dst is None else np.asarray(s_dst, dtype=T).reshape(n, K)
    s_src = (Z3 * a3[1]).sum(axis=2, dtype=T) if s_src is None else np.asarray(s_src, dtype=T).reshape(n_src, K)
    x = s_dst[rows] + s_src[cols]
    e = np.where(x > 0, x, T(slope) * x)
    if lse is None:
        em = np.where(keep, e, -np.inf) if softmax_over_kept else e
        m = _segmax(em, indptr)
        m[~np.isfinite(m)] = 0                                  # rows without (kept) entries
        ssum = _segsum(np.exp(em - m[rows]), indptr)
        ssum[ssum == 0] = 1
        lse = (m + np.log(ssum)).astype(T)
    else:
        lse = np.asarray(lse, dtype=T).reshape(n, K)
    alpha = np.exp(e - lse[rows])
    aq = alpha * q                                              # one multiply of the weight by q
    out = _segsum(aq[:, :, None] * Z3[cols], indptr)
    r.update(s_dst=s_dst, s_src=s_src, out=out.reshape(n, d), lse=lse, alpha=alpha)
    if scales:
        sc = r["scale"] = dict(out=_segsum(aq[:, :, None] * np.abs(Z3)[cols], indptr).reshape(n, d), lse=np.maximum(np.abs(lse), 1))
    if G is None:
        return r
    G3 = np.asarray(G, dtype=T).reshape(n, K, dh)
    D = (G3 * out).sum(axis=2, dtype=T) if D is None else np.asarray(D, dtype=T).reshape(n, K)
    dalpha = (G3[rows] * Z3[cols]).sum(axis=2, dtype=T)
    ds = alpha * (q * dalpha - D[rows]) * np.where(x > 0, T(1), T(slope))
    ds_dst = _segsum(ds, indptr)
    order = np.argsort(cols, kind="stable")
    t_indptr = np.zeros(n_src + 1, dtype=np.int64)
    t_indptr[1:] = np.cumsum(np.bincount(cols, minlength=n_src))
    ds_src = _segsum(ds[order], t_indptr)
    G_Z = _segsum((aq[:, :, None] * G3[rows])[order], t_indptr)
    if square:
        G_Z = G_Z + ds_dst[:, :, None] * a3[0]
    G_Z = G_Z + ds_src[:, :, None] * a3[1]
    G_att = np.stack([(ds_dst[:, :, None] * Zd3).sum(axis=0, dtype=T), (ds_src[:, :, None] * Z3).sum(axis=0, dtype=T)])
    r.update(D=D, ds_dst=ds_dst, ds_src=ds_src, G_Z=G_Z.reshape(n_src, d), G_att=G_att.reshape(2, d))
    if scales:
        w = alpha * (q * np.abs(dalpha) + np.abs(D[rows])) * np.where(x > 0, T(1), T(slope))
        sd, ss = _segsum(w, indptr), _segsum(w[order], t_indptr)
        gz = _segsum((aq[:, :, None] * np.abs(G3[rows]))[order], t_indptr) + ss[:, :, None] * np.abs(a3[1])
        if square:
            gz = gz + sd[:, :, None] * np.abs(a3[0])
        sc.update(D=np.abs(G3 * out).sum(axis=2), ds_dst=sd, ds_src=ss, G_Z=gz.reshape(n_src, d))
    return r


def restate64(*a, exact=False, **kw):
    """the fp64 restatement: fp64 arithmetic on the fp32 inputs, rounded to fp32 at the end (exact: left in fp64)"""
    r = attention(*a, dtype=np.float64, **kw)
    return r if exact else {k: v.astype(np.float32) for k, v in r.items() if k != "scale"}


def twin32(*a, **kw):
    """the fp32 twin: the same formulas with every operation in fp32"""
    with np.errstate(over="ignore"):
        return {k: v.astype(np.float32) for k, v in attention(*a, dtype=np.float32, **kw).items()}


# ---- the cases of test_gpu_gat_dropout.py (a), measured on the CPU first ---------------------------------------------------------------
# (K, dh): the float4 path; float4 with one lane per group and k >> 2 up to 3; the element path with two Philox blocks;
# NT = 4 (float4, 65 lanes' worth); NT = 16 (element path, 257 columns)
DROP_SHAPES = [(4, 32), (16, 4), (6, 7), (1, 260), (1, 257)]
DROP_PS = (0.5, 0.9)
SEED, STREAM = 0x123456789ABCDEF, 3 * 64 + 1
RECT_DST0, RECT_SRC0 = 1000, 70000


def drop_cases():
    """(graph name, K, dh, p): kernel_graph_long as F and transposed at every shape and p, and the 200 x 320 block with
    non-zero dst0 / src0 at one float4 and one element shape"""
    return ([(g, K, dh, p) for g in ("long", "longT") for K, dh in DROP_SHAPES for p in DROP_PS]
            + [("rect", K, dh, p) for K, dh in ((4, 32), (6, 7)) for p in DROP_PS])


def case_offsets(name):
    return (RECT_DST0, RECT_SRC0) if name == "rect" else (0, 0)


_cases = {}


def drop_case(name, K, dh, p):
    """inputs (gat_ref.edge_case's for the shapes it has), the mask, the exact restatement with its row scales, and the twin;
    computed once per process"""
    key = (name, K, dh, p)
    if key not in _cases:
        indptr, indices, n_src = ref.edge_graphs()[name]
        n = indptr.size - 1
        Z, Z_dst, G, att = ref.tolerance_inputs(n, n_src, K, dh, att_scale=0.1 * min(1.0, (32.0 / dh) ** 0.5))
        Zd = None if n == n_src else Z_dst
        dst0, src0 = case_offsets(name)
        keep = keep_mask(indptr, indices, K, p, SEED, STREAM, dst0, src0)
        scale = dropout_ref.params(p)[1]
        want = restate64(indptr, indices, Z, att, K, keep, scale, G=G, Z_dst=Zd, exact=True, scales=True)
        twin = twin32(indptr, indices, Z, att, K, keep, scale, G=G, Z_dst=Zd)
        _cases[key] = dict(indptr=indptr, indices=indices, n_src=n_src, Z=Z, Z_dst=Zd, G=G, att=att, keep=keep, qscale=scale,
                           drop=drop_tuple(p, SEED, STREAM, dst0, src0), want=want, scale=want["scale"], twin=twin)
    return _cases[key]


# The bars of the _drop entry points on the row-scaled measure, one per output, fixed on the CPU before any device run.
# TWIN_DROP_MEASURED: the fp32 twin's worst rowdist from the exact restatement over drop_cases() (test_gat_dropout_cpu.py
# prints and asserts it).  Where that is within gat_ref.ROW_TOL / 8 the bar is gat_ref.ROW_TOL; where it is not, the bar is
# eight times the twin's worst, rounded up.  out, lse and D stay at ROW_TOL.  ds_dst, ds_src and G_Z do not, and the reason is
# the measure, not the formulas: a DROPPED entry's ds is alpha (0 - D) lrelu', one term whose scale is alpha |D|, while D
# carries the rounding of sum_c G out, which is relative to sum_c |G out|.  Without dropout D is a convex combination of the
# dalpha and a row with one entry has dalpha = D; with dropout a dropped entry meets a D that nearly cancels (|D| a
# thousandth of sum |G out| in the worst rows at p = 0.9), and ds_src / G_Z of a source with that one entry inherit it.
TWIN_DROP_MEASURED = dict(out=6.80e-7, lse=1.90e-7, D=2.03e-6, ds_dst=8.72e-5, ds_src=4.26e-4, G_Z=4.26e-4)
DROP_TOL = dict(out=ref.ROW_TOL, lse=ref.ROW_TOL, D=ref.ROW_TOL, ds_dst=7.0e-4, ds_src=3.5e-3, G_Z=3.5e-3)


# ---- the count probe of test_gpu_gat_dropout.py (b) --------------------------------------------------------------------------------------
def count_probe(K, dh, transposed=False, seed=SEED, stream=STREAM):
    """gat_ref.probe_block with att = 0 (alpha = 1 / L within an ulp), p = 0.5 (scale = 2: multiples are exact) and a one-hot
    dense operand, hot[v, head k, c] = 1 iff c == (position of v in its row) mod dh.  As F (rows: destinations, hot is Z)
    out[i, k, c] L / 2 is the NUMBER of kept entries of row i and head k at positions = c mod dh.  ``transposed``: the block
    is F^T (rows: sources, entries: destinations, hot is G, lse = log L of the row that lists the destination) and the same
    holds for G_Z[j, k, c]; the mask is then drawn with the roles swapped, as backward_src does.  Returns the block, hot, the
    mask in the block's entry order and those counts [5 x K x dh]."""
    indptr, indices, n_ent = ref.probe_block()
    n = indptr.size - 1
    pos = np.concatenate([np.arange(L) for L in ref.PROBE_ROWS])
    rows = np.repeat(np.arange(n), ref.PROBE_ROWS)
    hot = np.zeros((n_ent, K, dh), dtype=np.float32)
    for k in range(K):
        hot[indices.astype(np.int64), k, pos % dh] = 1.0
    i, j = (indices, rows) if transposed else (rows, indices)
    keep = words(i, j, K, seed, stream) >= np.uint32(dropout_ref.params(0.5)[0])
    counts = np.zeros((n, K, dh), dtype=np.int64)
    for k in range(K):
        np.add.at(counts, (rows[keep[:, k]], k, (pos % dh)[keep[:, k]]), 1)
    L = np.array(ref.PROBE_ROWS, dtype=np.float64)
    lse = np.empty((n_ent, K), dtype=np.float32)
    lse[indices.astype(np.int64)] = np.log(L)[rows, None]
    return dict(indptr=indptr, indices=indices, n_ent=n_ent, hot=hot.reshape(n_ent, K * dh), keep=keep, counts=counts, L=L,
                lse=lse, drop=drop_tuple(0.5, seed, stream))


def all_dropped_seed(i, j, K, p, stream, start=0):
    """the first seed from ``start`` on under which entry (i, j) is dropped in every one of the K heads"""
    for seed in range(start, start + 100000):
        if not (words([i], [j], K, seed, stream) >= np.uint32(dropout_ref.params(p)[0])).any():
            return seed
    raise AssertionError("no such seed")


# ---- the reference model ---------------------------------------------------------------------------------------------------------------
class oracle_gat_dropout(ref.oracle_gat):
    """gat_ref.oracle_gat with both dropouts, as the device model applies them: in a training forward number e (counted
    from ``epoch``; backward uses the number its forward used) the input of every layer l >= 1 is dropout_ref.apply(H) with
    stream e * 64 + l, the gradient that layer returns goes through the same call, and every layer's attention -- layer 0's
    included -- is the twin of attention() above with the mask of the same stream number at ``attn_p``."""

    def __init__(self, oracle, A, sizes, heads, p=0.0, attn_p=0.0, seed=0, epoch=0, **kw):
        super().__init__(oracle, A, sizes, heads, **kw)
        self.p, self.attn_p, self.seed, self.epoch = float(p), float(attn_p), int(seed), int(epoch)
        self.current, self.training, self.dropped = int(epoch), False, False     # dropped: the last train_forward dropped
        self._keep = {}

    def _stream(self, li):
        return (self.current * 64 + li) & 0xFFFFFFFF

    def _mask(self, li, K):
        key = (self.current, li)
        if key not in self._keep:
            self._keep = {k: v for k, v in self._keep.items() if k[0] == self.current}
            self._keep[key] = keep_mask(self.indptr, self.indices, K, self.attn_p, self.seed, self._stream(li))
        return self._keep[key]

    def _attention(self, li, L, on, G=None):
        D = None if G is None else self._D(L, G)
        if on and self.attn_p > 0.0:
            return (restate64 if self.exact else twin32)(self.indptr, self.indices, L.Z, L.att, L.heads, self._mask(li, L.heads),
                                                         dropout_ref.params(self.attn_p)[1], G=G, slope=self.slope, D=D)
        return self._attend(self.indptr, self.indices, L.Z, L.att, L.heads, G=G, slope=self.slope, D=D)

    def forward(self, H):
        orc = self.orc
        H = np.ascontiguousarray(H, dtype=np.float32)
        for li, L in enumerate(self.layers):
            if self.training and self.p > 0.0 and li > 0:
                H = np.ascontiguousarray(dropout_ref.apply(H, 0, self.p, self.seed, self._stream(li)))
            L.Z = L.lin.forward(H)
            L.out = np.ascontiguousarray(self._attention(li, L, self.training)["out"])
            H = orc.leaky_relu_forward(L.out) if L.activation else L.out
        return H

    def train_forward(self, X, Y):
        self.current, self.training, self.dropped = self.epoch, True, True
        if self.p > 0.0 or self.attn_p > 0.0:
            self.epoch += 1
        try:
            return super().train_forward(X, Y)
        finally:
            self.training = False

    def backward(self):
        orc, G = self.orc, self.G
        for li in reversed(range(len(self.layers))):
            L = self.layers[li]
            T = orc.leaky_relu_backward(L.out, G) if L.activation else G
            r = self._attention(li, L, self.dropped, G=T)
            L.G_att = r["G_att"]
            G = L.lin.backward(np.ascontiguousarray(r["G_Z"]))
            if G is not None and self.dropped and self.p > 0.0 and li > 0:
                G = np.ascontiguousarray(dropout_ref.apply(G, 0, self.p, self.seed, self._stream(li)))
