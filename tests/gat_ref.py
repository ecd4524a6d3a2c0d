"""Graph attention on the host, for the GAT tests: the contract of the mggcn_gat_* entry points (include/mggcn.h)
restated in fp64 with outputs rounded to fp32, an fp32 numpy twin that follows the same formulas (only the order of the
sums is numpy's), the kernel-test graph, and a reference model that composes the oracle's own linear, loss and Adam with
the restated attention without touching anything under oracle/.

F is a CSR pattern of n destinations x n_src sources; head k owns columns [k dh, (k + 1) dh):
    s_dst[i, k] = Z_dst[i, head k] . att[0, head k]      s_src[j, k] = Z[j, head k] . att[1, head k]
    x = s_dst[i, k] + s_src[j, k];  e = x > 0 ? x : slope x;  lse[i, k] = log sum_j exp(e)  (0 for a row without entries)
    alpha = exp(e - lse[i, k]);  out[i, head k] = sum_j alpha Z[j, head k]
    D[i, k] = G[i, head k] . out[i, head k];  dalpha = G[i, head k] . Z[j, head k]
    ds = alpha (dalpha - D[i, k]) (x > 0 ? 1 : slope);  ds_dst[i, k] = sum_j ds;  ds_src[j, k] = sum_i ds
    G_Z[j, head k] = sum_i alpha G[i, head k] + ds_dst[j, k] att[0, head k] + ds_src[j, k] att[1, head k]
    G_att[0] = sum_i ds_dst[i, k(c)] Z_dst[i, c];  G_att[1] = sum_j ds_src[j, k(c)] Z[j, c]
In the square case Z_dst is Z; a rectangular block has its own Z_dst and no ds_dst term in G_Z."""
import numpy as np

SLOPE = 0.2
ACT_SLOPE = 0.01
ADAM = (1e-2, 0.9, 0.999, 5e-4, 1e-8)
NAMES = ("s_dst", "s_src", "out", "lse", "D", "ds_dst", "ds_src", "G_Z", "G_att")


def relerr(got, want):
    """the matrix-normalised distance of test_gpu_gcn.py"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-30))


# ---- the kernel-test graph -------------------------------------------------------------------------------------------------------
SPECIAL_ROWS = {0: 0, 1: 1, 2: 64, 3: 65, 4: 1000, 5: 4097}
DUPLICATE_ROW = 6
UNREFERENCED = 7            # a column nobody gathers


def kernel_graph(n=320, n_src=320, seed=3):
    """(indptr, indices) of the n x n_src pattern: rows 0..5 of 0, 1, 64, 65, 1000 and 4097 entries, row 6 with one column
    twice, the last row empty, every other row of 1..11 entries; random columns, none of them UNREFERENCED"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 12, size=n)
    for r, l in SPECIAL_ROWS.items():
        lens[r] = l
    lens[DUPLICATE_ROW] = 3
    lens[n - 1] = 0
    allowed = np.array([c for c in range(n_src) if c != UNREFERENCED], dtype=np.uint32)
    indptr = np.zeros(n + 1, dtype=np.uint32)
    indptr[1:] = np.cumsum(lens)
    indices = allowed[rng.integers(0, allowed.size, size=int(indptr[-1]))]
    b = int(indptr[DUPLICATE_ROW])
    indices[b + 1] = indices[b]
    assert UNREFERENCED not in indices
    return indptr, np.ascontiguousarray(indices, dtype=np.uint32)


def transpose_pattern(indptr, indices, n_src):
    """CSR of the transposed pattern, entries of a row in increasing source-row order (mggcn_csr_transpose_host's)"""
    rows = np.repeat(np.arange(indptr.size - 1, dtype=np.uint32), np.diff(indptr.astype(np.int64)))
    order = np.argsort(indices, kind="stable")
    t_indptr = np.zeros(n_src + 1, dtype=np.uint32)
    t_indptr[1:] = np.cumsum(np.bincount(indices, minlength=n_src))
    return t_indptr, np.ascontiguousarray(rows[order], dtype=np.uint32)


def tolerance_inputs(n, n_src, K, dh, seed=11, att_scale=0.1):
    """Z, Z_dst (Z itself when square), G standard normal; att = att_scale x standard normal (|score| <~ 10 at 0.1)"""
    rng = np.random.default_rng(seed + 1000 * K + dh)
    d = K * dh
    Z = rng.standard_normal((n_src, d), dtype=np.float32)
    Z_dst = Z if n == n_src else rng.standard_normal((n, d), dtype=np.float32)
    G = rng.standard_normal((n, d), dtype=np.float32)
    att = (att_scale * rng.standard_normal((2, d))).astype(np.float32)
    return Z, Z_dst, G, att


# ---- the formulas, in one precision --------------------------------------------------------------------------------------------------
def _segsum(vals, indptr):
    """sums of consecutive segments of axis 0 (numpy's order), zeros for empty segments"""
    ip = np.asarray(indptr, dtype=np.int64)
    out = np.zeros((ip.size - 1,) + vals.shape[1:], dtype=vals.dtype)
    full = np.diff(ip) > 0
    if full.any():
        out[full] = np.add.reduceat(vals, ip[:-1][full], axis=0)
    return out


def _segmax(vals, indptr):
    ip = np.asarray(indptr, dtype=np.int64)
    out = np.full((ip.size - 1,) + vals.shape[1:], -np.inf, dtype=vals.dtype)
    full = np.diff(ip) > 0
    if full.any():
        out[full] = np.maximum.reduceat(vals, ip[:-1][full], axis=0)
    return out


def attention(indptr, indices, Z, att, K, G=None, Z_dst=None, slope=SLOPE, dtype=np.float64):
    """every quantity of NAMES (those of the backward pass when G is given) in ``dtype`` arithmetic, unrounded"""
    T = dtype
    n, n_src, d = indptr.size - 1, Z.shape[0], Z.shape[1]
    dh = d // K
    square = Z_dst is None
    Z3 = np.asarray(Z, dtype=T).reshape(n_src, K, dh)
    Zd3 = Z3 if square else np.asarray(Z_dst, dtype=T).reshape(n, K, dh)
    a3 = np.asarray(att, dtype=T).reshape(2, K, dh)
    rows = np.repeat(np.arange(n), np.diff(indptr.astype(np.int64)))
    cols = indices.astype(np.int64)
    r = {}
    s_dst = (Zd3 * a3[0]).sum(axis=2, dtype=T)
    s_src = (Z3 * a3[1]).sum(axis=2, dtype=T)
    x = s_dst[rows] + s_src[cols]
    e = np.where(x > 0, x, T(slope) * x)
    m = _segmax(e, indptr)
    empty = np.diff(indptr.astype(np.int64)) == 0
    m[empty] = 0
    ssum = _segsum(np.exp(e - m[rows]), indptr)
    ssum[empty] = 1
    lse = (m + np.log(ssum)).astype(T)
    alpha = np.exp(e - lse[rows])
    out = _segsum(alpha[:, :, None] * Z3[cols], indptr)
    r.update(s_dst=s_dst, s_src=s_src, out=out.reshape(n, d), lse=lse, alpha=alpha)
    if G is None:
        return r
    G3 = np.asarray(G, dtype=T).reshape(n, K, dh)
    D = (G3 * out).sum(axis=2, dtype=T)
    dalpha = (G3[rows] * Z3[cols]).sum(axis=2, dtype=T)
    ds = alpha * (dalpha - D[rows]) * np.where(x > 0, T(1), T(slope))
    ds_dst = _segsum(ds, indptr)
    order = np.argsort(cols, kind="stable")
    t_indptr = np.zeros(n_src + 1, dtype=np.int64)
    t_indptr[1:] = np.cumsum(np.bincount(cols, minlength=n_src))
    ds_src = _segsum(ds[order], t_indptr)
    G_Z = _segsum((alpha[:, :, None] * G3[rows])[order], t_indptr)
    if square:
        G_Z = G_Z + ds_dst[:, :, None] * a3[0]
    G_Z = G_Z + ds_src[:, :, None] * a3[1]
    G_att = np.stack([(ds_dst[:, :, None] * Zd3).sum(axis=0, dtype=T), (ds_src[:, :, None] * Z3).sum(axis=0, dtype=T)])
    r.update(D=D, ds_dst=ds_dst, ds_src=ds_src, G_Z=G_Z.reshape(n_src, d), G_att=G_att.reshape(2, d))
    return r


def restate64(*a, exact=False, **kw):
    """the fp64 restatement: fp64 arithmetic on the fp32 inputs, rounded to fp32 at the end (exact: left in fp64)"""
    r = attention(*a, dtype=np.float64, **kw)
    return r if exact else {k: v.astype(np.float32) for k, v in r.items()}


def twin32(*a, **kw):
    """the fp32 twin: the same formulas with every operation in fp32"""
    with np.errstate(over="ignore"):
        return {k: v.astype(np.float32) for k, v in attention(*a, dtype=np.float32, **kw).items()}


def row_mean(indptr, indices, Z):
    """the plain mean of Z over each row's entries (what the attention computes with att = 0), fp64; empty rows: 0"""
    cnt = np.diff(indptr.astype(np.int64)).astype(np.float64)
    s = _segsum(np.asarray(Z, dtype=np.float64)[indices.astype(np.int64)], indptr)
    return s / np.maximum(cnt, 1)[:, None]


# ---- the reference model ---------------------------------------------------------------------------------------------------------------
class oracle_gat:
    """The GAT model on the host: the oracle's Linear (forward, backward, Adam), leaky ReLU and softmax cross-entropy as they
    are, and the fp32 twin of the attention between them.  ``layers[i]`` has lin (oracle.Linear), att, G_att and the Adam
    state of att; att starts as the engine's (seed-99 uniform over an [out x 2] buffer) and is updated by the chain
    Linear.adam_update runs for W, with the oracle's own kernels.  ``loss``: None (the oracle's softmax cross-entropy over
    all rows) or a callable H -> (G, (loss, score)) -- the BCE and split tests pass theirs."""

    class _layer:
        pass

    def __init__(self, oracle, A, sizes, heads, slope=SLOPE, loss=None):
        self.orc, self.slope, self.loss = oracle, slope, loss
        F = oracle.transpose(A)                                 # the forward aggregates over A^T's rows, like oracle.Gcn
        self.indptr, self.indices = F.indptr.copy(), F.indices.copy()
        self.layers = []
        for i in range(1, len(sizes)):
            L = self._layer()
            L.lin = oracle.Linear(sizes[i - 1], sizes[i], i != 1)
            L.heads, L.activation = heads[i - 1], i + 1 < len(sizes)
            L.att = oracle.init_uniform(sizes[i], 2).reshape(2, sizes[i]).copy()
            L.G_att = np.zeros_like(L.att)
            L.m = L.v = None
            L.step = 0
            self.layers.append(L)

    def forward(self, H):
        orc = self.orc
        H = np.ascontiguousarray(H, dtype=np.float32)
        for L in self.layers:
            L.Z = L.lin.forward(H)
            L.out = np.ascontiguousarray(twin32(self.indptr, self.indices, L.Z, L.att, L.heads, slope=self.slope)["out"])
            H = orc.leaky_relu_forward(L.out) if L.activation else L.out
        return H

    def train_forward(self, X, Y):
        H = self.forward(X)
        if self.loss is not None:
            self.G, res = self.loss(H)
            return res
        ls, ac, self.G, _ = self.orc.softmax_cross_entropy(H, Y)
        n = np.float32(H.shape[0])
        return float(np.float32(ls) / n), float(np.float32(ac) / n)

    def backward(self):
        orc, G = self.orc, self.G
        for L in reversed(self.layers):
            T = orc.leaky_relu_backward(L.out, G) if L.activation else G
            r = twin32(self.indptr, self.indices, L.Z, L.att, L.heads, G=T, slope=self.slope)
            L.G_att = r["G_att"]
            G = L.lin.backward(np.ascontiguousarray(r["G_Z"]))

    def adam_update(self, lr=ADAM[0], beta1=ADAM[1], beta2=ADAM[2], weight_decay=ADAM[3], eps=ADAM[4]):
        orc = self.orc
        lib, p, f = orc.lib(), orc._ptr, orc.f32p
        for L in self.layers:
            L.lin.adam_update(lr, beta1, beta2, weight_decay, eps)
            if L.m is None:
                L.m, L.v, L.step = np.zeros_like(L.att), np.zeros_like(L.att), 0
            L.step += 1
            bc1, bc2 = np.float32(1 - beta1 ** L.step), np.float32(1 - beta2 ** L.step)
            L.att, L.G_att = np.ascontiguousarray(L.att), np.ascontiguousarray(L.G_att)
            lib.orc_axpy(p(L.att, f), p(L.G_att, f), weight_decay, L.att.size)          # the chain of W, gcn.hpp:146-172
            lib.orc_axpby(p(L.G_att, f), p(L.m, f), 1 - beta1, beta1, L.att.size)
            lib.orc_aaxpby(p(L.G_att, f), p(L.v, f), 1 - beta2, beta2, L.att.size)
            lib.orc_adam_final(p(L.att, f), p(L.m, f), p(L.v, f), lr, bc1, bc2, eps, L.att.size)
