"""Edge features in the GAT score on the host, for the gat(edge_attr=E) tests: the contract of the mggcn_gat_*_efeat_f32
entry points and their _drop twins (include/mggcn.h) restated in fp64 with an fp32 twin -- gat_ref.attention /
gat_dropout_ref.attention extended by E, U = att_edge, P_e and G_U --, the inputs and cases both test files share, the host
permutation between the two copies of E, the mutations the bar is held against, and the reference model.

F is a CSR pattern of n destinations x n_src sources, entry p = (i, j) of its indices array, E [nnz x de] in F's entry order,
U [K x de]:
    t_pk = sum_c E[p, c] U[k, c];  x = (s_dst[i, k] + s_src[j, k]) + t_pk;  e, lse, alpha, out, D, dalpha as in gat_ref
    ds = alpha (q dalpha - D[i, k]) lrelu'(x)  (q = 1 without dropout);  ds_dst, ds_src, G_Z, G_att as in gat_ref
    P_e[i, k de + c] = sum_j ds_ijk E[p, c];  G_U[k, c] = sum_i P_e[i, k de + c]
backward_src walks F^T with the OTHER copy of E, E_T = E[edge_perm(indices)]: ds_src and G_Z are restated from E_T here, so
that a copy in the wrong order is a different result (the mutation of test_gat_efeat_cpu.py)."""
import numpy as np

import dropout_ref
import gat_dropout_ref as dref
import gat_ref as ref
import gat_skip_ref
from gat_ref import _segmax, _segsum

NAMES = ("out", "lse", "D", "ds_dst", "P_e", "ds_src", "G_Z", "G_U")      # what the three entries and the column sum write


def edge_perm(indices):
    """perm with E[perm] in the entry order of the transposed pattern: mggcn_csr_transpose_host emits a transposed row in
    increasing source-row order, the stable order of the entries by column (gat_ref.transpose_pattern's)"""
    return np.argsort(np.asarray(indices), kind="stable")


def efeat_inputs(nnz, K, de, seed=41):
    """E = 0.5 x standard normal [nnz x de]; U = 0.2 / sqrt(de) x standard normal [K x de]: t has a deviation of about 0.1
    whatever de is, so the scores keep the spread gat_ref.tolerance_inputs gives them"""
    rng = np.random.default_rng(seed + 1000 * K + de)
    E = (0.5 * rng.standard_normal((nnz, de))).astype(np.float32)
    U = (0.2 / np.sqrt(de) * rng.standard_normal((K, de))).astype(np.float32)
    return E, U


def attention(indptr, indices, Z, att, K, E, U, keep=None, scale=1.0, G=None, Z_dst=None, slope=ref.SLOPE, dtype=np.float64,
              s_dst=None, s_src=None, lse=None, D=None, scales=False, E_T=None, head0_U=False, pe_without_q=False):
    """every quantity of NAMES (those of the backward pass when G is given) in ``dtype`` arithmetic, unrounded; ``keep`` /
    ``scale``: the mask of gat_dropout_ref (None: no dropout).  s_dst, s_src, lse and D replace the intermediates of the same
    name.  ``E_T``: the copy of E backward_src reads, in the transposed pattern's entry order (None: E[edge_perm]).  The
    mutations of the CPU tests: ``head0_U`` scores every head with U[0], ``pe_without_q`` forms P_e from a ds without q.
    With ``scales`` the result has "scale": per output the magnitude its terms add up to."""
    T = dtype
    n, n_src, d = indptr.size - 1, Z.shape[0], Z.shape[1]
    dh, de = d // K, E.shape[1]
    square = Z_dst is None
    Z3 = np.asarray(Z, dtype=T).reshape(n_src, K, dh)
    Zd3 = Z3 if square else np.asarray(Z_dst, dtype=T).reshape(n, K, dh)
    a3 = np.asarray(att, dtype=T).reshape(2, K, dh)
    E_, U_ = np.asarray(E, dtype=T), np.asarray(U, dtype=T).reshape(K, de)
    if head0_U:
        U_ = np.repeat(U_[:1], K, axis=0)
    rows = np.repeat(np.arange(n), np.diff(indptr.astype(np.int64)))
    cols = indices.astype(np.int64)
    q = np.ones((cols.size, K), dtype=T) if keep is None else np.where(np.asarray(keep, dtype=bool), T(scale), T(0)).astype(T)
    r = {}
    s_dst = (Zd3 * a3[0]).sum(axis=2, dtype=T) if s_dst is None else np.asarray(s_dst, dtype=T).reshape(n, K)
    s_src = (Z3 * a3[1]).sum(axis=2, dtype=T) if s_src is None else np.asarray(s_src, dtype=T).reshape(n_src, K)
    x0 = s_dst[rows] + s_src[cols]
    x = x0 + (E_ @ U_.T).astype(T)
    e = np.where(x > 0, x, T(slope) * x)
    if lse is None:
        m = _segmax(e, indptr)
        empty = np.diff(indptr.astype(np.int64)) == 0
        m[empty] = 0
        ssum = _segsum(np.exp(e - m[rows]), indptr)
        ssum[empty] = 1
        lse = (m + np.log(ssum)).astype(T)
    else:
        lse = np.asarray(lse, dtype=T).reshape(n, K)
    alpha = np.exp(e - lse[rows])
    aq = alpha * q
    out = _segsum(aq[:, :, None] * Z3[cols], indptr)
    r.update(s_dst=s_dst, s_src=s_src, out=out.reshape(n, d), lse=lse, alpha=alpha)
    if scales:
        sc = r["scale"] = dict(out=_segsum(aq[:, :, None] * np.abs(Z3)[cols], indptr).reshape(n, d), lse=np.maximum(np.abs(lse), 1))
    if G is None:
        return r
    G3 = np.asarray(G, dtype=T).reshape(n, K, dh)
    D = (G3 * out).sum(axis=2, dtype=T) if D is None else np.asarray(D, dtype=T).reshape(n, K)
    dalpha = (G3[rows] * Z3[cols]).sum(axis=2, dtype=T)
    lp = np.where(x > 0, T(1), T(slope))
    ds = alpha * (q * dalpha - D[rows]) * lp
    ds_dst = _segsum(ds, indptr)
    ds_pe = alpha * (dalpha - D[rows]) * lp if pe_without_q else ds
    P_e = _segsum(ds_pe[:, :, None] * E_[:, None, :], indptr)                    # [n x K x de]
    G_U = P_e.sum(axis=0, dtype=T)
    # the transposed walk, from the other copy of E
    order = edge_perm(cols)
    t_indptr = np.zeros(n_src + 1, dtype=np.int64)
    t_indptr[1:] = np.cumsum(np.bincount(cols, minlength=n_src))
    E_T = E_[order] if E_T is None else np.asarray(E_T, dtype=T)
    xT = x0[order] + (E_T @ U_.T).astype(T)
    alphaT = np.exp(np.where(xT > 0, xT, T(slope) * xT) - lse[rows[order]])
    lpT = np.where(xT > 0, T(1), T(slope))
    dsT = alphaT * (q[order] * dalpha[order] - D[rows[order]]) * lpT
    ds_src = _segsum(dsT, t_indptr)
    G_Z = _segsum(((alphaT * q[order])[:, :, None] * G3[rows[order]]), t_indptr)
    if square:
        G_Z = G_Z + ds_dst[:, :, None] * a3[0]
    G_Z = G_Z + ds_src[:, :, None] * a3[1]
    G_att = np.stack([(ds_dst[:, :, None] * Zd3).sum(axis=0, dtype=T), (ds_src[:, :, None] * Z3).sum(axis=0, dtype=T)])
    r.update(D=D, ds_dst=ds_dst, ds_src=ds_src, G_Z=G_Z.reshape(n_src, d), G_att=G_att.reshape(2, d),
             P_e=P_e.reshape(n, K * de), G_U=G_U.reshape(K, de))
    if scales:
        w = alpha * (q * np.abs(dalpha) + np.abs(D[rows])) * lp
        sd, ss = _segsum(w, indptr), _segsum(w[order], t_indptr)
        gz = _segsum((aq[:, :, None] * np.abs(G3[rows]))[order], t_indptr) + ss[:, :, None] * np.abs(a3[1])
        if square:
            gz = gz + sd[:, :, None] * np.abs(a3[0])
        # sum |ds| |E| with |ds| the magnitude ds's own two terms add up to, w -- what ds_dst and ds_src are measured by.  The
        # value |ds| itself will not do: in a row of one kept entry alpha = 1 and D = q dalpha, ds is EXACTLY 0 in fp64 and
        # rounding noise of size eps w in any fp32 evaluation, the twin's included, which would be at infinite distance.
        pe = _segsum(w[:, :, None] * np.abs(E_)[:, None, :], indptr)
        sc.update(D=np.abs(G3 * out).sum(axis=2), ds_dst=sd, ds_src=ss, G_Z=gz.reshape(n_src, d),
                  P_e=pe.reshape(n, K * de), G_U=pe.sum(axis=0).reshape(K, de))
    return r


def restate64(*a, exact=False, **kw):
    """the fp64 restatement: fp64 arithmetic on the fp32 inputs, rounded to fp32 at the end (exact: left in fp64)"""
    r = attention(*a, dtype=np.float64, **kw)
    return r if exact else {k: v.astype(np.float32) for k, v in r.items() if k != "scale"}


def twin32(*a, **kw):
    """the fp32 twin: the same formulas with every operation in fp32"""
    with np.errstate(over="ignore"):
        return {k: v.astype(np.float32) for k, v in attention(*a, dtype=np.float32, **kw).items()}


# ---- the device cases, measured on the CPU first ----------------------------------------------------------------------------------------
# (K, dh): the float4 path with full groups; one lane per group and four Philox blocks; the element path; NT > 1; the element
# path at NT = 16.  de: a scalar edge weight, odd 12-byte rows, 8, the limit -- the full cross at the first and the third
# shape, de = 8 elsewhere.
EFEAT_SHAPES = [(4, 32), (16, 4), (6, 7), (1, 260), (1, 257)]
EFEAT_DES = (1, 3, 8, 16)
EFEAT_CROSS = [(4, 32), (6, 7)]
EFEAT_PS = (None, 0.5, 0.9)                  # plain, and the _drop twins


def shape_des():
    return [(K, dh, de) for K, dh in EFEAT_SHAPES for de in (EFEAT_DES if (K, dh) in EFEAT_CROSS else (8,))]


def efeat_cases():
    """(graph name, K, dh, de, p): kernel_graph_long as F and transposed at every (shape, de), the 200 x 320 block (with
    non-zero dst0 / src0 under dropout) at the two cross shapes; each plain and at p = 0.5 and 0.9"""
    return ([(g, K, dh, de, p) for g in ("long", "longT") for K, dh, de in shape_des() for p in EFEAT_PS]
            + [("rect", K, dh, de, p) for K, dh in EFEAT_CROSS for de in EFEAT_DES for p in EFEAT_PS])


_cases = {}


def efeat_case(name, K, dh, de, p):
    """inputs (gat_ref.tolerance_inputs' and efeat_inputs'), the mask, the exact restatement with its row scales, and the twin;
    computed once per process"""
    key = (name, K, dh, de, p)
    if key not in _cases:
        indptr, indices, n_src = ref.edge_graphs()[name]
        n = indptr.size - 1
        Z, Z_dst, G, att = ref.tolerance_inputs(n, n_src, K, dh, att_scale=0.1 * min(1.0, (32.0 / dh) ** 0.5))
        Zd = None if n == n_src else Z_dst
        E, U = efeat_inputs(indices.size, K, de)
        perm = edge_perm(indices)
        kw, drop = {}, None
        if p is not None:
            dst0, src0 = dref.case_offsets(name)
            kw = dict(keep=dref.keep_mask(indptr, indices, K, p, dref.SEED, dref.STREAM, dst0, src0), scale=dropout_ref.params(p)[1])
            drop = dref.drop_tuple(p, dref.SEED, dref.STREAM, dst0, src0)
        want = restate64(indptr, indices, Z, att, K, E, U, G=G, Z_dst=Zd, exact=True, scales=True, **kw)
        twin = twin32(indptr, indices, Z, att, K, E, U, G=G, Z_dst=Zd, **kw)
        _cases[key] = dict(indptr=indptr, indices=indices, n_src=n_src, Z=Z, Z_dst=Zd, G=G, att=att, E=E, E_T=E[perm], U=U,
                           perm=perm, drop=drop, kw=kw, want=want, scale=want["scale"], twin=twin)
    return _cases[key]


def mode(p):
    return "plain" if p is None else "drop"


def bar_rule(twin_worst, floor):
    """the project's rule: where the twin's worst rowdist is within floor / 8 the bar is ``floor``; otherwise eight times the
    twin's worst, rounded up to two significant digits"""
    if twin_worst <= floor / 8:
        return floor
    x = 8 * twin_worst
    step = 10.0 ** (int(np.floor(np.log10(x))) - 1)
    return float(np.round(np.ceil(x / step - 1e-9) * step, 12))


# The bars of the efeat entry points on the row-scaled measure, per mode and output, fixed on the CPU before any device run.
# TWIN_EFEAT_MEASURED: the fp32 twin's worst rowdist from the exact restatement over efeat_cases() (test_gat_efeat_cpu.py
# prints it and asserts that the bars follow from it by bar_rule).  The floor is gat_ref.ROW_TOL for every output of both
# modes: the _drop twins' ds_dst, P_e, ds_src and G_Z get eight times THIS twin's worst (a dropped entry meets a D that nearly
# cancels, gat_dropout_ref says why), not the bars gat_dropout_ref derived from its own inputs.  P_e and G_U are measured against sum |ds| |E|, |ds| being the magnitude the
# two terms of ds add up to (attention() says why the value itself cannot be the yardstick).
TWIN_EFEAT_MEASURED = {
    "plain": dict(out=6.46e-7, lse=2.11e-7, D=1.06e-6, ds_dst=2.19e-6, P_e=2.55e-6, ds_src=1.47e-5, G_Z=1.34e-6, G_U=4.14e-8),
    "drop": dict(out=8.28e-7, lse=2.11e-7, D=7.67e-7, ds_dst=1.11e-4, P_e=6.66e-5, ds_src=2.99e-4, G_Z=5.36e-5, G_U=8.74e-8),
}
# plain ds_src: 1.47e-5 at ("longT", 4, 32, 8), a hair above ROW_TOL / 8, so its bar is 8 x that; the four drop bars likewise
EFEAT_TOL = {
    "plain": dict(out=ref.ROW_TOL, lse=ref.ROW_TOL, D=ref.ROW_TOL, ds_dst=ref.ROW_TOL, P_e=ref.ROW_TOL, ds_src=1.2e-4,
                  G_Z=ref.ROW_TOL, G_U=ref.ROW_TOL),
    "drop": dict(out=ref.ROW_TOL, lse=ref.ROW_TOL, D=ref.ROW_TOL, ds_dst=8.9e-4, P_e=5.4e-4, ds_src=2.4e-3, G_Z=4.3e-4,
                 G_U=ref.ROW_TOL),
}


def floor_of(md, name):
    """the bar an output has where the twin is within an eighth of it: gat_ref.ROW_TOL, for every output of both modes"""
    return ref.ROW_TOL


def distances(got, c):
    """{name: worst rowdist} of the outputs in ``got`` against the exact restatement of case ``c``; G_U is one row"""
    res = {}
    for name, v in got.items():
        want, scale = c["want"][name], c["scale"][name]
        if name == "G_U":
            want, scale, v = want.reshape(1, -1), scale.reshape(1, -1), np.asarray(v).reshape(1, -1)
        res[name] = ref.rowerr(v, want, scale)[1]
    return res


def fixed_order_colsum(P, max_blocks=512):
    """the column sums of P [rows x width] in fp32 in the order of the fixed-order reduction layer behind
    mggcn_gatv2_att_grad_f32 (csrc/gat_internal.h gat_column_sums, csrc/reduce.h colsum_final_kernel): tpr = the power of two
    covering the width (256 at the most) threads per row and R = 256 / tpr rows per workgroup and turn; a thread adds its
    rows blk R + rr, + grid R, ... in order, a workgroup its R slots in slot order, and the partials of the (at most
    ``max_blocks``) workgroups meet as four slices b, b + 4, ... added in order and combined as (w0 + w1) + (w2 + w3)"""
    P = np.ascontiguousarray(P, dtype=np.float32)
    n, width = P.shape
    tl = min(max(width - 1, 0).bit_length(), 8)
    R = 256 >> tl
    grid = min(-(-n // R), max_blocks)
    part = np.zeros((grid, width), dtype=np.float32)
    for blk in range(grid):
        s = None
        for rr in range(R):
            acc = np.zeros(width, dtype=np.float32)
            for r in range(blk * R + rr, n, grid * R):
                acc = acc + P[r]
            s = acc if s is None else s + acc
        part[blk] = s
    w = np.zeros((4, width), dtype=np.float32)
    for sl in range(4):
        for b in range(sl, grid, 4):
            w[sl] = w[sl] + part[b]
    return (w[0] + w[1]) + (w[2] + w[3])


# ---- the reference model ---------------------------------------------------------------------------------------------------------------
class oracle_gat_efeat(gat_skip_ref.oracle_gat_skip):
    """gat(edge_attr=E) on the host: gat_skip_ref.oracle_gat_skip (both dropouts, skip=, norm=) with the attention above.
    ``E`` is in A's entry order, as the model takes it; the forward walks A^T, so the layers read E[edge_perm(A.indices)].
    ``layers[i]`` gains att_edge (the engine's start: seed-99 uniform over a [de x heads] buffer), G_att_edge and the Adam
    state of att_edge, stepped by the chain of att."""

    def __init__(self, oracle, A, sizes, heads, E, edge_weights=None, **kw):
        super().__init__(oracle, A, sizes, heads, **kw)
        E = np.ascontiguousarray(E, dtype=np.float32)
        perm = edge_perm(A.indices[int(A.indptr[0]):int(A.indptr[-1])])
        rows = np.repeat(np.arange(A.indptr.size - 1, dtype=np.uint32), np.diff(A.indptr.astype(np.int64)))
        assert np.array_equal(rows[perm], self.indices), "the permutation does not line up with the oracle's transpose"
        self.E_F = np.ascontiguousarray(E[perm])
        de = E.shape[1]
        for i, L in enumerate(self.layers):
            L.att_edge = (oracle.init_uniform(de, L.heads).reshape(L.heads, de).copy() if edge_weights is None
                          else np.array(edge_weights[i], dtype=np.float32).reshape(L.heads, de))
            L.G_att_edge = np.zeros_like(L.att_edge)
            L.em = L.ev = None
            L.estep = 0

    def _attention(self, li, L, on, G=None):
        D = None if G is None else self._D(L, G)
        kw = {}
        if on and self.attn_p > 0.0:
            kw = dict(keep=self._mask(li, L.heads), scale=dropout_ref.params(self.attn_p)[1])
        return (restate64 if self.exact else twin32)(self.indptr, self.indices, L.Z, L.att, L.heads, self.E_F, L.att_edge, G=G,
                                                     slope=self.slope, D=D, **kw)

    def _attn_back(self, li, L, T):
        res = self._attention(li, L, self.dropped, G=T)
        L.G_att, L.G_att_edge = res["G_att"], res["G_U"]
        return np.ascontiguousarray(res["G_Z"])

    def adam_update(self, lr=ref.ADAM[0], beta1=ref.ADAM[1], beta2=ref.ADAM[2], weight_decay=ref.ADAM[3], eps=ref.ADAM[4]):
        super().adam_update(lr, beta1, beta2, weight_decay, eps)
        orc = self.orc
        lib, p, f = orc.lib(), orc._ptr, orc.f32p
        for L in self.layers:
            if L.em is None:
                L.em, L.ev, L.estep = np.zeros_like(L.att_edge), np.zeros_like(L.att_edge), 0
            L.estep += 1
            bc1, bc2 = np.float32(1 - beta1 ** L.estep), np.float32(1 - beta2 ** L.estep)
            U, GU = np.ascontiguousarray(L.att_edge, dtype=np.float32), np.ascontiguousarray(L.G_att_edge, dtype=np.float32)
            lib.orc_axpy(p(U, f), p(GU, f), weight_decay, U.size)                   # the chain of att
            lib.orc_axpby(p(GU, f), p(L.em, f), 1 - beta1, beta1, U.size)
            lib.orc_aaxpby(p(GU, f), p(L.ev, f), 1 - beta2, beta2, U.size)
            lib.orc_adam_final(p(U, f), p(L.em, f), p(L.ev, f), lr, bc1, bc2, eps, U.size)
            L.att_edge, L.G_att_edge = U, GU
