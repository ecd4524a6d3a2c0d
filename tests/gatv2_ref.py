"""GATv2 (dynamic attention) on the host, for the GATv2 tests: the contract of the mggcn_gatv2_* entry points
(include/mggcn.h) restated in fp64, an fp32 numpy twin that follows the same formulas (only the order of the sums is
numpy's), the row scales of gat_ref.rowdist for every output, the shape list with the variant each shape reaches, the bar
per output, and a reference model that composes the oracle's own linear, loss and Adam with the twin.

F is a CSR pattern of n destinations x n_src sources; head k owns columns [k dh, (k + 1) dh); Zs has one row per source
(the row that gets aggregated), Zd one row per destination, att is [1 x K dh]:
    t_ijk[c] = Zd[i, k dh + c] + Zs[j, k dh + c]    u = t > 0 ? t : slope t    lrelu' = t > 0 ? 1 : slope
    e_ijk = sum_c att[k dh + c] u_ijk[c]           lse[i, k] = log sum_j exp(e_ijk)  (0 for a row without entries)
    alpha = exp(e - lse[i, k])                     out[i, head k] = sum_j alpha Zs[j, head k]
    D[i, k] = G[i, head k] . out[i, head k]        dalpha = G[i, head k] . Zs[j, head k]       ds = alpha (dalpha - D[i, k])
    v_ijk[c] = ds att[k dh + c] lrelu'(t_ijk[c])   G_Zd[i] = sum_j v      G_Zs[j] = sum_i (alpha G[i] + v)
    P[i, k dh + c] = sum_j ds u_ijk[c]             G_att = sum_i P[i]
"""
import numpy as np

import dropout_ref
import gat_ref as ref
from gat_ref import ADAM, ROW_TOL, SLOPE, _segmax, _segsum

NAMES = ("out", "lse", "D", "G_Zd", "P", "G_Zs", "G_att")


def attention_v2(indptr, indices, Zs, Zd, att, K, G=None, slope=SLOPE, dtype=np.float64, lse=None, D=None, scales=False,
                 vprime="t"):
    """every quantity of NAMES (those of the backward pass when G is given) in ``dtype`` arithmetic, unrounded, plus alpha
    and e [nnz x K].  ``lse`` and ``D`` replace the intermediates of the same name (backward_dst and backward_src read them
    as operands).  With ``scales`` the result has "scale": per output the magnitude its terms add up to (gat_ref.rowdist).
    ``vprime`` is a mutation for the CPU tests: "zs" takes lrelu' of Zs alone in v, which is NOT the contract."""
    T = dtype
    n, n_src, d = indptr.size - 1, Zs.shape[0], Zs.shape[1]
    dh = d // K
    assert Zd.shape == (n, d) and K * dh == d
    Zs3 = np.asarray(Zs, dtype=T).reshape(n_src, K, dh)
    Zd3 = np.asarray(Zd, dtype=T).reshape(n, K, dh)
    a3 = np.asarray(att, dtype=T).reshape(1, K, dh)
    rows = np.repeat(np.arange(n), np.diff(indptr.astype(np.int64)))
    cols = indices.astype(np.int64)
    empty = np.diff(indptr.astype(np.int64)) == 0
    t = Zd3[rows] + Zs3[cols]
    pos = t > 0
    u = np.where(pos, t, T(slope) * t)
    del t
    e = (u * a3).sum(axis=2, dtype=T)
    if lse is None:
        m = _segmax(e, indptr)
        m[empty] = 0
        ssum = _segsum(np.exp(e - m[rows]), indptr)
        ssum[empty] = 1
        lse = (m + np.log(ssum)).astype(T)
    else:
        lse = np.asarray(lse, dtype=T).reshape(n, K)
    alpha = np.exp(e - lse[rows])
    out = _segsum(alpha[:, :, None] * Zs3[cols], indptr)
    r = dict(out=out.reshape(n, d), lse=lse, alpha=alpha, e=e)
    if scales:
        sc = r["scale"] = dict(out=_segsum(alpha[:, :, None] * np.abs(Zs3)[cols], indptr).reshape(n, d),
                               lse=np.maximum(np.abs(lse), 1))
    if G is None:
        return r
    G3 = np.asarray(G, dtype=T).reshape(n, K, dh)
    D = (G3 * out).sum(axis=2, dtype=T) if D is None else np.asarray(D, dtype=T).reshape(n, K)
    dalpha = (G3[rows] * Zs3[cols]).sum(axis=2, dtype=T)
    ds = alpha * (dalpha - D[rows])
    dl = np.where(pos if vprime == "t" else Zs3[cols] > 0, T(1), T(slope))
    v = ds[:, :, None] * a3 * dl
    order = np.argsort(cols, kind="stable")
    t_indptr = np.zeros(n_src + 1, dtype=np.int64)
    t_indptr[1:] = np.cumsum(np.bincount(cols, minlength=n_src))
    G_Zd = _segsum(v, indptr)
    G_Zs = _segsum((alpha[:, :, None] * G3[rows] + v)[order], t_indptr)
    del v
    P = _segsum(ds[:, :, None] * u, indptr)
    G_att = (ds[:, :, None] * u).sum(axis=0, dtype=T)
    r.update(D=D, G_Zd=G_Zd.reshape(n, d), G_Zs=G_Zs.reshape(n_src, d), P=P.reshape(n, d), G_att=G_att.reshape(1, d))
    if scales:
        w = alpha * (np.abs(dalpha) + np.abs(D[rows]))
        vs = w[:, :, None] * np.abs(a3) * np.where(pos, T(1), T(slope))
        ps = w[:, :, None] * np.abs(u)
        sc.update(D=np.abs(G3 * out).sum(axis=2), G_Zd=_segsum(vs, indptr).reshape(n, d),
                  G_Zs=_segsum((alpha[:, :, None] * np.abs(G3[rows]) + vs)[order], t_indptr).reshape(n_src, d),
                  P=_segsum(ps, indptr).reshape(n, d), G_att=ps.sum(axis=0).reshape(1, d))
    return r


def restate64(*a, exact=False, **kw):
    """the fp64 restatement: fp64 arithmetic on the fp32 inputs, rounded to fp32 at the end (exact: left in fp64)"""
    r = attention_v2(*a, dtype=np.float64, **kw)
    return r if exact else {k: v.astype(np.float32) for k, v in r.items() if k != "scale"}


def twin32(*a, **kw):
    """the fp32 twin: the same formulas with every operation in fp32"""
    with np.errstate(over="ignore"):
        return {k: v.astype(np.float32) for k, v in attention_v2(*a, dtype=np.float32, **kw).items()}


# ---- shapes, inputs and cases ------------------------------------------------------------------------------------------------------------
# (K, dh): the variant on aligned operands (csrc/gat_internal.h: float4 path iff dh % 4 == 0); one per compiled (VEC, NT, U)
# plus the masked-tile cases
SHAPES = [
    (4, 32),        # (4,1,4)  nt 1: 8 lanes, all used
    (4, 12),        # (4,1,4)  nt 1: 3 of 4 lanes of a group
    (16, 4),        # (4,1,4)  nt 1: one lane per group, 64 groups, the most heads
    (1, 100),       # (4,1,4)  nt 1: 25 of 32 lanes
    (1, 260),       # (4,4,1)  nt 2: 65 float4 over 64 lanes, the second tile one lane wide
    (1, 1024),      # (4,4,1)  nt 4: the widest call, all tiles full
    (3, 7),         # (1,1,4)  nt 1: 7 of 8 lanes
    (2, 65),        # (1,4,2)  nt 2
    (1, 255),       # (1,4,2)  nt 4: the last tile one lane short
    (1, 257),       # (1,16,1) nt 5: the last tile one lane wide
]
RECT_SHAPES = [(4, 32), (1, 260), (3, 7), (2, 65), (1, 257)]        # one shape per variant on the 200 x 320 block
AUTOGRAD_SHAPES = [(4, 32), (3, 7), (1, 260), (16, 4), (2, 65)]      # where the formulas were checked against autograd


def inputs(n, n_src, K, dh, seed=11, att_scale=None):
    """Zs [n_src x d], Zd [n x d] and G [n x d] standard normal; att [1 x d] = att_scale x standard normal, by default
    0.1 sqrt(32 / dh) beyond dh = 32 (gat_ref.edge_case's rule: the scores keep the spread they have at dh = 32)"""
    rng = np.random.default_rng(seed + 1000 * K + dh)
    d = K * dh
    if att_scale is None:
        att_scale = 0.1 * min(1.0, (32.0 / dh) ** 0.5)
    Zs = rng.standard_normal((n_src, d), dtype=np.float32)
    Zd = rng.standard_normal((n, d), dtype=np.float32)
    G = rng.standard_normal((n, d), dtype=np.float32)
    att = (att_scale * rng.standard_normal((1, d))).astype(np.float32)
    return Zs, Zd, G, att


def cases():
    """(graph name, K, dh) of every case the bars are measured over and the device runs: gat_ref.edge_graphs()"""
    return [(g, K, dh) for g in ("long", "longT") for K, dh in SHAPES] + [("rect", K, dh) for K, dh in RECT_SHAPES]


_cases = {}


def case(name, K, dh):
    """inputs, the exact restatement with its row scales, and the twin of one case; computed once per process and left
    unchanged by everyone who reads it"""
    key = (name, K, dh)
    if key not in _cases:
        indptr, indices, n_src = ref.edge_graphs()[name]
        n = indptr.size - 1
        Zs, Zd, G, att = inputs(n, n_src, K, dh)
        want = restate64(indptr, indices, Zs, Zd, att, K, G=G, exact=True, scales=True)
        twin = twin32(indptr, indices, Zs, Zd, att, K, G=G)
        _cases[key] = dict(indptr=indptr, indices=indices, n=n, n_src=n_src, Zs=Zs, Zd=Zd, G=G, att=att, want=want,
                           scale=want["scale"], twin=twin)
    return _cases[key]


# The bar of every output on the row-scaled measure, fixed on the CPU before any device run (the project's rule):
# gat_ref.ROW_TOL where the fp32 twin's worst rowdist from the exact restatement over cases() stays within ROW_TOL / 8, eight
# times the twin's worst otherwise.  TWIN_MEASURED is what test_gatv2_cpu.py measures (it prints and asserts it); every
# output stays within ROW_TOL / 8 = 1e-5 (the worst is P at row 191 of ("long", 3, 7)), so every bar is ROW_TOL.
TWIN_MEASURED = dict(out=7.18e-7, lse=2.15e-7, D=6.56e-7, G_Zd=4.82e-6, P=8.50e-6, G_Zs=2.45e-6, G_att=4.49e-7)
BAR = dict.fromkeys(NAMES, ROW_TOL)


def bar_rule(twin_worst):
    return ROW_TOL if twin_worst <= ROW_TOL / 8 else 8 * twin_worst


# ---- the dynamic-attention probe -----------------------------------------------------------------------------------------------------------
def dynamic_probe():
    """K = 1, dh = 2, att = (1, -1), two destinations that both list the two sources: with f = lrelu at slope 0.2
        e_ij = f(Zd[i, 0] + Zs[j, 0]) - f(Zd[i, 1] + Zs[j, 1])
    Zs = [[2, 2], [0, 0]], Zd = [[1, -3], [-3, 1]]:
        e_00 = f(3) - f(-1) = 3.2    e_01 = f(1) - f(-3) = 1.6      destination 0 prefers source 0
        e_10 = f(-1) - f(3) = -3.2   e_11 = f(-3) - f(1) = -1.6     destination 1 prefers source 1
    The two destinations rank the sources in opposite orders, which no score of the form lrelu(s_dst[i] + s_src[j]) can do:
    that one is monotone in s_src[j] for every i.  Every score is a sum of two exactly representable terms."""
    indptr = np.array([0, 2, 4], dtype=np.uint32)
    indices = np.array([0, 1, 0, 1], dtype=np.uint32)
    Zs = np.array([[2.0, 2.0], [0.0, 0.0]], dtype=np.float32)
    Zd = np.array([[1.0, -3.0], [-3.0, 1.0]], dtype=np.float32)
    att = np.array([[1.0, -1.0]], dtype=np.float32)
    return indptr, indices, Zs, Zd, att


# ---- the position probe of the forward -------------------------------------------------------------------------------------------------------
def forward_probe_case(t, K, dh):
    """slot t of gat_ref.probe_hot on gat_ref.probe_block(): att is 1 in column 0 of every head and 0 elsewhere, Zd = 0, and
    column 0 of every head of Zs is 0 but 40 at the source at the probed position of each row -- every score is exactly 0 or
    40 in fp32, out[row] is that source's row of Zs and lse = 40 (the other weights add up to less than 4097 e^-40)"""
    indptr, indices, n_src = ref.probe_block()
    n, d = indptr.size - 1, K * dh
    Zs = np.random.default_rng(41 + 1000 * K + dh).standard_normal((n_src, d), dtype=np.float32)
    pos, hot = ref.probe_hot(t)
    Zs[:, ::dh] = 0.0
    Zs[hot[:, None], np.arange(0, d, dh)[None, :]] = 40.0
    att = np.zeros((1, d), dtype=np.float32)
    att[0, ::dh] = 1.0
    Zd = np.zeros((n, d), dtype=np.float32)
    want = restate64(indptr, indices, Zs, Zd, att, K, exact=True, scales=True)
    return dict(indptr=indptr, indices=indices, n=n, n_src=n_src, Zs=Zs, Zd=Zd, att=att, pos=pos, hot=hot, want=want)


STRESS_SLOPE = 0.25
STRESS_ATT = {(4, 32): 6, (3, 7): 16}              # (K, dh): att is drawn from the integers of [-a, a]


def stress_case(K, dh):
    """gat_ref.probe_block() with att scaled so that the scores reach the hundreds, and every score exact in fp32: Zs, Zd
    are integers of [-3, 3], att integers of [-a, a] with a = STRESS_ATT[(K, dh)], and the call's slope is 0.25, so every
    term att lrelu(t) is a multiple of 0.25 below 2^11 and their sum is exact in any order.  What the device's lse is held
    against is then the scores themselves (``e`` of the exact restatement), not the device's rounding of them; the scores
    stay below 256, where fp32 still resolves lse to 1.6e-5 / 2."""
    indptr, indices, n_src = ref.probe_block()
    n, d = indptr.size - 1, K * dh
    rng = np.random.default_rng(51 + 1000 * K + dh)
    a = STRESS_ATT[(K, dh)]
    Zs = rng.integers(-3, 4, size=(n_src, d)).astype(np.float32)
    Zd = rng.integers(-3, 4, size=(n, d)).astype(np.float32)
    G = rng.standard_normal((n, d), dtype=np.float32)
    att = rng.integers(-a, a + 1, size=(1, d)).astype(np.float32)
    want = restate64(indptr, indices, Zs, Zd, att, K, G=G, slope=STRESS_SLOPE, exact=True, scales=True)
    return dict(indptr=indptr, indices=indices, n=n, n_src=n_src, Zs=Zs, Zd=Zd, G=G, att=att, want=want)


def alpha_row_sums(indptr, e, lse):
    """sum_j alpha_ijk per (row, head) in fp64 from the exact scores e [nnz x K] and a given lse: 1 where lse is right"""
    rows = np.repeat(np.arange(indptr.size - 1), np.diff(indptr.astype(np.int64)))
    return _segsum(np.exp(np.asarray(e, dtype=np.float64) - np.asarray(lse, dtype=np.float64)[rows]), indptr)


# ---- the reference model ---------------------------------------------------------------------------------------------------------------------
class oracle_gatv2(ref.oracle_gat):
    """The GATv2 model on the host, built the way gat_ref.oracle_gat is: the oracle's Linear of 2 out columns (Z2 = [Zs | Zd],
    the bias inside both halves), leaky ReLU and loss as they are, and the fp32 twin of attention_v2 between them.  att [1 x
    out] starts as the engine's (seed-99 uniform over an [out x 1] buffer) and is updated by oracle_gat.adam_update, the chain
    of W.  Feature dropout as the device model applies it (gat_dropout_ref.oracle_gat_dropout's): in training forward number
    e (counted from ``epoch``) the input of every layer l >= 1 is dropout_ref.apply(H) with stream e * 64 + l, and the gradient
    that layer returns goes through the same call."""

    def __init__(self, oracle, A, sizes, heads, slope=SLOPE, loss=None, p=0.0, seed=0, epoch=0, dtype=np.float32):
        self.orc, self.slope, self.loss = oracle, slope, loss
        self._set_dtype(dtype)
        F = oracle.transpose(A)
        self.indptr, self.indices = F.indptr.copy(), F.indices.copy()
        self.layers = []
        for i in range(1, len(sizes)):
            L = self._layer()
            L.lin = oracle.Linear(sizes[i - 1], 2 * sizes[i], i != 1)
            L.out_width, L.heads, L.activation = sizes[i], heads[i - 1], i + 1 < len(sizes)
            L.att = oracle.init_uniform(sizes[i], 1).reshape(1, sizes[i]).copy()
            L.G_att = np.zeros_like(L.att)
            L.m = L.v = None
            L.step = 0
            self.layers.append(L)
        self.p, self.seed, self.epoch = float(p), int(seed), int(epoch)
        self.current, self.training, self.dropped = int(epoch), False, False

    def _stream(self, li):
        return (self.current * 64 + li) & 0xFFFFFFFF

    def _twin(self, L, G=None):
        w = L.out_width
        return (restate64 if self.exact else twin32)(self.indptr, self.indices, np.ascontiguousarray(L.Z[:, :w]),
                                                     np.ascontiguousarray(L.Z[:, w:]), L.att, L.heads, G=G, slope=self.slope,
                                                     D=None if G is None else self._D(L, G))

    def forward(self, H):
        orc = self.orc
        H = np.ascontiguousarray(H, dtype=np.float32)
        for li, L in enumerate(self.layers):
            if self.training and self.p > 0.0 and li > 0:
                H = np.ascontiguousarray(dropout_ref.apply(H, 0, self.p, self.seed, self._stream(li)))
            L.Z = L.lin.forward(H)
            L.out = np.ascontiguousarray(self._twin(L)["out"])
            H = orc.leaky_relu_forward(L.out) if L.activation else L.out
        return H

    def train_forward(self, X, Y):
        self.current, self.training, self.dropped = self.epoch, True, True
        if self.p > 0.0:
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
            r = self._twin(L, G=T)
            L.G_att = r["G_att"]
            G = L.lin.backward(np.ascontiguousarray(np.concatenate([r["G_Zs"], r["G_Zd"]], axis=1)))
            if G is not None and self.dropped and self.p > 0.0 and li > 0:
                G = np.ascontiguousarray(dropout_ref.apply(G, 0, self.p, self.seed, self._stream(li)))
