"""Dot-product (transformer) attention on the host, for the gatdot tests: the contract of the mggcn_gatdot_* entry points
(include/mggcn.h) restated in fp64, an fp32 numpy twin that follows the same formulas (only the order of the sums is
numpy's), the row scales of gat_ref.rowdist for every output, the shape list with the variant each shape reaches, the bar
per output, and a reference model that composes the oracle's own linear, loss and Adam with the twin.

F is a CSR pattern of n destinations x n_src sources; head k owns columns [k dh, (k + 1) dh); Zq has one row per
destination, Zk and Zv one row per source; c = fp32(1 / sqrt(dh)) unless ``scale`` says otherwise:
    e_ijk = c (Zq[i, head k] . Zk[j, head k])      lse[i, k] = log sum_j exp(e_ijk)  (0 for a row without entries)
    alpha = exp(e - lse[i, k])                     out[i, head k] = sum_j alpha Zv[j, head k]
    D[i, k] = G[i, head k] . out[i, head k]        dalpha = G[i, head k] . Zv[j, head k]       ds = alpha (dalpha - D[i, k])
    G_Zq[i, head k] = c sum_j ds Zk[j, head k]     G_Zk[j, head k] = c sum_i ds Zq[i, head k]  G_Zv[j, head k] = sum_i alpha G[i, head k]
"""
import numpy as np

import dropout_ref
import gat_ref as ref
import gatv2_ref as v2
from gat_ref import ROW_TOL, _segmax, _segsum

NAMES = ("out", "lse", "D", "G_Zq", "G_Zk", "G_Zv")
MUTATIONS = {"no c": "G_Zq", "G_Zk from Zk": "G_Zk", "no D": "G_Zq"}     # mutation -> an output it spoils


def default_scale(dh):
    """c = fp32(1 / sqrt(dh)), the model's"""
    return np.float32(1 / np.sqrt(dh))


def attention_dot(indptr, indices, Zq, Zk, Zv, K, G=None, scale=None, dtype=np.float64, lse=None, D=None, scales=False,
                  mutate=None):
    """every quantity of NAMES (those of the backward pass when G is given) in ``dtype`` arithmetic, unrounded, plus alpha
    and e [nnz x K].  ``lse`` and ``D`` replace the intermediates of the same name (backward_dst and backward_src read them
    as operands).  With ``scales`` the result has "scale": per output the magnitude its terms add up to (gat_ref.rowdist).
    ``mutate`` is one of MUTATIONS, for the CPU tests: "no c" leaves the factor c out of the scores, "G_Zk from Zk"
    accumulates G_Zk from the source's own key where the contract has the destination's query, "no D" leaves D out of ds --
    none of them is the contract."""
    T = dtype
    assert mutate is None or mutate in MUTATIONS
    n, n_src, d = indptr.size - 1, Zk.shape[0], Zk.shape[1]
    dh = d // K
    assert Zq.shape == (n, d) and Zv.shape == (n_src, d) and K * dh == d
    c = T(default_scale(dh) if scale is None else np.float32(scale))
    ce = T(1) if mutate == "no c" else c
    Zq3 = np.asarray(Zq, dtype=T).reshape(n, K, dh)
    Zk3 = np.asarray(Zk, dtype=T).reshape(n_src, K, dh)
    Zv3 = np.asarray(Zv, dtype=T).reshape(n_src, K, dh)
    rows = np.repeat(np.arange(n), np.diff(indptr.astype(np.int64)))
    cols = indices.astype(np.int64)
    empty = np.diff(indptr.astype(np.int64)) == 0
    e = ce * (Zq3[rows] * Zk3[cols]).sum(axis=2, dtype=T)
    if lse is None:
        m = _segmax(e, indptr)
        m[empty] = 0
        ssum = _segsum(np.exp(e - m[rows]), indptr)
        ssum[empty] = 1
        lse = (m + np.log(ssum)).astype(T)
    else:
        lse = np.asarray(lse, dtype=T).reshape(n, K)
    alpha = np.exp(e - lse[rows])
    out = _segsum(alpha[:, :, None] * Zv3[cols], indptr)
    r = dict(out=out.reshape(n, d), lse=lse, alpha=alpha, e=e)
    if scales:
        sc = r["scale"] = dict(out=_segsum(alpha[:, :, None] * np.abs(Zv3)[cols], indptr).reshape(n, d),
                               lse=np.maximum(np.abs(lse), 1))
    if G is None:
        return r
    G3 = np.asarray(G, dtype=T).reshape(n, K, dh)
    D = (G3 * out).sum(axis=2, dtype=T) if D is None else np.asarray(D, dtype=T).reshape(n, K)
    dalpha = (G3[rows] * Zv3[cols]).sum(axis=2, dtype=T)
    ds = alpha * (dalpha if mutate == "no D" else dalpha - D[rows])
    order = np.argsort(cols, kind="stable")
    t_indptr = np.zeros(n_src + 1, dtype=np.int64)
    t_indptr[1:] = np.cumsum(np.bincount(cols, minlength=n_src))
    G_Zq = ce * _segsum(ds[:, :, None] * Zk3[cols], indptr)
    other = Zk3[cols] if mutate == "G_Zk from Zk" else Zq3[rows]
    G_Zk = ce * _segsum((ds[:, :, None] * other)[order], t_indptr)
    G_Zv = _segsum((alpha[:, :, None] * G3[rows])[order], t_indptr)
    r.update(D=D, G_Zq=G_Zq.reshape(n, d), G_Zk=G_Zk.reshape(n_src, d), G_Zv=G_Zv.reshape(n_src, d))
    if scales:
        w = alpha * (np.abs(dalpha) + np.abs(D[rows]))
        sc.update(D=np.abs(G3 * out).sum(axis=2),
                  G_Zq=(np.abs(c) * _segsum(w[:, :, None] * np.abs(Zk3)[cols], indptr)).reshape(n, d),
                  G_Zk=(np.abs(c) * _segsum((w[:, :, None] * np.abs(Zq3)[rows])[order], t_indptr)).reshape(n_src, d),
                  G_Zv=_segsum((alpha[:, :, None] * np.abs(G3)[rows])[order], t_indptr).reshape(n_src, d))
    return r


def restate64(*a, exact=False, **kw):
    """the fp64 restatement: fp64 arithmetic on the fp32 inputs, rounded to fp32 at the end (exact: left in fp64)"""
    r = attention_dot(*a, dtype=np.float64, **kw)
    return r if exact else {k: v.astype(np.float32) for k, v in r.items() if k != "scale"}


def twin32(*a, **kw):
    """the fp32 twin: the same formulas with every operation in fp32"""
    with np.errstate(over="ignore"):
        return {k: v.astype(np.float32) for k, v in attention_dot(*a, dtype=np.float32, **kw).items()}


# ---- shapes, inputs and cases ------------------------------------------------------------------------------------------------------------
# gatv2_ref's lists as they are: one shape per compiled (VEC, NT, U) plus the masked-tile cases, 16 heads and the widest call
SHAPES = v2.SHAPES
RECT_SHAPES = v2.RECT_SHAPES
AUTOGRAD_SHAPES = [(4, 32), (3, 7), (1, 260), (16, 4), (2, 65)]


def inputs(n, n_src, K, dh, seed=17):
    """Zq, G [n x d] and Zk, Zv [n_src x d] standard normal: c = 1 / sqrt(dh) keeps the scores at unit spread for every dh"""
    rng = np.random.default_rng(seed + 1000 * K + dh)
    d = K * dh
    Zq = rng.standard_normal((n, d), dtype=np.float32)
    Zk = rng.standard_normal((n_src, d), dtype=np.float32)
    Zv = rng.standard_normal((n_src, d), dtype=np.float32)
    G = rng.standard_normal((n, d), dtype=np.float32)
    return Zq, Zk, Zv, G


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
        Zq, Zk, Zv, G = inputs(n, n_src, K, dh)
        want = restate64(indptr, indices, Zq, Zk, Zv, K, G=G, exact=True, scales=True)
        twin = twin32(indptr, indices, Zq, Zk, Zv, K, G=G)
        _cases[key] = dict(indptr=indptr, indices=indices, n=n, n_src=n_src, Zq=Zq, Zk=Zk, Zv=Zv, G=G, want=want,
                           scale=want["scale"], twin=twin)
    return _cases[key]


# The bar of every output on the row-scaled measure, fixed on the CPU before any device run (the project's rule):
# gat_ref.ROW_TOL where the fp32 twin's worst rowdist from the exact restatement over cases() stays within ROW_TOL / 8, eight
# times the twin's worst otherwise.  TWIN_MEASURED is what test_gatdot_cpu.py measures (it prints and asserts it); every
# output stays within ROW_TOL / 8 = 1e-5 (the worst is G_Zq at row 176 of ("long", 2, 65)), so every bar is ROW_TOL.
TWIN_MEASURED = dict(out=8.60e-7, lse=2.88e-7, D=1.46e-6, G_Zq=4.59e-6, G_Zk=3.02e-6, G_Zv=1.02e-6)
BAR = dict.fromkeys(NAMES, ROW_TOL)


def bar_rule(twin_worst):
    return ROW_TOL if twin_worst <= ROW_TOL / 8 else 8 * twin_worst


# ---- the two-destination known answer -----------------------------------------------------------------------------------------------------
def dynamic_probe():
    """K = 1, dh = 4 (c = 1/2), two destinations that both list the two sources:
        Zq = [[2, 0, 0, 0], [0, 2, 0, 0]]     Zk = [[3, 1, 0, 0], [1, 3, 0, 0]]     Zv = [[1, 0, 0, 0], [0, 1, 0, 0]]
        e_00 = 3   e_01 = 1      destination 0 prefers source 0: alpha_00 = 1 / (1 + e^-2)
        e_10 = 1   e_11 = 3      destination 1 prefers source 1
    The two destinations rank the sources in opposite orders (no v1 score can), every score is exact, and out[i] holds the
    two coefficients of destination i in its first two columns."""
    indptr = np.array([0, 2, 4], dtype=np.uint32)
    indices = np.array([0, 1, 0, 1], dtype=np.uint32)
    Zq = np.array([[2.0, 0, 0, 0], [0, 2.0, 0, 0]], dtype=np.float32)
    Zk = np.array([[3.0, 1.0, 0, 0], [1.0, 3.0, 0, 0]], dtype=np.float32)
    Zv = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0]], dtype=np.float32)
    return indptr, indices, Zq, Zk, Zv


# ---- the position probe of the forward -------------------------------------------------------------------------------------------------------
PROBE_SCALE = 0.5


def forward_probe_case(t, K, dh):
    """slot t of gat_ref.probe_hot on gat_ref.probe_block(), called with scale = 1/2: Zq is 1 in column 0 of every head and
    0 elsewhere, and column 0 of every head of Zk is 0 but 80 at the source at the probed position of each row (its other
    columns are noise that the zeros of Zq cancel) -- every score is exactly 0 or 40 in fp32, out[row] is that source's row of
    Zv and lse = 40 (the other weights add up to less than 4097 e^-40)"""
    indptr, indices, n_src = ref.probe_block()
    n, d = indptr.size - 1, K * dh
    rng = np.random.default_rng(43 + 1000 * K + dh)
    Zk = rng.standard_normal((n_src, d), dtype=np.float32)
    Zv = rng.standard_normal((n_src, d), dtype=np.float32)
    pos, hot = ref.probe_hot(t)
    Zk[:, ::dh] = 0.0
    Zk[hot[:, None], np.arange(0, d, dh)[None, :]] = 80.0
    Zq = np.zeros((n, d), dtype=np.float32)
    Zq[:, ::dh] = 1.0
    want = restate64(indptr, indices, Zq, Zk, Zv, K, scale=PROBE_SCALE, exact=True, scales=True)
    return dict(indptr=indptr, indices=indices, n=n, n_src=n_src, Zq=Zq, Zk=Zk, Zv=Zv, pos=pos, hot=hot, want=want)


# ---- scores in the hundreds ------------------------------------------------------------------------------------------------------------------
STRESS_SHAPES = [(4, 16), (1, 64)]               # dh a power of 4: c = 1/4 and 1/8, powers of two


def stress_case(K, dh):
    """gat_ref.probe_block() with integer Zq and Zk of [-a, a]: every product is an integer, every partial sum stays below
    2^24 and c is a power of two, so every score is exact in fp32 in any order of summation.  a is the smallest range at
    which the largest |e| of the case reaches 100 (it then lies in [100, 256): asserted by the tests).  Zv and G are
    standard normal."""
    key = ("stress", K, dh)
    if key in _cases:
        return _cases[key]
    assert 4 ** round(np.log(dh) / np.log(4)) == dh
    indptr, indices, n_src = ref.probe_block()
    n, d = indptr.size - 1, K * dh
    for a in range(1, 64):
        rng = np.random.default_rng(53 + 1000 * K + dh)
        Zq = rng.integers(-a, a + 1, size=(n, d)).astype(np.float32)
        Zk = rng.integers(-a, a + 1, size=(n_src, d)).astype(np.float32)
        Zv = rng.standard_normal((n_src, d), dtype=np.float32)
        G = rng.standard_normal((n, d), dtype=np.float32)
        want = restate64(indptr, indices, Zq, Zk, Zv, K, G=G, exact=True, scales=True)
        if np.abs(want["e"]).max() >= 100:
            break
    _cases[key] = dict(indptr=indptr, indices=indices, n=n, n_src=n_src, Zq=Zq, Zk=Zk, Zv=Zv, G=G, a=a, want=want,
                       scale=want["scale"])
    return _cases[key]


alpha_row_sums = v2.alpha_row_sums


# ---- the reference model ---------------------------------------------------------------------------------------------------------------------
class oracle_gatdot(v2.oracle_gatv2):
    """The dot-product attention model on the host, built the way gatv2_ref.oracle_gatv2 (a gat_ref.oracle_gat) is: the
    oracle's Linear of 3 out columns (Z3 = [Zq | Zk | Zv], the bias inside all three thirds), leaky ReLU and loss as they
    are, and the fp32 twin of attention_dot between them; no attention parameter, so Adam updates the linears alone.
    Feature dropout as oracle_gatv2 applies it (forward and train_forward are its own)."""

    def __init__(self, oracle, A, sizes, heads, loss=None, p=0.0, seed=0, epoch=0, dtype=np.float32):
        self.orc, self.loss = oracle, loss
        self._set_dtype(dtype)
        F = oracle.transpose(A)
        self.indptr, self.indices = F.indptr.copy(), F.indices.copy()
        self.layers = []
        for i in range(1, len(sizes)):
            L = self._layer()
            L.lin = oracle.Linear(sizes[i - 1], 3 * sizes[i], i != 1)
            L.out_width, L.heads, L.activation = sizes[i], heads[i - 1], i + 1 < len(sizes)
            self.layers.append(L)
        self.p, self.seed, self.epoch = float(p), int(seed), int(epoch)
        self.current, self.training, self.dropped = int(epoch), False, False

    def _twin(self, L, G=None):
        w = L.out_width
        Zq, Zk, Zv = (np.ascontiguousarray(L.Z[:, t * w:(t + 1) * w]) for t in range(3))
        return (restate64 if self.exact else twin32)(self.indptr, self.indices, Zq, Zk, Zv, L.heads, G=G,
                                                     D=None if G is None else self._D(L, G))

    def backward(self):
        orc, G = self.orc, self.G
        for li in reversed(range(len(self.layers))):
            L = self.layers[li]
            T = orc.leaky_relu_backward(L.out, G) if L.activation else G
            r = self._twin(L, G=T)
            G = L.lin.backward(np.ascontiguousarray(np.concatenate([r["G_Zq"], r["G_Zk"], r["G_Zv"]], axis=1)))
            if G is not None and self.dropped and self.p > 0.0 and li > 0:
                G = np.ascontiguousarray(dropout_ref.apply(G, 0, self.p, self.seed, self._stream(li)))

    def adam_update(self, lr=ref.ADAM[0], beta1=ref.ADAM[1], beta2=ref.ADAM[2], weight_decay=ref.ADAM[3], eps=ref.ADAM[4]):
        for L in self.layers:
            L.lin.adam_update(lr, beta1, beta2, weight_decay, eps)
