"""The exported attention coefficients on the host, for the tests of mggcn_gat_alpha_f32 / mggcn_gatv2_alpha_f32 and of
gat.attention_weights: the cases, the measure, its bar, and the mutations the bar must tell apart.  Everything is built on
gat_ref.attention (v1) and gatv2_ref.attention_v2 (v2), which return ``alpha`` [nnz x K] already; only what those two have
no switch for -- the score of another entry's source and lrelu outside the dot product, for v2 -- is restated here
(alpha_v2), and test_gat_alpha_cpu.py holds that restatement against gatv2_ref's.

The measure.  For entry p and head k, with want = the fp64 restatement's alpha,
    dist = |got - want| / (want c_p),    v1: c_p = max(1, |x| + |lse|),    v2: c_p = max(1, sum_c |att_c lrelu(t_c)| + |lse|)
(x = s_dst[i, k] + s_src[j, k], every quantity from the fp64 restatement): alpha = exp(e - lse), so an absolute error d in
the exponent is a RELATIVE error d in alpha, and the exponent's error in fp32 is 2^-24 times the magnitudes that were
rounded on the way to it -- the terms of the score and lse.  An entry whose exact alpha is below 2^-100 is outside expf's
normal range and is compared absolutely instead (got <= 2^-99); that rule is a condition, not a measurement: no tolerance
case has such an entry (asserted on the CPU), only the stress cases use it.

The bar, by the project's rule (gat_ref.TWIN_ROW_MEASURED / ROW_TOL are the model): the fp32 twin's worst distance over
cases() -- gat_ref.twin32 / gatv2_ref.twin32, which compute their own scores and lse in fp32 -- measured on the CPU before any
device run, times 8, rounded up.  test_gat_alpha_cpu.py measures it again, prints it and asserts it."""
import numpy as np

import gat_ref as ref
import gatv2_ref as v2
from gat_ref import SLOPE, _segmax, _segsum

GRAPHS = ("long", "longT", "rect")          # gat_ref.edge_graphs(): "rect" is the 200 x 320 block, for v1 and v2 alike
# (K, dh): one per compiled (VEC, NT, U) variant of the v2 kernel -- (4,1,4), (1,1,4), (1,4,2), (4,4,1), (1,16,1) -- and for the
# v1 kernel K % 4 == 0 (16-byte stores) next to K = 3, 2, 1 (elements)
SHAPES = [(4, 32), (3, 7), (2, 65), (1, 260), (1, 257)]
TINY = 2.0 ** -100                          # below: the absolute rule
TINY_GOT = 2.0 ** -99

# The twin's worst distance over cases(), per variant, as test_gat_alpha_cpu.py measures it (it prints and asserts them): v1 at
# entry 7600, head 1 of ("long", 4, 32), v2 at entry 6379 of ("rect", 3, 7).  One bar for both: 8 x the larger, rounded up --
# about 30 units of 2^-24 c_p, far below gat_ref.ROW_TOL (8e-5), as a quantity without a sum over entries should be.
TWIN_MEASURED = dict(v1=2.15e-7, v2=1.90e-7)
BAR = 1.8e-6


def cases():
    return [(g, K, dh) for g in GRAPHS for K, dh in SHAPES]


def entry_rows(indptr):
    return np.repeat(np.arange(indptr.size - 1), np.diff(indptr.astype(np.int64)))


def dist(got, want, cp):
    """[nnz x K] of |got - want| / (want c_p); every want must be >= TINY (the caller masks the others)"""
    want = np.asarray(want, dtype=np.float64)
    return np.abs(np.asarray(got, dtype=np.float64).reshape(want.shape) - want) / (want * cp)


def worst(got, want, cp):
    """(distance, (entry, head)) of the worst entry"""
    q = dist(got, want, cp)
    if not q.size:
        return 0.0, (-1, -1)
    p = np.unravel_index(int(np.argmax(q)), q.shape)
    return float(q[p]), (int(p[0]), int(p[1]))


def check(got, want, cp):
    """the whole rule: (worst distance over the entries with want >= TINY, its place, the largest got among the others);
    asserts nothing"""
    want = np.asarray(want, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64).reshape(want.shape)
    big = want >= TINY
    q = np.where(big, np.abs(got - want) / (np.where(big, want, 1.0) * cp), 0.0)
    p = np.unravel_index(int(np.argmax(q)), q.shape) if q.size else (-1, -1)
    return (float(q[p]) if q.size else 0.0), (int(p[0]), int(p[1])), (float(got[~big].max()) if (~big).any() else 0.0)


def row_sums(indptr, alpha):
    return _segsum(np.asarray(alpha, dtype=np.float64), indptr)


# ---- v1 -------------------------------------------------------------------------------------------------------------------------------
def cp_v1(indptr, indices, s_dst, s_src, lse, score_cols=None):
    rows, cols = entry_rows(indptr), (indices if score_cols is None else score_cols).astype(np.int64)
    x = np.asarray(s_dst, dtype=np.float64)[rows] + np.asarray(s_src, dtype=np.float64)[cols]
    return np.maximum(1.0, np.abs(x) + np.abs(np.asarray(lse, dtype=np.float64)[rows]))


def alpha_v1(c, K, **kw):
    """gat_ref.attention's alpha of an edge_case / stress_case dict in fp64, with its keyword mutations (lse=, slope=,
    score_cols=, s_dst=, s_src=)"""
    return ref.attention(c["indptr"], c["indices"], c["Z"], c["att"], K, Z_dst=c.get("Z_dst"), dtype=np.float64, **kw)["alpha"]


_cases = {}


def case_v1(name, K, dh):
    """gat_ref.edge_case plus: ``alpha`` / ``cp`` of the exact restatement, the twin's alpha, and the injected form --
    ``s_dst32``, ``s_src32``, ``lse32`` (the restatement's, rounded to fp32) with ``alpha_inj`` / ``cp_inj``, the fp64 alpha
    of exactly those fp32 scalars"""
    key = ("v1", name, K, dh)
    if key not in _cases:
        c = dict(ref.edge_case(name, K, dh))
        w = c["want"]
        c["alpha"], c["twin_alpha"] = w["alpha"], c["twin"]["alpha"]
        c["cp"] = cp_v1(c["indptr"], c["indices"], w["s_dst"], w["s_src"], w["lse"])
        s32 = {k: w[k].astype(np.float32) for k in ("s_dst", "s_src", "lse")}
        c.update(s_dst32=s32["s_dst"], s_src32=s32["s_src"], lse32=s32["lse"])
        c["alpha_inj"] = alpha_v1(c, K, **s32)
        c["cp_inj"] = cp_v1(c["indptr"], c["indices"], **s32)
        _cases[key] = c
    return _cases[key]


def stress_v1(kind, K, dh):
    """gat_ref.stress_case with the restatement's lse rounded to fp32 and injected on both sides: s_dst = 0, s_src the
    stress scores (exact in fp32), ``alpha`` the fp64 coefficients of those scalars, ``cp`` their magnitudes"""
    key = ("v1 stress", kind, K, dh)
    if key not in _cases:
        c = dict(ref.stress_case(kind, K, dh))
        n = c["indptr"].size - 1
        c["Z_dst"] = np.zeros((n, K * dh), dtype=np.float32)
        c["s_dst32"], c["s_src32"] = np.zeros((n, K), dtype=np.float32), c["s_src"]
        c["lse32"] = c["want"]["lse"].astype(np.float32)
        kw = dict(s_dst=c["s_dst32"], s_src=c["s_src32"], lse=c["lse32"])
        c["alpha"] = alpha_v1(c, K, **kw)
        c["cp"] = cp_v1(c["indptr"], c["indices"], **kw)
        _cases[key] = c
    return _cases[key]


# ---- v2 -------------------------------------------------------------------------------------------------------------------------------
def alpha_v2(indptr, indices, Zs, Zd, att, K, slope=SLOPE, dtype=np.float64, lse=None, score_cols=None, outside=False):
    """gatv2_ref.attention_v2's forward restated with two more switches: dict(alpha, e, lse, mag) with mag[p, k] =
    sum_c |att_c lrelu(t_c)|.  ``score_cols``: the source whose head-row an entry's score is computed from; ``outside``: the
    GAT (v1) order, lrelu applied to the finished dot product att . t -- neither is the contract."""
    T = dtype
    n, n_src, d = indptr.size - 1, Zs.shape[0], Zs.shape[1]
    dh = d // K
    Zs3, Zd3 = np.asarray(Zs, dtype=T).reshape(n_src, K, dh), np.asarray(Zd, dtype=T).reshape(n, K, dh)
    a3 = np.asarray(att, dtype=T).reshape(1, K, dh)
    rows = entry_rows(indptr)
    cols = (indices if score_cols is None else score_cols).astype(np.int64)
    t = Zd3[rows] + Zs3[cols]
    u = np.where(t > 0, t, T(slope) * t)
    if outside:
        y = (t * a3).sum(axis=2, dtype=T)
        e = np.where(y > 0, y, T(slope) * y)
    else:
        e = (u * a3).sum(axis=2, dtype=T)
    mag = np.abs(u * a3).sum(axis=2)
    if lse is None:
        empty = np.diff(indptr.astype(np.int64)) == 0
        m = _segmax(e, indptr)
        m[empty] = 0
        ssum = _segsum(np.exp(e - m[rows]), indptr)
        ssum[empty] = 1
        lse = (m + np.log(ssum)).astype(T)
    else:
        lse = np.asarray(lse, dtype=T).reshape(n, K)
    return dict(alpha=np.exp(e - lse[rows]), e=e, lse=lse, mag=mag)


def cp_v2(indptr, mag, lse):
    return np.maximum(1.0, np.asarray(mag, dtype=np.float64) + np.abs(np.asarray(lse, dtype=np.float64)[entry_rows(indptr)]))


def _v2_args(c, K):
    return (c["indptr"], c["indices"], c["Zs"], c["Zd"], c["att"], K)


def case_v2(name, K, dh):
    """gatv2_ref.case plus ``alpha`` / ``cp`` of the exact restatement, the twin's alpha, and the injected form: ``lse32`` (the
    restatement's, rounded to fp32) with ``alpha_inj`` / ``cp_inj``"""
    key = ("v2", name, K, dh)
    if key not in _cases:
        c = dict(v2.case(name, K, dh))
        w = c["want"]
        r = alpha_v2(*_v2_args(c, K))
        c["alpha"], c["twin_alpha"], c["mag"] = w["alpha"], c["twin"]["alpha"], r["mag"]
        c["restated"] = r["alpha"]
        c["cp"] = cp_v2(c["indptr"], r["mag"], w["lse"])
        c["lse32"] = w["lse"].astype(np.float32)
        c["alpha_inj"] = v2.attention_v2(*_v2_args(c, K), lse=c["lse32"])["alpha"]
        c["cp_inj"] = cp_v2(c["indptr"], r["mag"], c["lse32"])
        _cases[key] = c
    return _cases[key]


def stress_v2(K, dh):
    """gatv2_ref.stress_case (scores exact in fp32, in the hundreds, slope 0.25) with the restatement's lse rounded to fp32
    and injected on both sides"""
    key = ("v2 stress", K, dh)
    if key not in _cases:
        c = dict(v2.stress_case(K, dh))
        c["lse32"] = c["want"]["lse"].astype(np.float32)
        r = alpha_v2(*_v2_args(c, K), slope=v2.STRESS_SLOPE, lse=c["lse32"])
        c["alpha"], c["cp"] = r["alpha"], cp_v2(c["indptr"], r["mag"], c["lse32"])
        _cases[key] = c
    return _cases[key]


# ---- the mutations the bar must tell apart --------------------------------------------------------------------------------------------
def previous_sources(indices):
    """score_cols: every entry takes the score of the entry before it in the indices array (the first: the last's)"""
    return np.roll(indices.astype(np.int64), 1)


def next_rows(lse):
    return np.roll(np.asarray(lse), -1, axis=0)


def mutations_v1(c, K):
    """name -> alpha [nnz x K] in fp64 of a wrong kernel on the inputs of case_v1"""
    lse = c["want"]["lse"]
    return {"lse of the next row": alpha_v1(c, K, lse=next_rows(lse)),
            "no leaky slope": alpha_v1(c, K, slope=1.0, lse=lse),
            "the previous entry's score": alpha_v1(c, K, score_cols=previous_sources(c["indices"]), lse=lse)}


def mutations_v2(c, K):
    lse, a = c["want"]["lse"], _v2_args(c, K)
    return {"lse of the next row": alpha_v2(*a, lse=next_rows(lse))["alpha"],
            "no leaky slope": alpha_v2(*a, slope=1.0, lse=lse)["alpha"],
            "the previous entry's score": alpha_v2(*a, score_cols=previous_sources(c["indices"]), lse=lse)["alpha"],
            "lrelu outside the dot product": alpha_v2(*a, outside=True, lse=lse)["alpha"]}


# ---- the reference models, layer by layer ------------------------------------------------------------------------------------------------
def model_alphas(O, X, variant):
    """[(alpha, cp)] per layer of a gat_ref.oracle_gat / gatv2_ref.oracle_gatv2 built with dtype=np.float64, after its plain
    forward of X: the fp64 coefficients of the layer's own (fp32) Z and att"""
    O.forward(X)
    res = []
    for L in O.layers:
        if variant == "v2":
            w = L.out_width
            r = alpha_v2(O.indptr, O.indices, np.ascontiguousarray(L.Z[:, :w]), np.ascontiguousarray(L.Z[:, w:]), L.att, L.heads,
                         slope=O.slope)
            res.append((r["alpha"], cp_v2(O.indptr, r["mag"], r["lse"])))
        else:
            r = ref.attention(O.indptr, O.indices, L.Z, L.att, L.heads, slope=O.slope, dtype=np.float64)
            res.append((r["alpha"], cp_v1(O.indptr, O.indices, r["s_dst"], r["s_src"], r["lse"])))
    return res
