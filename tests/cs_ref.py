"""Correct and Smooth on the host (mg-gcn_amd/smoothing.py, csrc/propagate.hip): the numpy restatement in fp64 and its fp32
twin, which evaluates the kernels' stated expressions (include/mggcn.h) with the SpMM as a row-ordered fp32 sum.  Both
take the factors the kernels get: fp32(alpha) and fp32(1 - alpha), the subtraction in double (``factors``).

Every function takes ``dtype``: np.float64 computes in double throughout (the reference); np.float32 rounds where the
kernels round (the twin).  ``planted_case`` and ``model_case`` build the inputs the CPU and the GPU tests share, and
``pipeline`` results are cached per case: a reference is computed once and never modified."""
import functools

import numpy as np

INF = float("inf")
SCALE_LIMIT = 1000.0


def factors(alpha):
    """(alpha, beta) as the step kernel receives them, as doubles holding fp32 values"""
    return float(np.float32(alpha)), float(np.float32(1.0 - float(alpha)))


def onehot(Y, m, dtype):
    y = np.asarray(Y).reshape(-1)
    out = np.zeros((y.size, m), dtype=dtype)
    ok = (y >= 0) & (y < m)
    out[np.flatnonzero(ok), y[ok]] = 1
    return out


def residual(logits, Y, S, train_set, dtype=np.float64):
    """steps 1-2: P = softmax(logits) (max-subtracted, e / sum), E0 = onehot - P on the training rows and +0.0 elsewhere,
    and the sum of |E0| (fp32 twin: a plain fp32 sum, rows in order)"""
    x = np.asarray(logits, dtype=np.float32).astype(dtype)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    s = e[:, :1].copy()
    for c in range(1, e.shape[1]):                      # column order, in dtype
        s = s + e[:, c:c + 1]
    P = e / s
    train = np.asarray(S).reshape(-1) == train_set
    E0 = np.where(train[:, None], onehot(Y, x.shape[1], dtype) - P, dtype(0))
    total = dtype(0)
    for r in np.abs(E0).sum(axis=1, dtype=dtype):
        total = dtype(total + r)
    return P, E0, total


def spmm(indptr, indices, data, X, dtype=np.float64):
    """A X; fp32 twin: every row's entries in storage order, the product rounded, then added (no fma)"""
    ip = np.asarray(indptr).astype(np.int64)
    ix = np.asarray(indices).astype(np.int64)
    a = np.asarray(data, dtype=np.float32).astype(dtype)
    X = np.asarray(X, dtype=dtype)
    deg = np.diff(ip)
    out = np.zeros((deg.size, X.shape[1]), dtype=dtype)
    for k in range(int(deg.max()) if deg.size else 0):
        rows = np.flatnonzero(deg > k)
        e = ip[rows] + k
        out[rows] = out[rows] + a[e, None] * X[ix[e]]
    return out


def step(T, R, S, alpha, beta, lo, hi, train_set=0, fix=False, dtype=np.float64):
    """out = min(max(fmaf(alpha, T, beta * R), lo), hi), max(v, lo) = v < lo ? lo : v, min(v, hi) = v > hi ? hi : v; with
    ``fix`` a training row is R's.  alpha and beta hold fp32 values.  The twin takes fp32 operands: beta * R is exact in
    double and rounds once; alpha * T is exact in double, the sum rounds in double and then to fp32 -- bit-exact where the
    double sum is exact (operands of few significant bits), within one ulp otherwise."""
    T64, R64 = np.asarray(T, dtype=dtype).astype(np.float64), np.asarray(R, dtype=dtype).astype(np.float64)
    if dtype == np.float32:
        br = (np.float64(np.float32(beta)) * R64).astype(np.float32).astype(np.float64)
        v = (np.float64(np.float32(alpha)) * T64 + br).astype(np.float32)
    else:
        v = alpha * T64 + beta * R64
    lo, hi = dtype(lo), dtype(hi)
    v = np.where(v < lo, lo, v)
    v = np.where(v > hi, hi, v).astype(dtype)
    if fix:
        train = np.asarray(S).reshape(-1) == train_set
        v = np.where(train[:, None], np.asarray(R, dtype=dtype), v)
    return v


def propagate(indptr, indices, data, R, layers, alpha, beta, lo, hi, S=None, train_set=0, fix=False, dtype=np.float64):
    """X <- R, then ``layers`` times X <- post(alpha (A X) + beta R)"""
    X = np.asarray(R, dtype=dtype)
    for _ in range(layers):
        X = step(spmm(indptr, indices, data, X, dtype), R, S, alpha, beta, lo, hi, train_set, fix, dtype)
    return X


def row_scale(E, total, inv_T, dtype=np.float64):
    """(s_i, the raw quotient sigma / l1_i) of the autoscale rule: s = 1 where the quotient is not finite or above 1000"""
    E = np.asarray(E, dtype=dtype)
    l1 = np.zeros(E.shape[0], dtype=dtype)
    for c in range(E.shape[1]):
        l1 = l1 + np.abs(E[:, c])
    sigma = dtype(dtype(total) * dtype(inv_T))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = sigma / l1
    return np.where(np.abs(q) <= SCALE_LIMIT, q, dtype(1)).astype(dtype), q


def correct(P, E, Y, S, train_set, total, inv_T, scale, autoscale, set_labels, dtype=np.float64):
    """step 4 (and G0 of step 5 with ``set_labels``): out = fmaf(s, E, P).  Returns (out, s)"""
    P, E = np.asarray(P, dtype=dtype), np.asarray(E, dtype=dtype)
    s = row_scale(E, total, inv_T, dtype)[0] if autoscale else np.full(P.shape[0], scale, dtype=dtype)
    out = (s[:, None].astype(np.float64) * E.astype(np.float64) + P.astype(np.float64)).astype(dtype)   # one rounding
    if set_labels:
        train = np.asarray(S).reshape(-1) == train_set
        out = np.where(train[:, None], onehot(Y, P.shape[1], dtype), out)
    return out, s


def inv_count(S, train_set, dtype):
    T = int((np.asarray(S).reshape(-1) == train_set).sum())
    return float(np.float32(1.0 / T)) if dtype == np.float32 else 1.0 / T


def pipeline(graph, logits, Y, S, train_set, L1, a1, L2, a2, autoscale=True, scale=1.0, dtype=np.float64):
    """steps 1-6 as smoothing.correct_and_smooth runs them; every intermediate in the result"""
    ip, ix, dv = graph
    P, E0, total = residual(logits, Y, S, train_set, dtype)
    al, be = factors(a1)
    if autoscale:
        E = propagate(ip, ix, dv, E0, L1, al, be, -1.0, 1.0, dtype=dtype)
    else:
        E = propagate(ip, ix, dv, E0, L1, al, be, -INF, INF, S, train_set, True, dtype)
    inv_T = inv_count(S, train_set, dtype)
    Z, s = correct(P, E, Y, S, train_set, total, inv_T, scale, autoscale, False, dtype)
    G0 = correct(P, E, Y, S, train_set, total, inv_T, scale, autoscale, True, dtype)[0]
    al, be = factors(a2)
    G = propagate(ip, ix, dv, G0, L2, al, be, 0.0, 1.0, dtype=dtype)
    quotient = row_scale(E, total, inv_T, dtype)[1]
    return dict(P=P, E0=E0, total=total, E=E, s=s, Z=Z, G0=G0, G=G, quotient=quotient, pred=G.argmax(axis=1))


def margins(G):
    """per row, the largest value minus the second largest (0 for one column: nothing to confuse)"""
    G = np.asarray(G, dtype=np.float64)
    if G.shape[1] < 2:
        return np.full(G.shape[0], INF)
    top = np.sort(G, axis=1)
    return top[:, -1] - top[:, -2]


def threshold_clear(quotient, rel=1e-3):
    """the autoscale rule's one discontinuity: no finite quotient lies within ``rel`` (relative) of 1000"""
    q = np.asarray(quotient, dtype=np.float64)
    q = q[np.isfinite(q)]
    return bool((np.abs(q - SCALE_LIMIT) > rel * SCALE_LIMIT).all())


def z_scale(want):
    """the row-scaled measure's yardstick for Z = P + s E: per row, the largest |P| + |s E| of its columns"""
    sc = (np.abs(want["P"]) + np.abs(want["s"][:, None] * want["E"])).max(axis=1, keepdims=True)
    return np.broadcast_to(sc, want["P"].shape)


# ---- shared inputs -----------------------------------------------------------------------------------------------------------------
def splits(n, rng, train=0.3, val=0.2):
    """0 train / 1 validation / 2 test in the given shares, and a few rows of no split (7)"""
    u = rng.random(n)
    S = np.where(u < train, 0, np.where(u < train + val, 1, 2)).astype(np.int32)
    S[rng.choice(n, size=max(1, n // 100), replace=False)] = 7
    return S


def noisy_logits(Y, C, noise, rng):
    return (2.0 * onehot(Y, C, np.float64) + noise * rng.standard_normal((np.asarray(Y).size, C))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def planted_case(n=1000, C=5, seed=0, noise=1.6):
    """A planted-partition graph (C equal communities, expected 8 neighbours inside and 3 outside, both directions, no
    self-loops), sym_normalize'd by the caller; the community is the class; 30 % training rows; logits = 2 onehot + noise"""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    Y = rng.integers(0, C, size=n).astype(np.int32)
    same = Y[:, None] == Y[None, :]
    prob = np.where(same, 8.0 / (n / C), 3.0 / (n - n / C))
    upper = np.triu(rng.random((n, n)) < prob, 1)
    adj = sp.csr_matrix((upper | upper.T).astype(np.float32))
    adj.sort_indices()
    S = splits(n, rng)
    logits = noisy_logits(Y, C, noise, rng)
    return dict(ip=adj.indptr.astype(np.uint32), ix=adj.indices.astype(np.uint32), dv=adj.data.astype(np.float32), n=n, C=C,
                Y=Y, S=S, logits=logits, params=dict(L1=20, a1=0.8, L2=20, a2=0.8, autoscale=True, scale=1.0))


MODEL_N = 600
MODEL_KINDS = ("asym", "sym")
MODEL_CLASSES = (7, 41)
MODEL_LAYERS = ((0, 0), (3, 3), (20, 20))


@functools.lru_cache(maxsize=None)
def model_graph(datasets, kind):
    """datasets.synth_powerlaw_csr(600, ...) or its symmetric twin, with sym_normalize'd values"""
    if kind == "sym":
        ip, ix, dv = datasets.synth_symmetric_powerlaw_csr(MODEL_N, MODEL_N + 2 * 2700, 120, seed=3)
    else:
        ip, ix, dv = datasets.synth_powerlaw_csr(MODEL_N, 6000, 120, seed=3)
    return ip, ix, datasets.sym_normalize(ip, ix, dv)


@functools.lru_cache(maxsize=None)
def model_inputs(C, seed=11):
    rng = np.random.default_rng(seed + C)
    Y = rng.integers(0, C, size=MODEL_N).astype(np.int32)
    return dict(Y=Y, S=splits(MODEL_N, rng), logits=noisy_logits(Y, C, 1.5, rng))


@functools.lru_cache(maxsize=None)
def model_case(datasets, kind, C, L1, L2, autoscale):
    """the whole pipeline's inputs, the fp64 reference, the twin, and the bar on G: eight times the twin's worst absolute
    error on this input (the device's SpMM adds in another order than the twin's)"""
    g, inp = model_graph(datasets, kind), model_inputs(C)
    args = (g, inp["logits"], inp["Y"], inp["S"], 0, L1, 0.8, L2, 0.8, autoscale, 0.9)
    want, twin = pipeline(*args, dtype=np.float64), pipeline(*args, dtype=np.float32)
    bar = 8.0 * float(np.abs(twin["G"].astype(np.float64) - want["G"]).max())
    return dict(graph=g, want=want, twin=twin, bar=bar, **inp)


def decided_rows(want_G, bar):
    """the rows whose prediction an error of ``bar`` per element cannot change"""
    return margins(want_G) > 2.0 * bar
