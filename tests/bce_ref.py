"""The multi-label loss on the host, for the sigmoid-BCE tests: the contract of mggcn_sigmoid_bce_from_f32
(include/mggcn.h) restated in fp64, its fp32 twin with the kernel's formulas, the per-slot sums, and a wrapper that puts
the loss into an oracle.Gcn without touching anything under oracle/.

Per element, with z the logit and t in {0, 1}:  softplus(x) = max(x, 0) + log1p(exp(-|x|)),
loss = t ? softplus(-z) : softplus(z),  p = z >= 0 ? 1 / (1 + exp(-z)) : exp(z) / (1 + exp(z)),  pred = z > 0."""
import numpy as np

SPLIT_NAMES = ("train", "val", "test", "other")


def slot(S):
    """slot(s) = s for 0 <= s <= 2, 3 for every other value"""
    S = np.asarray(S).reshape(-1)
    return np.where((S >= 0) & (S <= 2), S, 3).astype(np.int64)


def _softplus(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def _sigmoid(z):
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(-np.abs(z))
        return np.where(z >= 0, 1 / (1 + e), e / (1 + e))


def loss64(Z, T):
    """the loss of every element, fp64 arithmetic on the fp32 logits"""
    z = np.asarray(Z, dtype=np.float64)
    return np.where(np.asarray(T) != 0, _softplus(-z), _softplus(z))


def prob64(Z):
    return _sigmoid(np.asarray(Z, dtype=np.float64))


def grad64(Z, T, grad_scale, train=None):
    """(p - t) * grad_scale on the rows where ``train`` is set (None: every row), 0 elsewhere; fp64"""
    g = (prob64(Z) - (np.asarray(T) != 0)) * float(grad_scale)
    if train is not None:
        g = np.where(np.asarray(train, dtype=bool).reshape(-1, 1), g, 0.0)
    return g


def pred(Z):
    """z > 0: +-0 and NaN predict negative"""
    with np.errstate(invalid="ignore"):
        return np.asarray(Z) > 0


def counts(Z, T, S=None):
    """[4 x 3] integers: (TP, FP, FN) of the slots train / val / test / other; S None: every row in slot 0"""
    p, t = pred(Z), np.asarray(T) != 0
    sl = np.zeros(p.shape[0], dtype=np.int64) if S is None else slot(S)
    out = np.zeros((4, 3), dtype=np.int64)
    for k in range(4):
        r = sl == k
        out[k] = ((p[r] & t[r]).sum(), (p[r] & ~t[r]).sum(), (~p[r] & t[r]).sum())
    return out


def loss_sums64(Z, T, S=None):
    """the four loss sums, fp64"""
    l = loss64(Z, T)
    sl = np.zeros(l.shape[0], dtype=np.int64) if S is None else slot(S)
    return np.array([l[sl == k].sum() for k in range(4)], dtype=np.float64)


def micro_f1(tp, fp, fn):
    den = 2.0 * tp + fp + fn
    return float(2.0 * tp / den) if den else float("nan")


# ---- fp32 twin: the kernel's formulas, element by element ----------------------------------------------------------------------
def loss32(Z, T):
    z = np.asarray(Z, dtype=np.float32)
    zt = np.where(np.asarray(T) != 0, -z, z)
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.maximum(zt, np.float32(0)) + np.log1p(np.exp(-np.abs(z)))).astype(np.float32)


def grad32(Z, T, grad_scale, train=None):
    z = np.asarray(Z, dtype=np.float32)
    one = np.float32(1)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(-np.abs(z))
        p = np.where(z >= 0, one / (one + e), e / (one + e)).astype(np.float32)
    g = ((p - (np.asarray(T) != 0).astype(np.float32)) * np.float32(grad_scale)).astype(np.float32)
    if train is not None:
        g = np.where(np.asarray(train, dtype=bool).reshape(-1, 1), g, np.float32(0)).astype(np.float32)
    return g


class oracle_bce:
    """The multi-label loss for an oracle.Gcn: train_forward becomes the oracle's own forward plus the fp32 restatement
    above (the loss sums are added in fp64: the order of the device's sums is not the oracle's business).  Sets O.G and
    returns (loss, micro_f1) of ``train_set`` -- of all rows when S is None; ``per`` keeps every slot's
    (loss, f1, (tp, fp, fn), rows) of the last call.  Wrap after layernorm_ref.oracle_layer_norm and BEFORE
    dropout_ref.oracle_dropout, which wraps train_forward on top."""

    def __init__(self, oracle, O, T, S=None, train_set=0):
        self.oracle, self.O = oracle, O
        self.T = np.asarray(T)
        self.S = None if S is None else np.asarray(S).reshape(-1)
        self.train_set = int(train_set)
        self.per = {}

        def train_forward(X, Y=None):
            H = O.forward(np.ascontiguousarray(X, dtype=np.float32))
            return self.loss(H)
        O.train_forward = train_forward

    def loss(self, H):
        n, m = H.shape
        train = None if self.S is None else self.S == self.train_set
        rows = n if train is None else int(train.sum())
        self.O.G = np.ascontiguousarray(grad32(H, self.T, 1.0 / (float(rows) * m), train))
        self.O.logits = H
        l = loss32(H, self.T).astype(np.float64)
        sl = np.zeros(n, dtype=np.int64) if self.S is None else slot(self.S)
        c = counts(H, self.T, self.S)
        for k, name in enumerate(SPLIT_NAMES):
            r = int((sl == k).sum())
            self.per[name] = ((float(l[sl == k].sum() / (r * m)) if r else float("nan")), micro_f1(*c[k]),
                              tuple(int(v) for v in c[k]), r)
        return self.per[SPLIT_NAMES[self.train_set if self.S is not None else 0]][:2]


# ---- the model tests' inputs ------------------------------------------------------------------------------------------------
def model_data(pkg, n=1536, F=20, C=8):
    """graph, features, targets at density 0.2 and sets drawn 60 / 20 / 20, shared by the single-GPU and the row-partition
    tests"""
    ip, ix, dv = pkg.datasets.synth_powerlaw_csr(n, n * 16, 700, seed=21)
    rng = np.random.default_rng(22)
    X = rng.standard_normal((n, F), dtype=np.float32)
    T = (rng.random((n, C)) < 0.2).astype(np.int32)
    S = rng.choice(3, size=n, p=(0.6, 0.2, 0.2)).astype(np.int32)
    return (ip, ix, dv), X, T, S
