"""Masked label inputs on the host, for the label-input tests: the mask, the two kernels and the model semantics of
gat(label_input=rate) restated from their contract (include/mggcn.h: mggcn_label_input_*), without the package.

  mask      training row r (global number) is fed in training forward e iff word 0 of
            Philox4x32-10(counter = (0xFFFFFFFF, r & 0xffffffff, r >> 32, e), key = (seed & 0xffffffff, seed >> 32))
            is below floor(rate * 2^32); dropout_ref's Philox is the generator
  forward   Z[i] += E[y_i] for the fed rows, one fp32 add per element; S_e[i] = 3 there, the training set on the other
            training rows
  backward  G_E[c] = the sum of G_Z[i] over the fed rows of class c (fp64 here)
  model     [X | M onehot(y)] [W ; E] = X W + M E[y]: the label-input model is the plain model on the augmented features
            and the augmented first weight matrix, with the loss over the training rows that were not fed
"""
import math

import numpy as np

import dropout_ref

COLUMN_GROUP = 0xFFFFFFFF
FED_SET = 3
CHUNK = 64                      # csrc/label_input.hip kLabelChunk: list entries per partial of the backward kernel
_LOW = np.uint64(0xFFFFFFFF)


def threshold(rate):
    assert 0.0 <= rate < 1.0
    return int(math.floor(rate * 2.0 ** 32))


def words(rows, seed, epoch):
    """word 0 of the draw of every global row number in ``rows``"""
    r = np.asarray(rows, dtype=np.uint64).reshape(-1)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return dropout_ref.philox4x32_10((COLUMN_GROUP, r & _LOW, r >> np.uint64(32), int(epoch) & 0xFFFFFFFF),
                                     (seed & 0xFFFFFFFF, seed >> 32))[0]


def fed_mask(rows, thr, seed, epoch, feed_all=False):
    """True for the global rows that are fed; ``thr``: the uint32 threshold"""
    n = np.asarray(rows).size
    if feed_all:
        return np.ones(n, dtype=bool)
    return words(rows, seed, epoch).astype(np.uint64) < np.uint64(thr)


def lists(S, Y, train_set, n_classes):
    """(rows, cls, cls_ptr): the training rows sorted by (class, row), their classes, the segment of each class"""
    s, y = np.asarray(S).reshape(-1), np.asarray(Y).reshape(-1).astype(np.int64)
    train = np.flatnonzero(s == train_set)
    order = np.lexsort((train, y[train]))
    rows, cls = train[order], y[train][order]
    cls_ptr = np.searchsorted(cls, np.arange(n_classes + 1))
    return rows.astype(np.int32), cls.astype(np.int32), cls_ptr.astype(np.int32)


def forward(Z, S, E, rows, cls, fed, kept_set=0, fed_set=FED_SET):
    """(Z', S') of mggcn_label_input_forward_f32: ``fed`` is a bool per list entry; S may be None"""
    Z = np.array(Z, dtype=np.float32)
    r, c = np.asarray(rows, dtype=np.int64), np.asarray(cls, dtype=np.int64)
    Z[r[fed]] = Z[r[fed]] + np.asarray(E, dtype=np.float32)[c[fed]]            # rows are unique: one fp32 add per element
    if S is None:
        return Z, None
    S = np.array(S, dtype=np.int32).reshape(-1)
    S[r] = np.where(fed, fed_set, kept_set)
    return Z, S


def backward64(G_Z, rows, cls, fed, n_classes):
    """(G_E, sum |g|, fed rows) per class in fp64: the restatement and what its error bound needs"""
    G = np.asarray(G_Z, dtype=np.float64)
    r, c = np.asarray(rows, dtype=np.int64)[fed], np.asarray(cls, dtype=np.int64)[fed]
    G_E, A = np.zeros((n_classes, G.shape[1])), np.zeros((n_classes, G.shape[1]))
    np.add.at(G_E, c, G[r])
    np.add.at(A, c, np.abs(G[r]))
    return G_E, A, np.bincount(c, minlength=n_classes)


def gamma(k):
    """Higham's gamma_k for fp32 sums of k terms (any order): k u / (1 - k u), u = 2^-24"""
    ku = np.asarray(k, dtype=np.float64) * 2.0 ** -24
    return ku / (1.0 - ku)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def epoch_sets(S, train_set, thr, seed, epoch, feed_all=False, row0=0):
    """(M, S_e): the bool per vertex that is fed, and the sets the loss of that forward sees"""
    s = np.asarray(S, dtype=np.int32).reshape(-1)
    train = np.flatnonzero(s == train_set)
    M = np.zeros(s.size, dtype=bool)
    M[train] = fed_mask(train + row0, thr, seed, epoch, feed_all)
    S_e = s.copy()
    S_e[M] = FED_SET
    return M, S_e


def counts(S_e):
    s = np.asarray(S_e).reshape(-1)
    c = [int((s == k).sum()) for k in range(3)]
    return dict(zip(("train", "val", "test", "other"), c + [int(s.size) - sum(c)]))


def augmented_features(X, Y, M, n_classes):
    """[X | M onehot(y)]"""
    X = np.asarray(X, dtype=np.float32)
    onehot = np.zeros((X.shape[0], n_classes), dtype=np.float32)
    idx = np.flatnonzero(M)
    onehot[idx, np.asarray(Y).reshape(-1)[idx]] = 1.0
    return np.ascontiguousarray(np.concatenate([X, onehot], axis=1))


def split_loss(orc, Y, keep):
    """the ``loss=`` callable of the reference models for the softmax cross-entropy over the rows of ``keep``:
    H -> (G, (loss, acc)), the gradient scaled by 1 / the number of kept rows and zero elsewhere"""
    y = np.asarray(Y).reshape(-1)
    k = int(keep.sum())

    def loss(H):
        _, _, G, O = orc.softmax_cross_entropy(H, Y, n_global=k)
        G = np.ascontiguousarray(G)
        G[~keep] = 0
        p = O[np.arange(y.size), y].astype(np.float64)
        return G, (float(np.abs(np.log(p))[keep].sum() / k), float((O.argmax(axis=1) == y)[keep].mean()))
    return loss


class oracle_label_input:
    """Label inputs for a reference model (gat_ref.oracle_gat and its subclasses), by patching the bound methods of its
    first layer's linear: forward adds E[y] to the fed rows of Z, backward sums G_Z into ``G_E`` (fp64, rounded once).
    ``M``: the bool per vertex that is fed in the forwards that follow."""

    def __init__(self, O, E, Y, M):
        self.O, self.E, self.M = O, np.array(E, dtype=np.float32), np.asarray(M, dtype=bool)
        self.y = np.asarray(Y).reshape(-1).astype(np.int64)
        self.G_E = None
        lin = O.layers[0].lin
        fwd, bwd = lin.forward, lin.backward

        def forward(X):
            Z = fwd(X)
            idx = np.flatnonzero(self.M)
            Z[idx] = Z[idx] + self.E[self.y[idx]]
            return Z

        def backward(G):
            idx = np.flatnonzero(self.M)
            G_E = np.zeros(self.E.shape)
            np.add.at(G_E, self.y[idx], np.asarray(G, dtype=np.float64)[idx])
            self.G_E = G_E.astype(np.float32)
            return bwd(G)
        lin.forward, lin.backward = forward, backward


# ---- the learning fixture ------------------------------------------------------------------------------------------------------------------
# A planted-partition graph whose features are pure noise in one column (too little to tell 300 training vertices apart, so a
# model cannot memorise its neighbours) and whose neighbours' labels determine the class (9 of 10 sources share the
# destination's block).  The reference model alone, on the CPU (reference_learning below: gatdot_ref.oracle_gatdot on the
# augmented features, the device model's initial values), reaches after LEARN["epochs"] epochs a validation accuracy of
LEARN_REFERENCE = {"plain": 0.346, "label": 0.950}
# and both bars of the device test sit inside that gap:
LEARN_BARS = {"plain": 0.55, "label": 0.75}                # plain stays below, label_input=0.5 gets above
LEARN = dict(n=600, classes=5, deg=8, p_in=0.9, features=1, hidden=32, heads=4, epochs=60, rate=0.5, seed=3, label_seed=11)


def learning_case():
    """(csr, X, Y, S) of the fixture"""
    c = LEARN
    ip, ix, dv, Y = planted_partition(c["n"], c["classes"], c["deg"], c["p_in"], seed=c["seed"])
    rng = np.random.default_rng(c["seed"] + 1)
    X = rng.standard_normal((c["n"], c["features"]), dtype=np.float32)
    S = rng.choice(3, size=c["n"], p=(0.5, 0.25, 0.25)).astype(np.int32)
    return (ip, ix, dv), X, Y, S


def reference_learning(orc, label):
    """the validation accuracy of the reference model after training on the fixture, with (``label``) or without label
    inputs; evaluation feeds every training label"""
    import gatdot_ref
    c = LEARN
    (ip, ix, dv), X, Y, S = learning_case()
    F, C, zw = c["features"], c["classes"], 3 * c["hidden"]
    O = gatdot_ref.oracle_gatdot(orc, orc.Csr(ip.copy(), ix.copy(), dv.copy(), c["n"]), [F + (C if label else 0), c["hidden"], C],
                                 [c["heads"], 1])
    if label:                                              # the device's start: W and E are tensors of their own
        E = orc.init_uniform(zw, C).reshape(C, zw)
        O.layers[0].lin.W = np.ascontiguousarray(np.concatenate([orc.init_uniform(F, zw), E], axis=0))
    thr = threshold(c["rate"])
    for e in range(c["epochs"]):
        M, S_e = epoch_sets(S, 0, thr, c["label_seed"], e) if label else (None, S)
        O.loss = split_loss(orc, Y, S_e == 0)
        O.train_forward(augmented_features(X, Y, M, C) if label else X, Y)
        O.backward()
        O.adam_update()
    if label:
        M, _ = epoch_sets(S, 0, thr, c["label_seed"], 0, feed_all=True)
    H = O.forward(augmented_features(X, Y, M, C) if label else X)
    return float((H.argmax(axis=1) == Y.reshape(-1))[S == 1].mean())


def planted_partition(n, n_classes, deg, p_in, seed):
    """(indptr, indices, values, Y): a directed graph of n vertices in n_classes equal blocks, ``deg`` sources per
    destination of which each is from the destination's own block with probability p_in, a uniform vertex otherwise; CSR of
    A with A[j, i] = 1 for source j of destination i (the models aggregate over A^T's rows), values 1"""
    rng = np.random.default_rng(seed)
    Y = rng.integers(0, n_classes, size=n).astype(np.int32)
    members = [np.flatnonzero(Y == c) for c in range(n_classes)]
    dst = np.repeat(np.arange(n), deg)
    own = rng.random(n * deg) < p_in
    src = rng.integers(0, n, size=n * deg)
    pick = rng.random(n * deg)
    for c in range(n_classes):
        sel = own & (Y[dst] == c)
        src[sel] = members[c][(pick[sel] * members[c].size).astype(np.int64)]
    order = np.lexsort((dst, src))                          # rows of A are sources
    indptr = np.zeros(n + 1, dtype=np.uint32)
    np.cumsum(np.bincount(src, minlength=n), out=indptr[1:])
    return indptr, dst[order].astype(np.uint32), np.ones(n * deg, dtype=np.float32), Y.reshape(-1, 1)
