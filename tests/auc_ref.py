"""ROC-AUC restated in numpy, independent of the device algorithm (csrc/roc_auc.hip walks sorted tie groups; this searches):
per class and view, sort the keys of the negatives, then
    2U = sum over the positives of searchsorted(neg, key, "left") + searchsorted(neg, key, "right").
Also the key map, the value word, and the summary metrics.roc_auc_evaluator returns, restated."""
import math

import numpy as np

VIEWS = ("train", "val", "test", "other", "all")


def keys_of(logits):
    """x = logit + 0.0f (so -0.0 ties with +0.0), u = bits(x), key = (u >> 31) ? ~u : (u | 0x80000000)"""
    x = np.asarray(logits, dtype=np.float32) + np.float32(0.0)
    u = np.ascontiguousarray(x).view(np.uint32)
    return np.where(u >> np.uint32(31) != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def slots_of(sets, n):
    if sets is None:
        return np.zeros(n, dtype=np.int64)
    s = np.asarray(sets).reshape(-1).astype(np.int64)
    return np.where((s >= 0) & (s < 3), s, 3)


def vals_of(targets, sets):
    """value = slot << 1 | (target != 0), one column per class"""
    t = np.asarray(targets)
    return ((slots_of(sets, t.shape[0])[:, None] << 1) | (t != 0)).astype(np.uint32)


def two_u(pos_keys, neg_keys):
    neg = np.sort(np.asarray(neg_keys))
    pos = np.asarray(pos_keys)
    return int(np.searchsorted(neg, pos, "left").astype(np.int64).sum() + np.searchsorted(neg, pos, "right").astype(np.int64).sum())


def stats(logits, targets, sets=None):
    """[C][5][3] Python integers (2U, P, N): views train, val, test, other, all"""
    logits, targets = np.asarray(logits, dtype=np.float32), np.asarray(targets)
    n, C = logits.shape
    keys, slot = keys_of(logits), slots_of(sets, n)
    out = []
    for c in range(C):
        pos = targets[:, c] != 0
        row = []
        for k in range(5):
            member = np.ones(n, dtype=bool) if k == 4 else slot == k
            p, q = keys[member & pos, c], keys[member & ~pos, c]
            row.append((two_u(p, q), int(p.size), int(q.size)))
        out.append(row)
    return out


def auc_of(u2, p, q):
    den = 2 * p * q
    return u2 / den if den else float("nan")


def summary(st):
    """{"train": ..., ..., "all": ...} the mean over the classes whose AUC is defined (exactly rounded sum / count), and
    "per_class" [5 x C]"""
    per_class = np.array([[auc_of(*st[c][k]) for c in range(len(st))] for k in range(5)], dtype=np.float64).reshape(5, len(st))
    out = {"per_class": per_class}
    for k, name in enumerate(VIEWS):
        known = [v for v in per_class[k].tolist() if not math.isnan(v)]
        out[name] = math.fsum(known) / len(known) if known else float("nan")
    return out


def pair_count(scores, labels):
    """the O(P N) definition on the floats: 2 (p > n) + (p == n) over every (positive, negative) pair"""
    s = np.asarray(scores, dtype=np.float32)
    y = np.asarray(labels) != 0
    p, q = s[y][:, None], s[~y][None, :]
    return int((2 * (p > q).astype(np.int64) + (p == q)).sum())
