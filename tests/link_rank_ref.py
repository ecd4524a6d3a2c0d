"""The ranking metrics of the link head restated in numpy float64 (link.rank_metrics, csrc/link_rank.hip): the counts from
scores, and MRR / Hits@K from the counts by OGB's formulas."""
import numpy as np


def counts(s_pos, s_neg):
    """(greater, equal) per positive as int64: s_neg [m x K] holds each positive's own negatives, s_neg [m_neg] one list shared
    by all.  The scores are compared as the floats they are (-0.0 == +0.0)."""
    s_pos, s_neg = np.asarray(s_pos).reshape(-1, 1), np.asarray(s_neg)
    if s_neg.ndim == 1:
        s_neg = s_neg.reshape(1, -1)
    return (s_neg > s_pos).sum(axis=1).astype(np.int64), (s_neg == s_pos).sum(axis=1).astype(np.int64)


def metrics(greater, equal, ks, shared):
    """(mrr, {k: hits@k}): rank = 1 + greater + equal / 2; own negatives: hits@k = mean(rank <= k) (OGB _eval_mrr); a shared
    list: hits@k = mean(positive > k-th largest negative) = mean(greater + equal < k) (OGB _eval_hits)"""
    g, e = np.asarray(greater, dtype=np.float64), np.asarray(equal, dtype=np.float64)
    rank = 1.0 + g + e / 2.0
    return float(np.mean(1.0 / rank)), {k: float(np.mean(g + e < k) if shared else np.mean(rank <= k)) for k in ks}
