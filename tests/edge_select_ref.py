"""The exact fan-out on the host: the contract of mggcn_edge_sample_select_u32 (include/mggcn.h) restated with a per-row
np.sort over edge_sample_ref.words, the Horvitz-Thompson factors of the exact sample, and the graph of the kernel tests.
Row i of a forward matrix has as candidates its entries with i != j (global numbers, duplicates counted), m_i of them:
thr[i] = t_keep where m_i <= k, min(the (k+1)-th smallest candidate word, t_keep, 0xFFFFFFFE) otherwise."""
import numpy as np

import edge_sample_ref as ref

SEED, EPOCH = 0x0123456789ABCDEF, 3
N_ROWS, N_COLS, LONG, STRADDLE = 300, 6000, 5000, 11      # STRADDLE: the row whose k-th and (k+1)-th smallest words are one pair


def t_keep(keep):
    return int(ref.thresholds(np.zeros(2, dtype=np.int64), None, keep)[0])


def select(indptr, indices, k, keep, row0=0, col0=0, seed=0, epoch=0):
    dst, src, _ = ref.pairs(indptr, indices, 0, row0, col0)
    w = ref.words(dst, src, seed, epoch)
    thr = np.full(indptr.size - 1, t_keep(keep), dtype=np.uint32)
    for r in range(indptr.size - 1):
        s = slice(int(indptr[r]), int(indptr[r + 1]))
        cand = np.sort(w[s][dst[s] != src[s]])
        if cand.size > k:
            thr[r] = min(int(cand[k]), t_keep(keep), 0xFFFFFFFE)
    return thr


def exact_inverse_factors(indptr, indices, k):
    """one Python float64 expression per row, rounded to fp32 once"""
    out = np.empty(indptr.size - 1, dtype=np.float32)
    for r in range(out.size):
        m = sum(1 for c in indices[int(indptr[r]):int(indptr[r + 1])] if int(c) != r)
        out[r] = np.float32(1.0 if m == 0 else float(m) / float(min(k, m)))
    return out


_graphs = {}


def graph(k, reg):
    """(indptr, indices), 300 x 6000, columns in no order.  Rows 0-12: 0 entries; 1 (itself); k; k + 1; k + 1 with a self entry
    (m == k); 63; 64; 65; reg - 1; reg; reg + 1 (reg: the register path's longest row); 2 k + 6 with the candidate of the k-th
    smallest word (SEED, EPOCH, no offsets) written over the largest's: the duplicate straddles ranks k / k + 1; 5000.  The
    rest: 0 .. 150 entries, every third row with a self entry, every fifth a pair twice, every seventh a pair three times."""
    if (k, reg) not in _graphs:
        rng = np.random.default_rng(k)
        lengths = [0, 1, k, k + 1, k + 1, 63, 64, 65, reg - 1, reg, reg + 1, 2 * k + 6, LONG]
        lengths += list(rng.integers(0, 151, size=N_ROWS - len(lengths)))
        rows = [rng.choice(N_COLS - N_ROWS, size=int(n), replace=False) + N_ROWS for n in lengths]      # no self entry yet
        rows[1][0], rows[4][0] = 1, 4
        for r in range(13, N_ROWS):
            if r % 3 == 2 and lengths[r] > 0:
                rows[r][0] = r
            if r % 5 == 0 and lengths[r] > 4:
                rows[r][2] = rows[r][1]
            if r % 7 == 0 and lengths[r] > 6:
                rows[r][5] = rows[r][4] = rows[r][3]
        c = rows[STRADDLE].astype(np.uint64)
        order = np.argsort(ref.words(np.full(c.size, STRADDLE, dtype=np.uint64), c, SEED, EPOCH), kind="stable")
        rows[STRADDLE][order[-1]] = rows[STRADDLE][order[k - 1]]
        _graphs[(k, reg)] = (np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32), np.concatenate(rows).astype(np.uint32))
    return _graphs[(k, reg)]
