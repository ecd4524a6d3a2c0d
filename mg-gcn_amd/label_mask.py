"""The mask of gat(label_input=rate) on the host: which training rows feed their label in training forward ``epoch``.

Row r (global row number) is fed iff word 0 of
    Philox4x32-10(counter = (0xFFFFFFFF, r & 0xffffffff, r >> 32, epoch & 0xffffffff), key = (seed & 0xffffffff, seed >> 32))
is below floor(rate * 2^32) -- the definition of include/mggcn.h (mggcn_label_input_forward_f32), restated in vectorised
numpy.  The device regenerates the same bits in both kernels; the host needs only their COUNT, before the loss kernel of
the epoch is launched (the gradient scale is 1 / the number of training rows that were not fed) and without a
synchronisation, which is what fed_count is for.  The first counter word is a column group that mggcn_dropout_f32 never
draws, so a seed shared with dropout shares no bits.
"""
from __future__ import annotations

import math
import numbers

import numpy as np

COLUMN_GROUP = 0xFFFFFFFF                # the first counter word of every draw
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)       # Philox4x32: the multipliers
_W0, _W1 = 0x9E3779B9, 0xBB67AE85                            # and the key increments
_LOW, _32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def threshold(rate) -> int:
    """floor(rate * 2^32) as the uint32 the kernels compare with, computed in double; ValueError (naming label_input) for
    a rate outside [0, 1) or one that is not a number"""
    if not isinstance(rate, numbers.Real) or isinstance(rate, bool) or not 0.0 <= rate < 1.0:        # no NaN either
        raise ValueError(f"label_input: the rate must be a number in [0, 1), got {rate!r}")
    return int(math.floor(float(rate) * 4294967296.0))


def words(rows, seed: int, epoch: int) -> np.ndarray:
    """word 0 of the draw of every global row number in ``rows`` (any integer array), as uint32"""
    r = np.ascontiguousarray(rows).astype(np.uint64).reshape(-1)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    c0 = np.full(r.shape, COLUMN_GROUP, dtype=np.uint64)
    c1, c2 = r & _LOW, r >> _32
    c3 = np.full(r.shape, int(epoch) & 0xFFFFFFFF, dtype=np.uint64)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                          # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _32) ^ c1 ^ np.uint64(k0), p1 & _LOW, (p0 >> _32) ^ c3 ^ np.uint64(k1), p0 & _LOW
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0.astype(np.uint32)


def fed_mask(rows, threshold_: int, seed: int, epoch: int) -> np.ndarray:
    """True for the rows of ``rows`` that are fed in training forward ``epoch``"""
    if threshold_ == 0:
        return np.zeros(np.asarray(rows).size, dtype=bool)
    return words(rows, seed, epoch) < np.uint32(threshold_)


def fed_count(rows, threshold_: int, seed: int, epoch: int) -> int:
    return int(np.count_nonzero(fed_mask(rows, threshold_, seed, epoch)))
