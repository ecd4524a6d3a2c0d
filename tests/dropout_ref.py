"""Dropout on the host, for the dropout tests: Philox4x32-10 in numpy, the mask of mggcn_dropout_f32 (include/mggcn.h)
restated from its contract -- element (global row r, column c) of a call with (seed, stream) keeps its value iff word
c & 3 of Philox(counter = (c >> 2, r & 0xffffffff, r >> 32, stream), key = (seed & 0xffffffff, seed >> 32)) is >=
floor(p * 2^32) -- and a wrapper that puts that dropout into the CPU oracle's models without touching the oracle."""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # the multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # the key increments
_LOW = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: four uint32 values or arrays (broadcast against each other), key: two uint32 values -> four uint32 arrays"""
    c = [np.asarray(x, dtype=np.uint64) & _LOW for x in np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) for x in ctr])]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]             # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _LOW, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _LOW]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def params(p):
    """(threshold, scale) the host hands the kernel: floor(p * 2^32) and fp32(1 / (1 - p)), computed in double"""
    assert 0.0 <= p < 1.0
    return int(math.floor(p * 2.0 ** 32)), np.float32(1.0 / (1.0 - p))


def words(rows, m, row0, seed, stream):
    """the uint32 word of every element of a [rows x m] matrix whose first row is global row row0"""
    r = np.uint64(int(row0)) + np.arange(rows, dtype=np.uint64)
    g = np.arange((m + 3) // 4, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10((g[None, :], (r & _LOW)[:, None], (r >> np.uint64(32))[:, None], int(stream) & 0xFFFFFFFF),
                      (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(w, axis=-1).reshape(rows, -1)[:, :m]


def mask(rows, m, row0, p, seed, stream):
    """True where the element is KEPT"""
    return words(rows, m, row0, seed, stream) >= np.uint32(params(p)[0])


def apply(x, row0, p, seed, stream):
    """keep ? x * scale : +0.0 (one fp32 multiply; +0.0 also where x is NaN or an infinity)"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        scaled = x * params(p)[1]
    return np.where(mask(x.shape[0], x.shape[1], row0, p, seed, stream), scaled, np.float32(0.0)).astype(np.float32)


class oracle_dropout:
    """Dropout for an oracle.Gcn or oracle.DistGcn, by patching bound methods of its layers (nothing under oracle/
    changes): the input of every layer from index 1 on becomes D . H . scale in a training forward, and the gradient
    that layer returns D . G_out . scale, with the mask of (seed, stream = epoch * 64 + layer, row0).  ``epoch`` counts
    the train_forward calls, as the device model's dropout_epoch does; backward uses the number its forward used.

    oracle.Gcn: the layers' forward / backward.  oracle.DistGcn drives its layers' linears itself, so there every
    rank's lin.forward / lin.backward is patched, each with its rank's rows of the GLOBAL mask (row0 = p[rank]); that
    covers GEMM-first layers without a residual branch (the input of the layer IS lin's, its G_out IS lin's), the only
    kind from index 1 on in the models the tests build -- anything else is refused."""

    def __init__(self, O, p, seed=0, epoch=0):
        self.O, self.p, self.seed, self.epoch = O, float(p), int(seed), int(epoch)
        self.current, self.training = int(epoch), False
        inner = O.train_forward

        def train_forward(X, Y):
            self.current, self.training = self.epoch, True
            self.epoch += 1
            try:
                return inner(X, Y)
            finally:
                self.training = False
        O.train_forward = train_forward
        if hasattr(O, "ranks"):
            for j, layers in enumerate(O.ranks):
                for li, L in enumerate(layers):
                    if li >= 1:
                        if not L.gemm_first or L.residual_layer:
                            raise NotImplementedError("DistGcn wrapper: GEMM-first layers without a residual branch only")
                        self._patch(L.lin, li, int(O.p[j]))
        else:
            for li, L in enumerate(O.layers):
                if li >= 1:
                    self._patch(L, li, 0)

    def _drop(self, M, li, row0):
        return apply(M, row0, self.p, self.seed, (self.current * 64 + li) & 0xFFFFFFFF)

    def _patch(self, obj, li, row0):
        fwd, bwd = obj.forward, obj.backward

        def forward(H):
            return fwd(self._drop(H, li, row0) if self.training and self.p > 0.0 else H)

        def backward(G):
            out = bwd(G)
            return self._drop(out, li, row0) if out is not None and self.p > 0.0 else out
        obj.forward, obj.backward = forward, backward
