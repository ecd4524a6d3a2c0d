"""bf16 on the host, for the bf16-aggregation tests: round-to-nearest-even from fp32 the way torch's CPU cast does it
(``.to(torch.bfloat16)``; a NaN stays a NaN -- here the quiet NaN 0x7FC0 -- its payload is not compared), the exact
widening back to fp32, the CPU oracle's model with every aggregation on the rounded operand, and the bars of the model tests."""
import numpy as np


def bf16_bits(x) -> np.ndarray:
    """uint16 bit patterns of bf16(x), x fp32: nearest even, overflow -> +-inf, NaN -> 0x7FC0"""
    x = np.asarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    r[np.isnan(x)] = 0x7FC0
    return r


def widen(bits) -> np.ndarray:
    """fp32 values of bf16 bit patterns (exact)"""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def round_bf16(x) -> np.ndarray:
    """fp32 -> bf16 -> fp32"""
    return widen(bf16_bits(x))


def bf16_oracle(oracle, ip, ix, dv, n, sizes, residual_layer, f64acc=True):
    """oracle.Gcn with every SpMM wrapped as A . bf16(B): what gcn(agg_dtype="bf16") computes, sums in fp64 by default"""
    O = oracle.Gcn(oracle.Csr(ip, ix, dv, n), sizes, f64acc=f64acc, residual_layer=residual_layer)
    for L in O.layers:                                      # every aggregation multiplies by bf16(B)
        L.spmm_fwd = lambda B, f=L.spmm_fwd: f(round_bf16(B))
        L.spmm_bwd = lambda B, f=L.spmm_bwd: f(round_bf16(B))
    return O


# Gradient bars of the bf16 model tests.  The device and the oracle round DIFFERENT fp32 inputs to bf16 (they agree to ~1e-7, not bit for bit),
# so an element within 1e-7 of a rounding midpoint goes one way here and the other way there: a 2^-8 relative jump.
# The first layer's G_W = X^T T (random X) cancels down to a small fraction of its terms and shows those flips at
# ~1e-3 of its largest entry (measured on the CPU with the fp32 oracle standing in for the device: up to 4.1e-3 over
# three epochs); the layers above stay at <= 8e-5.  The bf16 model is farther from the fp32 model on the same
# measure: 2.3e-2 .. 3.3e-2 on the first layer, >= 7e-4 above it -- while the LOSS of the two differs by ~1e-6 only.
GRAD_BAR = {0: 1e-2}           # the first layer's G_W; every other gradient: GRAD_BAR_REST
GRAD_BAR_REST = 3e-4
W_SOLID_BAR = {0: 1e-2}        # well-conditioned entries of W after the Adam step (fp32 tests: 1e-4 for all layers)
