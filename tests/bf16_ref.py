"""bf16 on the host, for the bf16-aggregation tests: round-to-nearest-even from fp32 the way torch's CPU cast does it
(``.to(torch.bfloat16)``; a NaN stays a NaN -- here the quiet NaN 0x7FC0 -- its payload is not compared), and the exact
widening back to fp32."""
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
