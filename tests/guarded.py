"""Guarded device views for the layout tests (test_gpu_layouts.py, test_gpu_gat_layouts.py): a rows x cols matrix with
leading dimension `ld` placed at element offset `off` inside one flat device buffer, with at least one guard row in front
and one behind (`tail_rows`: that many behind, so that a kernel that walks the matrix with another operand's leading
dimension still lands inside the allocation; `host`: the same buffer in host memory only, for the CPU model of the checks).
Every element outside the logical matrix holds a fixed NaN bit pattern -- a different one for inputs and for outputs --
so that a kernel that stores into a pad, or lets an input pad reach a stored result, is caught bit for bit."""
import numpy as np

# quiet NaNs with payloads that no arithmetic produces
OUT_NAN32, IN_NAN32 = 0x7FC0DEAD, 0xFFC0BEEF
OUT_NAN16, IN_NAN16 = 0x7FD5, 0xFFE3


def _torch():
    import torch
    return torch


class Guarded:
    """`logical`: float32 values (fp32) or uint16 bit patterns (bf16) of the matrix; None leaves the logical elements
    at the fill pattern too (an output that must be written, or a NaN-filled C that beta = 0 must never read)."""

    def __init__(self, rows, cols, ld, off=0, logical=None, output=False, bf16=False, tail_rows=None, host=False):
        assert ld >= cols and off >= 0
        self.rows, self.cols, self.ld, self.off, self.bf16 = rows, cols, ld, off, bf16
        self.bits_dtype = np.uint16 if bf16 else np.uint32
        self.itemsize = 2 if bf16 else 4
        fill = (OUT_NAN16 if output else IN_NAN16) if bf16 else (OUT_NAN32 if output else IN_NAN32)
        # the guard in front is at least one row and a multiple of 64 elements: before `off` the matrix starts on a
        # 256-byte (fp32) / 128-byte (bf16) boundary of the allocation (torch aligns allocations to at least that)
        self.head = -(-max(ld, 1) // 64) * 64
        self.start = self.head + off
        # the guard behind: the front guard's size, or tail_rows rows where that is more
        self.tail = self.head if tail_rows is None else max(self.head, tail_rows * ld)
        total = self.start + rows * ld + self.tail
        self.init = np.full(total, fill, dtype=self.bits_dtype)
        self.mask = np.zeros(total, dtype=bool)
        self._window(self.mask)[:] = True
        if logical is not None:
            src = np.asarray(logical)
            assert src.shape == (rows, cols), (src.shape, rows, cols)
            self._window(self.init)[:] = src.view(self.bits_dtype) if src.dtype != self.bits_dtype else src
        if host:
            self.t, self.host = None, self.init.copy()
            return
        torch = _torch()
        self.t = torch.from_numpy(self.init.view(np.int16 if bf16 else np.int32).copy()).cuda()

    def _window(self, flat):
        return flat[self.start:self.start + self.rows * self.ld].reshape(self.rows, self.ld)[:, :self.cols]

    @property
    def ptr(self) -> int:
        """device address of element (0, 0)"""
        return self.t.data_ptr() + self.start * self.itemsize

    def bits(self) -> np.ndarray:
        if self.t is None:
            return self.host
        return self.t.cpu().numpy().view(self.bits_dtype)

    def logical_bits(self, bits=None) -> np.ndarray:
        return self._window(self.bits() if bits is None else bits).copy()

    def values(self, bits=None) -> np.ndarray:
        """the logical matrix as float32 (fp32 buffers)"""
        assert not self.bf16
        return self.logical_bits(bits).view(np.float32)

    def _where(self, i) -> str:
        k = int(i) - self.start
        if k < 0:
            return f"front guard, {-k} element(s) before (0, 0)"
        r, c = divmod(k, self.ld)
        return f"row {r}, column {c}" if r < self.rows else f"back guard, row {r}, column {c}"

    def check_guards(self, what, bits=None):
        """(a) nothing outside the logical matrix changed, bit for bit"""
        b = self.bits() if bits is None else bits
        bad = np.flatnonzero((b != self.init) & ~self.mask)
        assert bad.size == 0, (f"{what}: {bad.size} element(s) outside the logical {self.rows}x{self.cols} matrix "
                               f"(ld {self.ld}, offset {self.off}) changed; first: {self._where(bad[0])}")

    def check_unchanged(self, what):
        """(b) an input buffer, pads and all, is exactly as it was uploaded"""
        b = self.bits()
        bad = np.flatnonzero(b != self.init)
        assert bad.size == 0, f"{what}: input buffer written ({bad.size} element(s)); first: {self._where(bad[0])}"
