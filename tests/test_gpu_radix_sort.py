"""The stable segmented radix sort (include/mggcn.h: mggcn_radix_sort_pairs_u32; csrc/radix_sort.hip) on the device against
np.argsort(kind="stable") per segment, exactly: the value of a pair is its input index, so stability shows in the values.
Every array -- keys, values, both scratch arrays and the work space -- sits inside a guarded allocation (tests/guarded.py)
and nothing outside [0, n_seg seg_len) may change; two calls give the same bits."""
import numpy as np
import pytest

from guarded import Guarded

pytestmark = pytest.mark.gpu

T = 4096                            # MGGCN_RADIX_SORT_TILE
SEG_LENS = (1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 1, 70_001)
N_SEGS = (1, 3, 41)
MAX_PAIRS = 4_000_000               # products above this are left out (none of the grid is: 41 x 70 001 = 2 870 041)
SHAPES = [(n_seg, seg_len) for seg_len in SEG_LENS for n_seg in N_SEGS if n_seg * seg_len <= MAX_PAIRS]
KEY_KINDS = ("random", "equal", "two", "top-byte", "low-byte", "sorted", "reverse")
BIT_RANGES = ((0, 32), (8, 24), (31, 32), (0, 1))


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


def _keys(kind, n_seg, seg_len, rng):
    shape = (n_seg, seg_len)
    if kind == "random":
        return rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)
    if kind == "equal":
        return np.full(shape, 0xDEADBEEF, dtype=np.uint32)
    if kind == "two":
        return np.where(rng.random(shape) < 0.5, np.uint32(0x80000001), np.uint32(0x7FFFFFFE)).astype(np.uint32)
    if kind == "top-byte":
        return (rng.integers(0, 256, size=shape, dtype=np.uint64) << 24 | 0x00ABCDEF).astype(np.uint32)
    if kind == "low-byte":
        return (rng.integers(0, 256, size=shape, dtype=np.uint64) | 0x12345600).astype(np.uint32)
    k = np.sort(rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32), axis=1)
    return k if kind == "sorted" else np.ascontiguousarray(k[:, ::-1])


def _expected(keys, begin_bit, end_bit):
    digit = (keys >> np.uint32(begin_bit)) & np.uint32((1 << (end_bit - begin_bit)) - 1)
    order = np.argsort(digit, axis=1, kind="stable")
    return np.take_along_axis(keys, order, axis=1), order.astype(np.uint32)


class _flat:
    """rows x cols contiguous u32 words inside a guarded allocation (a guard of at least one row in front and behind);
    .t is the tensor the call takes"""

    def __init__(self, rows, cols, logical=None, output=False):
        self.g = Guarded(rows, cols, cols, logical=logical, output=output)
        self.t = self.g.t[self.g.start:self.g.start + rows * cols]

    def words(self):
        return self.g.logical_bits().reshape(-1)


def _sort(pkg, ctx, keys, begin_bit, end_bit, what):
    n_seg, seg_len = keys.shape
    index = np.ascontiguousarray(np.broadcast_to(np.arange(seg_len, dtype=np.uint32), keys.shape))
    k, v = _flat(n_seg, seg_len, keys), _flat(n_seg, seg_len, index)
    ka, va = _flat(n_seg, seg_len, output=True), _flat(n_seg, seg_len, output=True)
    need = pkg.ops.radix_sort_work_bytes(n_seg, seg_len)
    assert need == ctx.lib.mggcn_radix_sort_work_bytes(n_seg, seg_len) and need % 4 == 0
    work = _flat(1, need // 4 + (need // 4) % 2, output=True)                      # an even count: the window stays 8-byte aligned
    pkg.ops.radix_sort_pairs(ctx, n_seg, seg_len, k.t, v.t, ka.t, va.t, work.t, begin_bit, end_bit)
    ctx.sync()
    for name, a in (("keys", k), ("vals", v), ("keys_alt", ka), ("vals_alt", va), ("work", work)):
        a.g.check_guards(f"{what}: {name}")
    return k.words().reshape(keys.shape), v.words().reshape(keys.shape)


@pytest.mark.parametrize("n_seg,seg_len", SHAPES)
def test_sort_matches_stable_argsort(pkg, ctx, n_seg, seg_len):
    rng = np.random.default_rng(1000 * n_seg + seg_len)
    cases = [(kind, 0, 32) for kind in KEY_KINDS] + [("random", b, e) for b, e in BIT_RANGES[1:]] + [("two", 31, 32), ("two", 0, 1)]
    for kind, b, e in cases:
        keys = _keys(kind, n_seg, seg_len, rng)
        what = f"{kind} keys, {n_seg} x {seg_len}, bits [{b}, {e})"
        got_k, got_v = _sort(pkg, ctx, keys, b, e, what)
        want_k, want_v = _expected(keys, b, e)
        np.testing.assert_array_equal(got_v, want_v, err_msg=what + ": values (the input index: order and stability)")
        np.testing.assert_array_equal(got_k, want_k, err_msg=what + ": keys")


@pytest.mark.parametrize("shape", [(3, 3 * T + 1), (41, T + 1), (1, 70_001)])
def test_two_calls_give_the_same_bits(pkg, ctx, shape):
    rng = np.random.default_rng(7)
    for kind, b, e in (("random", 0, 32), ("low-byte", 0, 32), ("two", 8, 24)):
        keys = _keys(kind, *shape, rng)
        first = _sort(pkg, ctx, keys, b, e, "first call")
        second = _sort(pkg, ctx, keys, b, e, "second call")
        np.testing.assert_array_equal(first[0], second[0])
        np.testing.assert_array_equal(first[1], second[1])


def test_an_empty_sort_launches_nothing_and_writes_nothing(pkg, ctx):
    k = _flat(1, 64, np.arange(64, dtype=np.uint32).reshape(1, 64))
    ctx.lib.mggcn_radix_sort_pairs_u32(ctx.stream(0), 0, 64, k.t.data_ptr(), None, None, None, 0, 32, None, 0)
    ctx.lib.mggcn_radix_sort_pairs_u32(ctx.stream(0), 64, 0, k.t.data_ptr(), None, None, None, 0, 32, None, 0)
    ctx.sync()
    k.g.check_unchanged("empty sort")
