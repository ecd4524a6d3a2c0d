"""The two kernels of the max aggregator (include/mggcn.h: mggcn_agg_max_forward_f32 / mggcn_agg_max_backward_f32) against
tests/sage_ref.py, through the C ABI on guarded operands (guarded.py).

The pattern (sage_ref.kernel_pattern): 40 rows over 50 sources with rows of 0, 1, 63, 64, 65, 128, 129 and 200 entries -- the
boundaries of the 64-entry chunks --, unsorted rows, duplicate pairs and a source nobody references.  The widths take each
of the five (VEC, NT, U) variants on both paths: contiguous and padded operands take the four-column path where d % 4 == 0,
operands (or arg alone) offset by one float the element path.  B is drawn from {-2, -1, -0.0, +0.0, 1, 2, -inf}: ties are
everywhere, and the forward is a selection, so everything is asserted exactly -- arg is the reference's, out carries the bits
of B[arg - src0, c].  The backward is exact on integer gradients (every sum is exact in fp32 whatever the order) and meets
the standard summation bound k 2^-23 sum|terms| on normal ones; its bits repeat across calls and row splits."""
import numpy as np
import pytest

import sage_ref as ref
from guarded import Guarded

pytestmark = pytest.mark.gpu

WIDTHS = [1, 3, 4, 41, 64, 128, 132, 260, 1024]
VALUES = np.array([-2, -1, -0.0, 0.0, 1, 2, -np.inf], dtype=np.float32)
# name -> (pads of B / out / arg or arg / G / G_B in elements, their offsets in elements)
LAYOUTS = {"contiguous": ((0, 0, 0), (0, 0, 0)), "padded": ((4, 8, 12), (0, 0, 0)), "offset": ((1, 2, 3), (1, 1, 1)),
           "offset-arg": ((4, 8, 4), (0, 0, 1))}


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


@pytest.fixture(scope="module")
def pat():
    import torch
    indptr, indices, n_src = ref.kernel_pattern()
    t_indptr, t_indices = ref.transpose_pattern(indptr, indices, n_src)
    p = dict(indptr=indptr, indices=indices, t_indptr=t_indptr, t_indices=t_indices, n=len(indptr) - 1, n_src=n_src)
    lens = np.diff(indptr.astype(np.int64))
    assert {0, 1, 63, 64, 65, 128, 129, 200} <= set(lens.tolist()) and n_src - 1 not in indices
    for k in ("indptr", "indices", "t_indptr", "t_indices"):
        p["d_" + k] = torch.from_numpy(np.ascontiguousarray(p[k], dtype=np.uint32).view(np.int32)).cuda()
    return p


def _values(shape, seed):
    return np.random.default_rng(seed).choice(VALUES, size=shape)


_forward_ref = {}


def _reference(pat, d, nan=False):
    """B and the reference's (out, arg), computed once per width and shared"""
    key = (d, nan)
    if key not in _forward_ref:
        B = _values((pat["n_src"], d), 100 + d)
        if nan:
            rng = np.random.default_rng(7)
            B[rng.random(B.shape) < 0.3] = np.nan
            B[pat["indices"][pat["indptr"][1]]] = np.nan            # row 1 has one entry: a row of NaNs only
        out, arg = ref.agg_max(pat["indptr"], pat["indices"], B)
        for a in (B, out, arg):
            a.setflags(write=False)
        _forward_ref[key] = (B, out, arg)
    return _forward_ref[key]


def _forward(ctx, pat, B, layout="contiguous", with_arg=True, src0=0, splits=None):
    """one forward (``splits``: the row ranges, each a call of its own) into fresh guarded outputs; (out bits, arg)"""
    n, n_src, d = pat["n"], pat["n_src"], B.shape[1]
    pads, offs = LAYOUTS[layout]
    gB = Guarded(n_src, d, d + pads[0], offs[0], logical=B)
    gO = Guarded(n, d, d + pads[1], offs[1], output=True)
    gA = Guarded(n, d, d + pads[2], offs[2], output=True)
    ip, ix = pat["d_indptr"].data_ptr(), pat["d_indices"].data_ptr()
    for r0, r1 in splits or [(0, n)]:
        ctx.lib.mggcn_agg_max_forward_f32(ctx.stream(0), r1 - r0, n_src, ip + 4 * r0, ix, gB.ptr, gB.ld, d, src0,
                                          gO.ptr + 4 * r0 * gO.ld, gO.ld, gA.ptr + 4 * r0 * gA.ld if with_arg else None,
                                          gA.ld if with_arg else 0)
    ctx.sync()
    what = f"agg max forward d={d} {layout}"
    gB.check_unchanged(what)
    gO.check_guards(what)
    gA.check_guards(what)
    if not with_arg:
        assert (gA.bits() == gA.init).all(), f"{what}: arg = NULL was written"
    return gO.logical_bits(), gA.logical_bits()


def _check_forward(pat, B, want_arg, out_bits, arg, src0=0, what=""):
    want = np.where(want_arg == ref.NONE, ref.NONE, (want_arg.astype(np.int64) + src0) & 0xFFFFFFFF).astype(np.uint32)
    if arg is not None:
        assert (arg == want).all(), f"{what}: arg differs from the reference at {np.argwhere(arg != want)[:4].tolist()}"
    none = want_arg == ref.NONE
    picked = np.take_along_axis(B.view(np.uint32), np.where(none, 0, want_arg).astype(np.int64), axis=0)
    want_bits = np.where(none, np.uint32(0), picked)                   # nothing selected: +0.0
    assert (out_bits == want_bits).all(), f"{what}: out does not carry the winner's bits"


@pytest.mark.parametrize("d", WIDTHS)
def test_forward_selects_exactly_on_every_layout(ctx, pat, d):
    B, _, want_arg = _reference(pat, d)
    runs = {}
    for layout in LAYOUTS:
        out_bits, arg = _forward(ctx, pat, B, layout)
        _check_forward(pat, B, want_arg, out_bits, arg, what=f"d={d} {layout}")
        runs[layout] = (out_bits, arg)
    # the four-column and the element path: the same bits (a selection)
    for layout in ("padded", "offset", "offset-arg"):
        assert (runs[layout][0] == runs["contiguous"][0]).all() and (runs[layout][1] == runs["contiguous"][1]).all()
    # arg = NULL: the value only
    for layout in ("contiguous", "offset"):
        out_bits, _ = _forward(ctx, pat, B, layout, with_arg=False)
        assert (out_bits == runs["contiguous"][0]).all()
    # src0: the global index of column 0
    out_bits, arg = _forward(ctx, pat, B, "contiguous", src0=1000)
    _check_forward(pat, B, want_arg, out_bits, arg, src0=1000, what=f"d={d} src0")
    # each half of the rows as a call of its own, at a cut inside the long rows
    for layout in ("contiguous", "offset"):
        out_bits, arg = _forward(ctx, pat, B, layout, splits=[(0, 5), (5, pat["n"])])
        assert (out_bits == runs["contiguous"][0]).all() and (arg == runs["contiguous"][1]).all()


@pytest.mark.parametrize("d", [3, 4, 41, 128, 260])
def test_forward_never_selects_a_nan(ctx, pat, d):
    B, want_out, want_arg = _reference(pat, d, nan=True)
    assert (want_arg[1] == ref.NONE).all() and not np.isnan(want_out).any()
    for layout in ("contiguous", "offset"):
        out_bits, arg = _forward(ctx, pat, B, layout)
        _check_forward(pat, B, want_arg, out_bits, arg, what=f"NaN d={d} {layout}")
        assert (out_bits[1] == 0).all() and (arg[1] == ref.NONE).all()      # a row of NaNs only: +0.0 and NONE


def test_forward_and_backward_of_no_rows_return(ctx, pat):
    d = 8
    B = _values((pat["n_src"], d), 1)
    out_bits, arg = _forward(ctx, pat, B, "contiguous", splits=[(3, 3)])
    gO = Guarded(pat["n"], d, d, output=True, host=True)
    assert (out_bits == gO.logical_bits()).all() and (arg == gO.logical_bits()).all()      # untouched: the fill pattern
    G = _values((pat["n"], d), 2)
    got = _backward(ctx, pat, np.zeros((pat["n"], d), dtype=np.uint32), G, splits=[(7, 7)], raw=True)
    assert (got == gO.logical_bits()[:1].repeat(pat["n_src"], axis=0)).all()


# ---- backward -------------------------------------------------------------------------------------------------------------------
def _backward(ctx, pat, arg, G, layout="contiguous", src0=0, splits=None, accumulate=None, raw=False, repeat=1):
    """one backward over the sorted transpose into a fresh guarded G_B (``accumulate``: its initial values, and the flag);
    the fp32 result, or its bits with ``raw``"""
    n, n_src, d = pat["n"], pat["n_src"], G.shape[1]
    pads, offs = LAYOUTS[layout]
    gA = Guarded(n, d, d + pads[0], offs[2], logical=arg.astype(np.uint32))
    gG = Guarded(n, d, d + pads[1], offs[1], logical=np.ascontiguousarray(G, dtype=np.float32))
    gB = Guarded(n_src, d, d + pads[2], offs[0], logical=accumulate, output=True)
    tip, tix = pat["d_t_indptr"].data_ptr(), pat["d_t_indices"].data_ptr()
    for _ in range(repeat):
        for r0, r1 in splits or [(0, n_src)]:
            ctx.lib.mggcn_agg_max_backward_f32(ctx.stream(0), r1 - r0, n, tip + 4 * r0, tix, gA.ptr, gA.ld, gG.ptr, gG.ld, d,
                                               src0 + r0, 1 if accumulate is not None else 0, gB.ptr + 4 * r0 * gB.ld, gB.ld)
    ctx.sync()
    what = f"agg max backward d={d} {layout}"
    gA.check_unchanged(what)
    gG.check_unchanged(what)
    gB.check_guards(what)
    return gB.logical_bits() if raw else gB.values()


def _int_G(shape, seed):
    return np.random.default_rng(seed).integers(-8, 9, size=shape).astype(np.float32)


@pytest.mark.parametrize("d", WIDTHS)
def test_backward_is_exact_on_integer_gradients_on_every_layout(ctx, pat, d):
    _, _, arg = _reference(pat, d)
    G = _int_G((pat["n"], d), 200 + d)
    want = ref.agg_max_backward(pat["t_indptr"], pat["t_indices"], arg, G, pat["n_src"])
    # the check is sensitive to the skip rule: delivering every entry of a duplicated pair gives another sum somewhere
    rows = np.repeat(np.arange(pat["n"]), np.diff(pat["indptr"].astype(np.int64)))
    cols = pat["indices"].astype(np.int64)
    every = np.zeros_like(want)
    np.add.at(every, cols, np.where(arg[rows] == cols[:, None].astype(np.uint32), G[rows].astype(np.float64), 0.0))
    assert (every != want).any() and (ref.scatter_arg(G.astype(np.float64), arg, pat["n_src"]) == want).all()
    first = None
    for layout in LAYOUTS:
        got = _backward(ctx, pat, arg, G, layout)
        assert (got == want).all(), f"d={d} {layout}: {np.argwhere(got != want)[:4].tolist()}"
        bits = got.view(np.uint32)
        first = bits if first is None else first
        assert (bits == first).all()
    assert (want[pat["n_src"] - 1] == 0).all()                         # the source nobody references
    # src0 shifts what the rows compare against
    shifted = np.where(arg == ref.NONE, ref.NONE, arg.astype(np.int64) + 77).astype(np.uint32)
    assert (_backward(ctx, pat, shifted, G, "contiguous", src0=77) == want).all()
    # ACCUMULATE adds onto a non-zero G_B
    base = _int_G((pat["n_src"], d), 300 + d)
    for layout in ("contiguous", "offset"):
        assert (_backward(ctx, pat, arg, G, layout, accumulate=base) == want + base).all()


def test_a_duplicated_pair_delivers_its_gradient_once(ctx):
    """one destination lists source 2 three times and source 0 once; all of its gradient goes to 2, once"""
    import torch
    d = 4
    t_indptr = np.array([0, 1, 1, 4], dtype=np.uint32)                # rows: source 0 -> [0], source 1 -> [], source 2 -> [0, 0, 0]
    t_indices = np.array([0, 0, 0, 0], dtype=np.uint32)
    p = dict(n=1, n_src=3, d_t_indptr=torch.from_numpy(t_indptr.view(np.int32)).cuda(),
             d_t_indices=torch.from_numpy(t_indices.view(np.int32)).cuda())
    arg = np.array([[2, 2, 0, ref.NONE]], dtype=np.uint32)
    G = np.array([[3, -5, 7, 11]], dtype=np.float32)
    got = _backward(ctx, p, arg, G)
    assert got.tolist() == [[0, 0, 7, 0], [0, 0, 0, 0], [3, -5, 0, 0]]


@pytest.mark.parametrize("d", WIDTHS)
def test_backward_meets_the_summation_bound_and_repeats_its_bits(ctx, pat, d):
    _, _, arg = _reference(pat, d)
    G = np.random.default_rng(400 + d).standard_normal((pat["n"], d)).astype(np.float32)
    T = (pat["t_indptr"], pat["t_indices"])
    want = ref.agg_max_backward(*T, arg, G, pat["n_src"])
    sum_abs = ref.agg_max_backward(*T, arg, np.abs(G), pat["n_src"])
    k = ref.agg_max_backward(*T, arg, np.ones_like(G), pat["n_src"])
    assert k.max() >= 8                                                # sums long enough for the bound to mean something
    whole = {}
    for layout in ("contiguous", "offset"):
        bits = _backward(ctx, pat, arg, G, layout, raw=True)
        err = np.abs(bits.view(np.float32).astype(np.float64) - want)
        worst = float((err / np.maximum(k * 2.0 ** -23 * sum_abs, 1e-300)).max())
        print(f"[agg-max] backward d={d} {layout}: worst |err| / (k 2^-23 sum|terms|) = {worst:.3f}")
        assert (err <= k * 2.0 ** -23 * sum_abs).all(), (d, layout, worst)
        whole[layout] = bits
        # the same bits on a second call, and for the rows split between calls (a cut, and every row alone would be the same)
        assert (_backward(ctx, pat, arg, G, layout, raw=True, repeat=2) == bits).all()
        assert (_backward(ctx, pat, arg, G, layout, raw=True, splits=[(0, 11), (11, pat["n_src"])]) == bits).all()
