"""The packed (arg, gradient) record of the max aggregator on the device (include/mggcn.h: mggcn_agg_max_pack_f32,
mggcn_agg_max_backward_rec_f32), through the C ABI on guarded operands (guarded.py).

The pattern is test_gpu_agg_max.py's (sage_ref.kernel_pattern transposed: rows of 0, 1, 63, 64, 65, 128, 129 and 200 entries
among the forward rows, duplicates, an unreferenced source) and so are the widths, which take each of the five (VEC, NT, U)
variants on both load paths.  Layouts -- every operand behind guards, with a leading dimension of its own:
  contiguous   ld = d (rec: 2 d), everything 16-byte aligned: the four-column path where d % 4 == 0
  padded       arg d + 4, G d + 8, G_B d + 12, rec 2 d + 8: the same path
  offset       arg, G and G_B one float off 16-byte alignment, rec two words off (8-byte aligned, as it must be): the element
               path of the plain AND of the record call at every width, so their geometry is equal
  rec8         arg, G and G_B contiguous, rec alone two words off: the record calls take the element path at d % 4 == 0 where
               the plain call takes four columns -- another geometry, compared on integer gradients only (exact in any order)
The pack is a copy of bit patterns; the record backward must give the plain entry point's bits wherever both run the same
variant, and sage_ref.agg_max_backward exactly on integer gradients everywhere."""
import numpy as np
import pytest

import sage_ref as ref
from guarded import OUT_NAN32, Guarded
from test_gpu_agg_max import WIDTHS, _int_G, _reference, ctx, pat        # noqa: F401  (the two fixtures, the shared reference)

pytestmark = pytest.mark.gpu

# name -> (pads of arg / G / G_B / rec, offsets of arg / G / G_B / rec) in 4-byte elements
LAYOUTS = {"contiguous": ((0, 0, 0, 0), (0, 0, 0, 0)), "padded": ((4, 8, 12, 8), (0, 0, 0, 0)),
           "offset": ((1, 2, 3, 2), (1, 1, 1, 2)), "rec8": ((0, 0, 0, 0), (0, 0, 0, 2))}
SAME_VARIANT = ("contiguous", "padded", "offset")


def _interleave(arg, gbits):
    rec = np.empty((arg.shape[0], 2 * arg.shape[1]), dtype=np.uint32)
    rec[:, 0::2], rec[:, 1::2] = arg, gbits
    return rec


def _pack(ctx, arg, gbits, layout, rows=None):
    """mggcn_agg_max_pack_f32 of (arg, G) into a fresh guarded record; returns the Guarded record"""
    n, d = arg.shape
    pads, offs = LAYOUTS[layout]
    gA = Guarded(n, d, d + pads[0], offs[0], logical=arg)
    gG = Guarded(n, d, d + pads[1], offs[1], logical=gbits)
    gR = Guarded(n, 2 * d, 2 * d + pads[3], offs[3], output=True)
    assert gR.ptr % 8 == 0 and gR.ld % 2 == 0
    ctx.lib.mggcn_agg_max_pack_f32(ctx.stream(0), gA.ptr, gA.ld, gG.ptr, gG.ld, n if rows is None else rows, d, gR.ptr, gR.ld)
    ctx.sync()
    what = f"agg max pack d={d} {layout}"
    gA.check_unchanged(what)
    gG.check_unchanged(what)
    gR.check_guards(what)
    return gR


def _backward(ctx, pat, arg, G, layout, rec, src0=0, splits=None, accumulate=None, repeat=1):
    """the backward over the sorted transpose into a fresh guarded G_B through the plain entry point or (``rec``) through the
    pack and the record entry point; ``splits``: the row ranges, each a call of its own with src0 + r0; the bits of G_B"""
    n, n_src, d = pat["n"], pat["n_src"], G.shape[1]
    pads, offs = LAYOUTS[layout]
    arg = np.ascontiguousarray(arg, dtype=np.uint32)
    gbits = np.ascontiguousarray(G, dtype=np.float32).view(np.uint32)
    gB = Guarded(n_src, d, d + pads[2], offs[2], logical=accumulate, output=True)
    tip, tix = pat["d_t_indptr"].data_ptr(), pat["d_t_indices"].data_ptr()
    flags = 1 if accumulate is not None else 0
    what = f"agg max backward{' rec' if rec else ''} d={d} {layout}"
    if rec:
        gR = _pack(ctx, arg, gbits, layout)
        assert (gR.logical_bits() == _interleave(arg, gbits)).all(), what
        before = gR.bits().copy()
    else:
        gA = Guarded(n, d, d + pads[0], offs[0], logical=arg)
        gG = Guarded(n, d, d + pads[1], offs[1], logical=gbits)
    for _ in range(repeat):
        for r0, r1 in splits or [(0, n_src)]:
            out = gB.ptr + 4 * r0 * gB.ld
            if rec:
                ctx.lib.mggcn_agg_max_backward_rec_f32(ctx.stream(0), r1 - r0, n, tip + 4 * r0, tix, gR.ptr, gR.ld, d, src0 + r0,
                                                       flags, out, gB.ld)
            else:
                ctx.lib.mggcn_agg_max_backward_f32(ctx.stream(0), r1 - r0, n, tip + 4 * r0, tix, gA.ptr, gA.ld, gG.ptr, gG.ld, d,
                                                   src0 + r0, flags, out, gB.ld)
    ctx.sync()
    if rec:
        assert (gR.bits() == before).all(), f"{what}: the record was written"
    else:
        gA.check_unchanged(what)
        gG.check_unchanged(what)
    gB.check_guards(what)
    return gB.logical_bits()


def _shift(arg, by):
    return np.where(arg == ref.NONE, ref.NONE, arg.astype(np.int64) + by).astype(np.uint32)


# ---- the pack -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", WIDTHS)
def test_pack_interleaves_the_bits_on_every_layout(ctx, d):
    """random 32-bit patterns on both sides, MGGCN_AGG_NONE, NaN payloads, infinities and signed zeros planted: words 2c and
    2c + 1 of a row are arg[i, c] and G[i, c] as they were, and nothing beyond 2 d words of a row is written"""
    n = 203                                               # more than one workgroup at every width
    rng = np.random.default_rng(d)
    arg = rng.integers(0, 1 << 32, size=(n, d), dtype=np.uint64).astype(np.uint32)
    gbits = rng.integers(0, 1 << 32, size=(n, d), dtype=np.uint64).astype(np.uint32)
    special = np.array([0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0x7F800001], dtype=np.uint32)
    for k, s in enumerate(special):
        gbits[k, (k * 5) % d] = s
        arg[k + 10, (k * 3) % d] = ref.NONE
    want = _interleave(arg, gbits)
    for layout in LAYOUTS:
        gR = _pack(ctx, arg, gbits, layout)
        got = gR.logical_bits()
        assert (got == want).all(), (d, layout, np.argwhere(got != want)[:4].tolist())
    # a row count of its own: the rows beyond it keep the fill pattern
    gR = _pack(ctx, arg, gbits, "padded", rows=7)
    got = gR.logical_bits()
    assert (got[:7] == want[:7]).all() and (got[7:] == OUT_NAN32).all()


# ---- the record backward against the plain entry point ------------------------------------------------------------------------
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("src0", [0, 77])
def test_record_backward_gives_the_plain_bits(ctx, pat, d, src0, accumulate):
    """on equally aligned operands the record call runs the plain call's (VEC, NT, U): the same bits, as one call, as three
    row ranges with src0 + r0 each, and on two repeated calls"""
    _, _, arg = _reference(pat, d)
    arg = _shift(arg, src0)
    G = np.random.default_rng(500 + d).standard_normal((pat["n"], d)).astype(np.float32)
    base = np.random.default_rng(600 + d).standard_normal((pat["n_src"], d)).astype(np.float32) if accumulate else None
    n_src = pat["n_src"]
    thirds = [(0, 11), (11, 30), (30, n_src)]
    for layout in SAME_VARIANT:
        plain = _backward(ctx, pat, arg, G, layout, False, src0, accumulate=base)
        assert np.isfinite(plain.view(np.float32)).all() and (plain != (0 if base is None else base.view(np.uint32))).any()
        for splits, repeat in ((None, 1), (thirds, 1), (None, 2)):
            want = plain if repeat == 1 else _backward(ctx, pat, arg, G, layout, False, src0, accumulate=base, repeat=repeat)
            if repeat == 2 and not accumulate:
                assert (want == plain).all()
            got = _backward(ctx, pat, arg, G, layout, True, src0, splits=splits, accumulate=base, repeat=repeat)
            assert (got == want).all(), (d, layout, src0, accumulate, splits, repeat, np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("d", WIDTHS)
def test_record_backward_is_exact_on_integer_gradients_on_every_layout(ctx, pat, d):
    _, _, arg = _reference(pat, d)
    G = _int_G((pat["n"], d), 200 + d)
    want = ref.agg_max_backward(pat["t_indptr"], pat["t_indices"], arg, G, pat["n_src"])
    assert (ref.scatter_arg(G.astype(np.float64), arg, pat["n_src"]) == want).all() and np.abs(want).max() > 0
    base = _int_G((pat["n_src"], d), 300 + d)
    for layout in LAYOUTS:
        got = _backward(ctx, pat, arg, G, layout, True).view(np.float32)
        assert (got == want).all(), f"d={d} {layout}: {np.argwhere(got != want)[:4].tolist()}"
        got = _backward(ctx, pat, _shift(arg, 77), G, layout, True, src0=77, accumulate=base,
                        splits=[(0, 11), (11, pat["n_src"])]).view(np.float32)
        assert (got == want + base).all(), f"d={d} {layout} src0 + accumulate + row ranges"
    assert (want[pat["n_src"] - 1] == 0).all()                         # the source nobody references


@pytest.mark.parametrize("layout", ["contiguous", "rec8"])
def test_a_duplicated_pair_delivers_its_gradient_once(ctx, layout):
    """one destination lists source 2 three times and source 0 once; all of its gradient goes to 2, once"""
    import torch
    t_indptr = np.array([0, 1, 1, 4], dtype=np.uint32)                # rows: source 0 -> [0], source 1 -> [], source 2 -> [0, 0, 0]
    t_indices = np.array([0, 0, 0, 0], dtype=np.uint32)
    p = dict(n=1, n_src=3, d_t_indptr=torch.from_numpy(t_indptr.view(np.int32)).cuda(),
             d_t_indices=torch.from_numpy(t_indices.view(np.int32)).cuda())
    arg = np.array([[2, 2, 0, ref.NONE]], dtype=np.uint32)
    G = np.array([[3, -5, 7, 11]], dtype=np.float32)
    got = _backward(ctx, p, arg, G, layout, True).view(np.float32)
    assert got.tolist() == [[0, 0, 7, 0], [0, 0, 0, 0], [3, -5, 0, 0]]


@pytest.mark.parametrize("d", [3, 4, 41, 128, 260])
def test_a_nan_in_an_unselected_gradient_stays_out(ctx, pat, d):
    """G[i, c] = NaN wherever nothing is selected (arg = NONE) and in every element of destination 0, whose selection is
    moved to a source that does not list it: the select keeps every NaN out of G_B"""
    _, _, arg = _reference(pat, d)
    arg = arg.copy()
    G = _int_G((pat["n"], d), 700 + d)
    G[arg == ref.NONE] = np.nan
    victim = 2                                                        # a destination with entries
    assert pat["indptr"][victim + 1] > pat["indptr"][victim]
    arg[victim] = pat["n_src"] - 1                                    # the source nobody references: no row compares equal
    G[victim] = np.nan
    assert np.isnan(G).any()
    want = ref.agg_max_backward(pat["t_indptr"], pat["t_indices"], arg, np.nan_to_num(G), pat["n_src"])
    for layout in LAYOUTS:
        got = _backward(ctx, pat, arg, G, layout, True).view(np.float32)
        assert np.isfinite(got).all() and (got == want).all(), (d, layout)


def test_no_rows_return_and_write_nothing(ctx, pat):
    d = 8
    arg = np.zeros((pat["n"], d), dtype=np.uint32)
    G = _int_G((pat["n"], d), 2)
    fill = OUT_NAN32                                                  # untouched: the fill pattern of an output
    got = _backward(ctx, pat, arg, G, "contiguous", True, splits=[(7, 7)])
    assert (got == fill).all()
    gR = _pack(ctx, arg, G.view(np.uint32), "contiguous", rows=0)
    assert (gR.logical_bits() == fill).all()
    ctx.lib.mggcn_agg_max_pack_f32(ctx.stream(0), None, d, None, d, 0, d, None, 2 * d)          # nothing is dereferenced
    ctx.lib.mggcn_agg_max_backward_rec_f32(ctx.stream(0), 0, 7, None, None, None, 2 * d, d, 0, 0, None, d)
    ctx.sync()


# ---- the wrappers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [41, 128])
def test_ops_wrappers_give_the_plain_bits(pkg, ctx, pat, d):
    import torch
    ops, dn = pkg.ops, pkg.dn_matrix
    n, n_src = pat["n"], pat["n_src"]
    _, _, arg_h = _reference(pat, d)
    F_T = pkg.csr_matrix(pat["t_indptr"].copy(), pat["t_indices"].copy(), np.ones(pat["t_indices"].size, dtype=np.float32), n)
    G_h = np.random.default_rng(d).standard_normal((n, d)).astype(np.float32)
    arg, G = dn.from_numpy(_shift(arg_h, 5).view(np.int32)), dn.from_numpy(G_h)
    plain, packed = dn.from_numpy(np.ones((n_src, d), dtype=np.float32)), dn.from_numpy(np.ones((n_src, d), dtype=np.float32))
    rec = torch.empty(n * d * 2, dtype=torch.int32, device="cuda")
    ops.agg_max_backward(ctx, F_T, arg, G, plain, accumulate=True, src0=5)
    ops.agg_max_pack(ctx, arg, G, rec)
    ops.agg_max_backward_rec(ctx, F_T, rec, d, packed, accumulate=True, src0=5)
    ctx.sync()
    assert (rec.cpu().numpy().view(np.uint32).reshape(n, 2 * d) == _interleave(_shift(arg_h, 5), G_h.view(np.uint32))).all()
    assert (packed.numpy().view(np.uint32) == plain.numpy().view(np.uint32)).all() and (plain.numpy() != 1).any()
    with pytest.raises(ValueError, match="alias"):
        ops.agg_max_backward_rec(ctx, F_T, rec, d, dn(n_src, d, rec.view(torch.float32)))
