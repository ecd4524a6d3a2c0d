"""The GAT kernels (csrc/gat.hip) where test_gpu_gat.py does not reach: every (VEC, NT, U) variant of the three sparse
kernels, rows of F^T longer than one, two and three chunks, single positions of a row probed with crafted scalars, the
running maximum of the forward under scores of +-80, and the two dense kernels at their edges.

The measure is row-scaled (gat_ref.rowdist): every element against the magnitude its own terms add up to, from the exact
fp64 restatement, at gat_ref.ROW_TOL -- eight times the fp32 twin's worst distance over the cases of (B), measured on the
CPU.  The matrix-normalised distance at TOL is asserted next to it, as test_gpu_gat.py does."""
import numpy as np
import pytest

import gat_ref as ref
from gat_ref import ROW_TOL, relerr, rowdist, rowerr
from test_gpu_gat import COLSUM_BLOCKS, TOL, _dense, _u32, run_device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


# ---- (B) every variant, on F with long rows, on F with long columns, on a rectangular block ----------------------------------------
_aligned = {}


def _edge_case(ctx, name, K, dh, **kw):
    c = ref.edge_case(name, K, dh)
    got = run_device(ctx, c["indptr"], c["indices"], c["Z"], c["att"], K, c["G"], Z_dst=c["Z_dst"], **kw)
    tag = f"[gat-edge] {name} K={K} dh={dh} {kw or ''}"
    for nm in ref.NAMES:
        want, twin = c["want"][nm], c["twin"][nm]
        dt, dg = relerr(twin, want.astype(np.float32)), relerr(got[nm], want.astype(np.float32))
        (_, rt), (row, rg) = rowerr(twin, want, c["scale"][nm]), rowerr(got[nm], want, c["scale"][nm])
        print(f"{tag} {nm}: matrix twin {dt:.3e} device {dg:.3e} | row-scaled twin {rt:.3e} device {rg:.3e} at row {row}")
        assert dt <= TOL / 3 and rt <= ROW_TOL / 8, ("the input is ill-conditioned for this bar", nm, dt, rt)
        assert dg <= TOL, (nm, K, dh, dg)
        assert rg <= ROW_TOL, (nm, K, dh, "row", row, rg, "twin:", rt)
    return got


@pytest.mark.parametrize("name,K,dh", ref.edge_cases())
def test_every_variant_row_by_row(ctx, name, K, dh):
    """all nine outputs of every (VEC, NT, U) variant (gat_ref.EDGE_SHAPES names which shape selects which) against the
    restatement, each row on its own scale: "long" has rows of 63 .. 4097 entries in F (forward, backward_dst), "longT" has
    them in F^T (backward_src), "rect" is the 200 x 320 block"""
    got = _edge_case(ctx, name, K, dh)
    if name == "long":
        _aligned[(K, dh)] = got


@pytest.mark.parametrize("K,dh", ref.EDGE_MISALIGNED)
def test_the_widest_calls_on_the_element_path(ctx, K, dh):
    """base pointers one float off and a leading dimension of d + 3: 1024 and 512 columns per head in 16 and 8 element
    tiles, against the restatement and against the float4 run of the same inputs"""
    aligned = _aligned.get((K, dh)) or _edge_case(ctx, "long", K, dh)
    off = _edge_case(ctx, "long", K, dh, offset=1, pad=3)
    c = ref.edge_case("long", K, dh)
    for nm in ref.NAMES:                            # two reduction orders of the same numbers
        assert relerr(off[nm], aligned[nm]) <= TOL, nm
        assert rowerr(off[nm], aligned[nm], c["scale"][nm])[1] <= ROW_TOL, nm


@pytest.mark.parametrize("operand", ["Z", "G", "out", "G_Z", "att"])
def test_one_misaligned_operand_is_enough_for_the_element_path(ctx, operand):
    """(4, 32) with one operand alone one float off 16-byte alignment: every kernel that touches it must leave the float4
    path (a float4 access there would be misaligned), and the results agree with the aligned run"""
    aligned = _aligned.get((4, 32)) or _edge_case(ctx, "long", 4, 32)
    off = _edge_case(ctx, "long", 4, 32, off={operand: 1})
    c = ref.edge_case("long", 4, 32)
    for nm in ref.NAMES:
        assert relerr(off[nm], aligned[nm]) <= TOL, nm
        assert rowerr(off[nm], aligned[nm], c["scale"][nm])[1] <= ROW_TOL, nm


# ---- single entry points on crafted scalars -------------------------------------------------------------------------------------------
def _forward(ctx, ip, ix, n, n_src, Zs, s_dst, s_src, K, dh):
    out, lse = _dense(n, K * dh), _dense(n, K)
    ctx.lib.mggcn_gat_forward_f32(ctx.stream(0), n, n_src, ip.data_ptr(), ix.data_ptr(), Zs.ptr, Zs.ld, s_dst.ptr, s_src.ptr, K, dh,
                                  ref.SLOPE, out.ptr, out.ld, lse.ptr)
    return out, lse


def _backward_src(ctx, tip, tix, n_src, n, Zs, s_dst, s_src, lse, D, Gd, at, K, dh):
    """over the pattern given as F^T: n_src rows that list destinations; no ds_dst term"""
    ds_src, G_Z = _dense(n_src, K), _dense(n_src, K * dh)
    ctx.lib.mggcn_gat_backward_src_f32(ctx.stream(0), n_src, n, tip.data_ptr(), tix.data_ptr(), Zs.ptr, Zs.ld, s_dst.ptr, s_src.ptr,
                                       lse.ptr, D.ptr, Gd.ptr, Gd.ld, at.ptr, None, K, dh, ref.SLOPE, ds_src.ptr, G_Z.ptr, G_Z.ld)
    return ds_src, G_Z


def _twin_first(c, names):
    for nm in names:
        rt = rowerr(c["twin"][nm], c["want"][nm], c["want"]["scale"][nm])[1]
        assert rt <= ROW_TOL / 8, ("the input is ill-conditioned for this bar", nm, rt)


@pytest.mark.parametrize("K,dh", [(4, 32), (3, 7)])
def test_forward_picks_the_entry_at_each_probed_position(ctx, K, dh):
    """(C) gat_ref.forward_probe_case: out[row] is the row of Z of the one source whose score is +40, and lse is 40, at
    positions 0, 63, 64, 127, 128, L - 2 and L - 1 of rows of 64, 65, 129, 193 and 4097 entries.  An index, a score or a
    weight attached to a neighbouring entry anywhere in the two prefetch stages gives some other row of Z"""
    c = ref.forward_probe_case(0, K, dh)
    n, n_src = c["indptr"].size - 1, c["n_src"]
    ip, ix, Zs = _u32(c["indptr"]), _u32(c["indices"]), _dense(n_src, K * dh, host=c["Z"])
    s_dst = _dense(n, K, host=np.zeros((n, K)))
    for t in range(ref.PROBE_SLOTS):
        c = ref.forward_probe_case(t, K, dh)
        want, Zhot = c["want"], c["Z"][c["hot"]]
        assert rowerr(want["out"], Zhot, want["scale"]["out"])[1] <= 1e-9           # the probe's own claim
        _twin_first(c, ("out", "lse"))
        out, lse = _forward(ctx, ip, ix, n, n_src, Zs, s_dst, _dense(n_src, K, host=c["s_src"]), K, dh)
        ctx.sync()
        d_out, d_lse = rowdist(out.numpy(), Zhot, want["scale"]["out"]), np.abs(lse.numpy() - 40.0).max(axis=1) / 40.0
        print(f"[gat-edge] forward probe K={K} dh={dh} positions {c['pos']}: out {d_out.max():.3e} lse {d_lse.max():.3e}")
        assert (d_out <= ROW_TOL).all(), (c["pos"], d_out)
        assert (d_lse <= ROW_TOL).all(), (c["pos"], d_lse)


@pytest.mark.parametrize("K,dh", [(4, 32), (3, 7)])
def test_backward_src_picks_the_entry_at_each_probed_position(ctx, K, dh):
    """(C) gat_ref.backward_src_probe_case, the same on the transposed side: G_Z[j] is G of the one destination with
    e - lse = 0 and ds_src[j, k] = slope (G_p . Z_j)[head k] -- index, s_dst, lse and D of an entry stay together through
    the prefetch"""
    c = ref.backward_src_probe_case(0, K, dh)
    n, n_src = c["n"], c["n_src"]
    zeros = np.zeros((n, K), dtype=np.float32)
    tip, tix = _u32(c["t_indptr"]), _u32(c["t_indices"])
    Zs, Gd, at = _dense(n_src, K * dh, host=c["Z"]), _dense(n, K * dh, host=c["G"]), _dense(2, K * dh, host=np.zeros((2, K * dh)))
    s_src, lse, D = _dense(n_src, K, host=np.zeros((n_src, K))), _dense(n, K, host=zeros), _dense(n, K, host=zeros)
    for t in range(ref.PROBE_SLOTS):
        c = ref.backward_src_probe_case(t, K, dh)
        want, Ghot = c["want"], c["G"][c["hot"]]
        assert rowerr(want["G_Z"], Ghot, want["scale"]["G_Z"])[1] <= 1e-9          # the probe's own claims
        assert rowerr(want["ds_src"], c["dots"], want["scale"]["ds_src"])[1] <= 1e-9
        _twin_first(c, ("G_Z", "ds_src"))
        ds_src, G_Z = _backward_src(ctx, tip, tix, n_src, n, Zs, _dense(n, K, host=c["s_dst"]), s_src, lse, D, Gd, at, K, dh)
        ctx.sync()
        d_gz = rowdist(G_Z.numpy(), Ghot, want["scale"]["G_Z"])
        d_ds = rowdist(ds_src.numpy(), c["dots"], want["scale"]["ds_src"])
        print(f"[gat-edge] backward_src probe K={K} dh={dh} positions {c['pos']}: G_Z {d_gz.max():.3e} ds_src {d_ds.max():.3e}")
        assert (d_gz <= ROW_TOL).all(), (c["pos"], d_gz)
        assert (d_ds <= ROW_TOL).all(), (c["pos"], d_ds)


@pytest.mark.parametrize("kind", ref.STRESS_KINDS)
@pytest.mark.parametrize("K,dh", [(4, 32), (3, 7)])
def test_running_maximum_under_stress(ctx, K, dh, kind):
    """(D) scores of -80 .. +80 laid out along rows of 64 .. 4097 entries (gat_ref.stress_scores): out and lse of the
    one-pass forward against the restatement fed the same fp32 scalars, the weights recomputed in fp64 from the device's
    lse add up to one, and backward_dst and backward_src on the same scalars give the restatement's D, ds_dst, ds_src, G_Z"""
    c = ref.stress_case(kind, K, dh)
    indptr, indices, n_src, want = c["indptr"], c["indices"], c["n_src"], c["want"]
    n, d = indptr.size - 1, K * dh
    names = ("out", "lse", "D", "ds_dst", "ds_src", "G_Z")
    _twin_first(c, names[:4])
    lib, st = ctx.lib, ctx.stream(0)
    ip, ix = _u32(indptr), _u32(indices)
    tip, tix = (_u32(a) for a in ref.transpose_pattern(indptr, indices, n_src))
    Zs, Gd, at = _dense(n_src, d, host=c["Z"]), _dense(n, d, host=c["G"]), _dense(2, d, host=c["att"])
    s_dst, s_src, D, ds_dst = _dense(n, K, host=np.zeros((n, K))), _dense(n_src, K, host=c["s_src"]), _dense(n, K), _dense(n, K)
    out, lse = _forward(ctx, ip, ix, n, n_src, Zs, s_dst, s_src, K, dh)
    lib.mggcn_gat_backward_dst_f32(st, n, n_src, ip.data_ptr(), ix.data_ptr(), Zs.ptr, Zs.ld, s_dst.ptr, s_src.ptr, lse.ptr, Gd.ptr,
                                   Gd.ld, out.ptr, out.ld, K, dh, ref.SLOPE, D.ptr, ds_dst.ptr)
    ds_src, G_Z = _backward_src(ctx, tip, tix, n_src, n, Zs, s_dst, s_src, lse, D, Gd, at, K, dh)
    ctx.sync()
    got = dict(zip(names, (out.numpy(), lse.numpy(), D.numpy(), ds_dst.numpy(), ds_src.numpy(), G_Z.numpy())))
    total = ref.alpha_row_sums(indptr, indices, c["s_src"], got["lse"])
    print(f"[gat-edge] stress {kind} K={K} dh={dh}: |sum alpha - 1| {np.abs(total - 1).max():.3e}")
    assert np.abs(total - 1).max() <= ROW_TOL, total
    for nm in names:
        row, dist = rowerr(got[nm], want[nm], want["scale"][nm])
        print(f"[gat-edge] stress {kind} K={K} dh={dh} {nm}: row-scaled {dist:.3e} at row {row}")
        assert np.isfinite(got[nm]).all(), nm
        assert dist <= ROW_TOL, (nm, kind, row, dist)


# ---- (E) the two dense kernels --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,dh,rows,offset,pad", [
    (16, 1, 37, 0, 0),          # 64 one-lane groups, 16 of them with a head
    (16, 64, 37, 0, 0),         # one group, sixteen turns
    (1, 1024, 37, 0, 0),        # the stride loop runs sixteen times over the 64 lanes
    (3, 7, 37, 1, 5),           # ldz = d + 5 from a base one float off
    (1, 1024, 5, 3, 5),
])
def test_scores_at_the_edges(ctx, K, dh, rows, offset, pad):
    d = K * dh
    rng = np.random.default_rng(41 + d)
    Z = rng.standard_normal((rows, d), dtype=np.float32)
    att = rng.standard_normal((2, d)).astype(np.float32)
    Zs, at = _dense(rows, d, offset, pad, Z), _dense(2, d, offset, 0, att)
    prod = Z.astype(np.float64).reshape(rows, 1, K, dh) * att.astype(np.float64).reshape(1, 2, K, dh)
    want, scale = prod.sum(axis=3), np.abs(prod).sum(axis=3)                     # [rows, 2, K]
    for which in ("both", "dst", "src"):
        s_dst, s_src = _dense(rows, K), _dense(rows, K)
        ctx.lib.mggcn_gat_scores_f32(ctx.stream(0), Zs.ptr, Zs.ld, at.ptr, s_dst.ptr if which != "src" else None,
                                     s_src.ptr if which != "dst" else None, rows, K, dh)
        ctx.sync()
        for side, buf in enumerate((s_dst, s_src)):
            if which in ("both", ("dst", "src")[side]):
                row, dist = rowerr(buf.numpy(), want[:, side], scale[:, side])
                print(f"[gat-edge] scores K={K} dh={dh} {which} side {side}: {dist:.3e} at row {row}")
                assert dist <= ROW_TOL, (which, side, row, dist)
            else:                                   # not requested: still the fill value
                np.testing.assert_array_equal(buf.numpy(), np.full((rows, K), 123.0, dtype=np.float32))


def _scores_backward_case(ctx, K, dh, n_dst, n_src, first=0, pad=0, offset=0):
    """G_att of ds and Z with n_dst / n_src rows (ds zero in the rows before ``first``) against the fp64 column sums, each
    column on the scale of the sum of its |terms|; a side without rows is passed as NULL and must come out as zeros"""
    d = K * dh
    rng = np.random.default_rng(51 + d + n_dst)
    want, scale, ptrs, keep = np.zeros((2, d)), np.zeros((2, d)), [], []
    for side, n in enumerate((n_dst, n_src)):
        if not n:
            ptrs += [None, None, d]
            continue
        ds, Z = rng.standard_normal((n, K)).astype(np.float32), rng.standard_normal((n, d), dtype=np.float32)
        ds[:first] = 0
        terms = np.repeat(ds.astype(np.float64), dh, axis=1) * Z
        want[side], scale[side] = terms.sum(axis=0), np.abs(terms).sum(axis=0)
        dsd, Zd = _dense(n, K, host=ds), _dense(n, d, offset, pad, Z)
        keep += [dsd, Zd]
        ptrs += [dsd.ptr, Zd.ptr, Zd.ld]
    G_att = _dense(2, d)
    ctx.lib.mggcn_gat_scores_backward_f32(ctx.stream(0), ptrs[0], ptrs[1], ptrs[2], n_dst, ptrs[3], ptrs[4], ptrs[5], n_src, K, dh,
                                          G_att.ptr)
    ctx.sync()
    side, dist = rowerr(G_att.numpy(), want, scale)
    print(f"[gat-edge] scores_backward K={K} dh={dh} n_dst={n_dst} n_src={n_src} first={first}: {dist:.3e} (side {side})")
    assert dist <= ROW_TOL, (K, dh, n_dst, n_src, side, dist)


@pytest.mark.parametrize("K,dh", [(1, 1), (3, 4), (3, 85), (16, 16), (1, 257), (2, 512)])
@pytest.mark.parametrize("n_dst,n_src", [(37, 0), (0, 41), (37, 300), (300, 37)])
def test_scores_backward_at_the_edges(ctx, K, dh, n_dst, n_src):
    """widths 1, 12, 255, 256, 257 and 1024: 1 to 256 threads per row (R = 256 .. 1 rows per turn), one to four column
    turns with a partly masked last turn at 257; two sides of different lengths, one of them without rows; row counts that
    are no multiple of R"""
    _scores_backward_case(ctx, K, dh, n_dst, n_src)


def test_scores_backward_beyond_one_pass_at_width_one(ctx):
    """width 1 takes R = 256 rows per workgroup and turn, so one pass of the capped grid covers 256 * COLSUM_BLOCKS rows;
    only the rows beyond it carry a non-zero ds (as test_gpu_gat.py (9) does at width 128), with a last turn that is not full"""
    first = 256 * COLSUM_BLOCKS
    _scores_backward_case(ctx, 1, 1, first + 300, first + 77, first=first)
    _scores_backward_case(ctx, 3, 85, 37, 2 * COLSUM_BLOCKS + 3, pad=5, offset=1)
