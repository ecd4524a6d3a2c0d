"""The packed destination record on the device (include/mggcn.h: mggcn_gat_pack_dst_f32, mggcn_gat_backward_src_rec_f32,
mggcn_gat_backward_src_rec_drop_f32): the pack is exact, and backward_src on the record gives the bits of the plain call on
the arrays the record was packed from -- on every (VEC, NT, U) variant, over F^T = kernel_graph_long (rows of 0 .. 4097
entries) and over the 200 x 320 block, with attention dropout at non-zero offsets, and on misaligned dense operands.  The
record's fourth float is NaN in every run: nothing may read it."""
import numpy as np
import pytest

import gat_dropout_ref as dref
import gat_ref as ref
from test_gpu_gat import _dense, _u32

pytestmark = pytest.mark.gpu

# one shape of gat_ref.EDGE_SHAPES per compiled variant, then the two layer shapes of the flagship epoch
VARIANT_SHAPES = [(2, 20), (1, 260), (3, 7), (1, 130), (1, 257)]
SHAPES = VARIANT_SHAPES + [(4, 32), (1, 41)]
GRAPHS = ("longT", "rect")
SENTINEL = 123.0
DST0, SRC0 = dref.RECT_DST0, dref.RECT_SRC0


def test_the_shapes_reach_every_variant():
    assert all(s in ref.EDGE_SHAPES for s in VARIANT_SHAPES)
    got = {ref.head_geometry_for(dh, dh % 4 == 0)[0] for _, dh in VARIANT_SHAPES}
    assert got == {(4, 1, 4), (4, 4, 1), (1, 1, 4), (1, 4, 2), (1, 16, 1)}
    indptr, indices, n_src = ref.edge_graphs()["longT"]
    lens = np.diff(ref.transpose_pattern(indptr, indices, n_src)[0].astype(np.int64))
    assert set(ref.LONG_ROWS.values()) <= set(lens.tolist())            # backward_src walks the rows of 0 .. 4097 entries


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


def _torch():
    import torch
    return torch


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _run(ctx, name, K, dh, drop=None, off=None, pad=0, spoil=None):
    """scores, forward and backward_dst through the plain (or _drop) entry points, then backward_src three ways on the same
    operands: plain, on the record, on the record again.  ``off``: {"Z" | "G" | "G_Z": floats} moves that operand's base;
    ``spoil``: index of the record float (0 .. 2) that gets 1 added before the record call.  Returns host copies."""
    torch = _torch()
    lib, st = ctx.lib, ctx.stream(0)
    indptr, indices, n_src = ref.edge_graphs()[name]
    n = indptr.size - 1
    square = n == n_src
    d = K * dh
    Z, Z_dst, G, att = ref.tolerance_inputs(n, n_src, K, dh, att_scale=0.1 * min(1.0, (32.0 / dh) ** 0.5))
    t_indptr, t_indices = ref.transpose_pattern(indptr, indices, n_src)
    ip, ix, tip, tix = _u32(indptr), _u32(indices), _u32(t_indptr), _u32(t_indices)
    o = dict(dict.fromkeys(("Z", "G", "G_Z"), 0), **(off or {}))
    Zs = _dense(n_src, d, o["Z"], pad, Z)
    Zd = Zs if square else _dense(n, d, o["Z"], pad, Z_dst)
    Gd, at, out = _dense(n, d, o["G"], pad, G), _dense(2, d, 0, 0, att), _dense(n, d, 0, pad)
    s_dst, lse, D, ds_dst = (_dense(n, K) for _ in range(4))
    s_src = _dense(n_src, K)
    rec = torch.full((n * K * 4 + 8,), SENTINEL, dtype=torch.float32, device="cuda")
    assert rec.data_ptr() % 16 == 0
    extra = () if drop is None else tuple(drop)
    sfx = "" if drop is None else "_drop"
    torch.cuda.synchronize()
    if square:
        lib.mggcn_gat_scores_f32(st, Zs.ptr, Zs.ld, at.ptr, s_dst.ptr, s_src.ptr, n_src, K, dh)
    else:
        lib.mggcn_gat_scores_f32(st, Zd.ptr, Zd.ld, at.ptr, s_dst.ptr, None, n, K, dh)
        lib.mggcn_gat_scores_f32(st, Zs.ptr, Zs.ld, at.ptr, None, s_src.ptr, n_src, K, dh)
    getattr(lib, f"mggcn_gat_forward{sfx}_f32")(st, n, n_src, ip.data_ptr(), ix.data_ptr(), Zs.ptr, Zs.ld, s_dst.ptr, s_src.ptr, K,
                                                dh, ref.SLOPE, out.ptr, out.ld, lse.ptr, *extra)
    getattr(lib, f"mggcn_gat_backward_dst{sfx}_f32")(st, n, n_src, ip.data_ptr(), ix.data_ptr(), Zs.ptr, Zs.ld, s_dst.ptr,
                                                     s_src.ptr, lse.ptr, Gd.ptr, Gd.ld, out.ptr, out.ld, K, dh, ref.SLOPE, D.ptr,
                                                     ds_dst.ptr, *extra)
    lib.mggcn_gat_pack_dst_f32(st, s_dst.ptr, lse.ptr, D.ptr, n, K, rec.data_ptr())
    ctx.sync()
    packed = rec.cpu().numpy().copy()
    body = rec[:n * K * 4].view(n * K, 4)
    body[:, 3] = float("nan")                                               # nothing may read the fourth float
    if spoil is not None:
        body[:, spoil] += 1.0
    torch.cuda.synchronize()
    dd = ds_dst.ptr if square else None
    res = dict(n=n, n_src=n_src, packed=packed, s_dst=s_dst.numpy(), lse=lse.numpy(), D=D.numpy())
    for key in ("plain", "rec", "again"):
        ds_src, G_Z = _dense(n_src, K), _dense(n_src, d, o["G_Z"], pad)
        torch.cuda.synchronize()
        if key == "plain":
            getattr(lib, f"mggcn_gat_backward_src{sfx}_f32")(st, n_src, n, tip.data_ptr(), tix.data_ptr(), Zs.ptr, Zs.ld, s_dst.ptr,
                                                             s_src.ptr, lse.ptr, D.ptr, Gd.ptr, Gd.ld, at.ptr, dd, K, dh, ref.SLOPE,
                                                             ds_src.ptr, G_Z.ptr, G_Z.ld, *extra)
        else:
            getattr(lib, f"mggcn_gat_backward_src_rec{sfx}_f32")(st, n_src, n, tip.data_ptr(), tix.data_ptr(), Zs.ptr, Zs.ld,
                                                                 rec.data_ptr(), s_src.ptr, Gd.ptr, Gd.ld, at.ptr, dd, K, dh,
                                                                 ref.SLOPE, ds_src.ptr, G_Z.ptr, G_Z.ld, *extra)
        ctx.sync()
        res[key] = (ds_src.numpy(), G_Z.numpy(), G_Z.flat.cpu().numpy().copy())
    return res


def _assert_pack_exact(r, K):
    n = r["n"]
    body = r["packed"][:n * K * 4].reshape(n, K, 4)
    for i, nm in enumerate(("s_dst", "lse", "D")):
        np.testing.assert_array_equal(_bits(body[:, :, i]), _bits(r[nm]), err_msg=nm)
    np.testing.assert_array_equal(_bits(body[:, :, 3]), np.zeros((n, K), dtype=np.uint32))          # +0.0
    np.testing.assert_array_equal(r["packed"][n * K * 4:], np.full(8, SENTINEL, dtype=np.float32))   # and not a float further


def _assert_same_bits(r, what):
    for key in ("rec", "again"):
        for i, nm in enumerate(("ds_src", "G_Z", "the whole G_Z allocation")):
            np.testing.assert_array_equal(_bits(r[key][i]), _bits(r["plain"][i]), err_msg=f"{what} {key} {nm}")
    assert np.isfinite(r["plain"][0]).all() and np.isfinite(r["plain"][1]).all()          # the NaN went nowhere
    assert np.abs(r["plain"][1]).max() > 0 and np.abs(r["plain"][0]).max() > 0


@pytest.mark.parametrize("name", GRAPHS)
@pytest.mark.parametrize("K,dh", SHAPES)
def test_record_call_gives_the_plain_bits(ctx, name, K, dh):
    """pack_dst is exact, and backward_src_rec gives the bits of backward_src in ds_src and G_Z, twice"""
    r = _run(ctx, name, K, dh)
    _assert_pack_exact(r, K)
    _assert_same_bits(r, (name, K, dh))


@pytest.mark.parametrize("name", GRAPHS)
@pytest.mark.parametrize("K,dh", SHAPES)
def test_record_drop_call_gives_the_plain_drop_bits(ctx, name, K, dh):
    """the _drop twins at p = 0.5 with dst0 = 1000 and src0 = 70000"""
    drop = dref.drop_tuple(0.5, dref.SEED, dref.STREAM, DST0, SRC0)
    r = _run(ctx, name, K, dh, drop=drop)
    _assert_pack_exact(r, K)
    _assert_same_bits(r, (name, K, dh, "drop"))
    plain = _run(ctx, name, K, dh)
    assert (_bits(plain["plain"][1]) != _bits(r["plain"][1])).any()             # and the mask does something


@pytest.mark.parametrize("which", ["G", "Z", "G_Z"])
@pytest.mark.parametrize("drop", [False, True])
def test_misaligned_operands_take_the_element_path_with_the_same_bits(ctx, which, drop):
    """(4, 32) with G, Z or G_Z alone one float off 16-byte alignment: the element path of both calls (each operand is one
    term of the launcher's float4 condition), the same bits on the same operands"""
    d = dref.drop_tuple(0.5, dref.SEED, dref.STREAM, DST0, SRC0) if drop else None
    r = _run(ctx, "longT", 4, 32, drop=d, off={which: 1})
    _assert_same_bits(r, (which, drop))
    aligned = _run(ctx, "longT", 4, 32, drop=d)
    assert ref.relerr(r["plain"][1], aligned["plain"][1]) <= 1e-4                # another order of the same sums


@pytest.mark.parametrize("spoil", [0, 1, 2])
def test_the_record_is_what_the_kernel_reads(ctx, spoil):
    """one added to s_dst, lse or D inside the record alone moves the record call's outputs: the three scalars come from it"""
    r = _run(ctx, "longT", 4, 32, spoil=spoil)
    assert (_bits(r["rec"][0]) != _bits(r["plain"][0])).any()
    np.testing.assert_array_equal(_bits(r["rec"][1]), _bits(r["again"][1]))


def test_no_rows_launches_nothing(ctx):
    torch = _torch()
    lib, st = ctx.lib, ctx.stream(0)
    rec = torch.full((64,), SENTINEL, dtype=torch.float32, device="cuda")
    ds_src, G_Z = _dense(4, 4), _dense(4, 16)
    torch.cuda.synchronize()
    lib.mggcn_gat_pack_dst_f32(st, None, None, None, 0, 4, rec.data_ptr())
    lib.mggcn_gat_backward_src_rec_f32(st, 0, 7, None, None, None, 16, rec.data_ptr(), None, None, 16, None, None, 4, 4, ref.SLOPE,
                                       ds_src.ptr, G_Z.ptr, 16)
    lib.mggcn_gat_backward_src_rec_drop_f32(st, 0, 7, None, None, None, 16, rec.data_ptr(), None, None, 16, None, None, 4, 4,
                                            ref.SLOPE, ds_src.ptr, G_Z.ptr, 16, *dref.drop_tuple(0.5, 1, 2, 3, 4))
    ctx.sync()
    for t in (rec, ds_src.flat, G_Z.flat):
        assert (t.cpu().numpy() == SENTINEL).all()
