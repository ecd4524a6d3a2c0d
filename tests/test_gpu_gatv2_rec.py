"""The packed (lse, D) record of GATv2 on the device (include/mggcn.h: mggcn_gatv2_pack_dst_f32,
mggcn_gatv2_backward_src_rec_f32): the pack is exact and writes nothing beyond its records, and backward_src on the record
gives the bits of the plain call on the arrays the record was packed from -- on every (VEC, NT, U) variant, over F^T =
kernel_graph_long (rows of 0 .. 4097 entries) and over the 200 x 320 block, in the model's halves layout, on misaligned dense
operands and on a row range passed as a call of its own."""
import numpy as np
import pytest

import gat_ref as ref
import gatv2_ref as v2
from test_gpu_gat import _dense, _u32

pytestmark = pytest.mark.gpu

# one shape per compiled variant (gatv2_ref.RECT_SHAPES, which holds (4, 32)), then the last layer of the flagship epoch
SHAPES = v2.RECT_SHAPES + [(1, 41)]
GRAPHS = ("longT", "rect")
SENTINEL = 123.0


def test_the_shapes_reach_every_variant(pkg):
    assert {"mggcn_gatv2_pack_dst_f32", "mggcn_gatv2_backward_src_rec_f32"} <= set(pkg._lib.PROTOTYPES)     # what the shapes are for
    assert (4, 32) in SHAPES and (1, 41) in SHAPES
    got = {ref.head_geometry_for(dh, dh % 4 == 0)[0] for _, dh in v2.RECT_SHAPES}
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


class _half:
    """one half of a [rows x 2 d] device buffer, with the interface of test_gpu_gat._dense"""

    def __init__(self, whole, d, half):
        self.whole, self.d, self.ld, self.ptr, self.half, self.flat = whole, d, whole.ld, whole.ptr + 4 * d * half, half, whole.flat

    def numpy(self):
        return self.whole.numpy()[:, self.half * self.d:(self.half + 1) * self.d].copy()


def _run(ctx, name, K, dh, halves=False, off=None, pad=0, spoil=None, nan_plain=False, t_rows=None):
    """forward and backward_dst through the plain entry points, the pack, then backward_src three ways on the same operands:
    plain, on the record, on the record again.  ``halves``: Zs | Zd and G_Zs | G_Zd as the halves of one [n x 2 d] buffer
    each (the square graph); ``off``: {"Zs" | "Zd" | "G" | "G_Zs": floats} moves that operand's base, ``pad``: every leading
    dimension is d + pad; ``spoil``: index of the record float (0, 1) that gets 1 added before the record calls;
    ``nan_plain``: lse and D are filled with NaN before the record calls; ``t_rows`` = (r0, r1): the record calls take that
    row range of F^T only.  Returns host copies."""
    torch = _torch()
    lib, st = ctx.lib, ctx.stream(0)
    indptr, indices, n_src = ref.edge_graphs()[name]
    n = indptr.size - 1
    d = K * dh
    Zs_h, Zd_h, G_h, att_h = v2.inputs(n, n_src, K, dh)
    t_indptr, t_indices = ref.transpose_pattern(indptr, indices, n_src)
    ip, ix, tip, tix = _u32(indptr), _u32(indices), _u32(t_indptr), _u32(t_indices)
    o = dict(dict.fromkeys(("Zs", "Zd", "G", "G_Zs"), 0), **(off or {}))
    if halves:
        assert n == n_src
        Z2 = _dense(n, 2 * d, 0, 0, np.concatenate([Zs_h, Zd_h], axis=1))
        Zs, Zd = _half(Z2, d, 0), _half(Z2, d, 1)
    else:
        Zs, Zd = _dense(n_src, d, o["Zs"], pad, Zs_h), _dense(n, d, o["Zd"], pad, Zd_h)
    G, att, out = _dense(n, d, o["G"], pad, G_h), _dense(1, d, 0, 0, att_h), _dense(n, d, 0, pad)
    G_Zd, P, lse, D = _dense(n, d, 0, pad), _dense(n, d, 0, pad), _dense(n, K), _dense(n, K)
    rec = torch.full((n * K * 2 + 8,), SENTINEL, dtype=torch.float32, device="cuda")
    assert rec.data_ptr() % 8 == 0
    torch.cuda.synchronize()
    lib.mggcn_gatv2_forward_f32(st, n, n_src, ip.data_ptr(), ix.data_ptr(), Zs.ptr, Zs.ld, Zd.ptr, Zd.ld, att.ptr, K, dh,
                                ref.SLOPE, out.ptr, out.ld, lse.ptr)
    lib.mggcn_gatv2_backward_dst_f32(st, n, n_src, ip.data_ptr(), ix.data_ptr(), Zs.ptr, Zs.ld, Zd.ptr, Zd.ld, att.ptr, lse.ptr,
                                     G.ptr, G.ld, out.ptr, out.ld, K, dh, ref.SLOPE, D.ptr, G_Zd.ptr, G_Zd.ld, P.ptr, P.ld)
    lib.mggcn_gatv2_pack_dst_f32(st, lse.ptr, D.ptr, n, K, rec.data_ptr())
    ctx.sync()
    res = dict(n=n, n_src=n_src, packed=rec.cpu().numpy().copy(), lse=lse.numpy(), D=D.numpy())
    r0, r1 = t_rows if t_rows is not None else (0, n_src)
    for key in ("plain", "rec", "again"):
        if halves:
            G_Zs = _half(_dense(n, 2 * d), d, 0)
        else:
            G_Zs = _dense(n_src, d, o["G_Zs"], pad)
        if key == "rec":
            if spoil is not None:
                rec[:n * K * 2].view(n * K, 2)[:, spoil] += 1.0
            if nan_plain:
                lse.flat.fill_(float("nan"))
                D.flat.fill_(float("nan"))
        torch.cuda.synchronize()
        if key == "plain":
            lib.mggcn_gatv2_backward_src_f32(st, n_src, n, tip.data_ptr(), tix.data_ptr(), Zs.ptr, Zs.ld, Zd.ptr, Zd.ld, att.ptr,
                                             lse.ptr, D.ptr, G.ptr, G.ld, K, dh, ref.SLOPE, G_Zs.ptr, G_Zs.ld)
        else:
            lib.mggcn_gatv2_backward_src_rec_f32(st, r1 - r0, n, tip.data_ptr() + 4 * r0, tix.data_ptr(), Zs.ptr + 4 * r0 * Zs.ld,
                                                 Zs.ld, Zd.ptr, Zd.ld, att.ptr, rec.data_ptr(), G.ptr, G.ld, K, dh, ref.SLOPE,
                                                 G_Zs.ptr + 4 * r0 * G_Zs.ld, G_Zs.ld)
        ctx.sync()
        res[key] = (G_Zs.numpy(), G_Zs.flat.cpu().numpy().copy())
    return res


def _assert_pack_exact(r, K):
    n = r["n"]
    body = r["packed"][:n * K * 2].reshape(n, K, 2)
    for i, nm in enumerate(("lse", "D")):
        np.testing.assert_array_equal(_bits(body[:, :, i]), _bits(r[nm]), err_msg=nm)
    np.testing.assert_array_equal(r["packed"][n * K * 2:], np.full(8, SENTINEL, dtype=np.float32))   # and not a float further


def _assert_same_bits(r, what):
    for key in ("rec", "again"):
        for i, nm in enumerate(("G_Zs", "the whole G_Zs allocation")):
            np.testing.assert_array_equal(_bits(r[key][i]), _bits(r["plain"][i]), err_msg=f"{what} {key} {nm}")
    assert np.isfinite(r["plain"][0]).all() and np.abs(r["plain"][0]).max() > 0


@pytest.mark.parametrize("name", GRAPHS)
@pytest.mark.parametrize("K,dh", SHAPES)
def test_record_call_gives_the_plain_bits(ctx, name, K, dh):
    """pack_dst is exact and stops at n K 2 floats, and backward_src_rec gives the bits of backward_src in G_Zs, twice"""
    r = _run(ctx, name, K, dh)
    _assert_pack_exact(r, K)
    _assert_same_bits(r, (name, K, dh))


def test_pack_copies_bit_patterns(ctx):
    """NaN payloads, infinities and signed zeros go through the pack as they are"""
    torch = _torch()
    n, K = 37, 3
    bits = np.random.default_rng(1).integers(0, 1 << 32, size=(2, n, K), dtype=np.uint64).astype(np.uint32)
    bits[0, 0, 0], bits[1, 0, 0], bits[0, 1, 0], bits[1, 1, 0] = 0x7FC00001, 0x80000000, 0xFF800000, 0xFFC12345
    lse, D = (torch.from_numpy(b.view(np.int32)).cuda() for b in bits)
    rec = torch.full((n * K * 2 + 8,), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.lib.mggcn_gatv2_pack_dst_f32(ctx.stream(0), lse.data_ptr(), D.data_ptr(), n, K, rec.data_ptr())
    ctx.sync()
    got = rec.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(got[:n * K * 2].reshape(n, K, 2), np.stack([bits[0], bits[1]], axis=2))
    np.testing.assert_array_equal(rec.cpu().numpy()[n * K * 2:], np.full(8, SENTINEL, dtype=np.float32))


@pytest.mark.parametrize("K,dh", [(4, 32), (3, 7)])
def test_the_halves_layout_gives_the_bits_of_separate_buffers(ctx, K, dh):
    """Zs | Zd and G_Zs | G_Zd as the halves of one [n x 2 out] buffer each (ld = 2 out, the model's layout): the record call
    has the plain call's bits, which are those of separate buffers (the same variant: the halves keep their alignment)"""
    r = _run(ctx, "longT", K, dh, halves=True)
    _assert_same_bits(r, ("halves", K, dh))
    apart = _run(ctx, "longT", K, dh)
    np.testing.assert_array_equal(_bits(r["rec"][0]), _bits(apart["plain"][0]))


@pytest.mark.parametrize("which", ["Zs", "Zd", "G", "G_Zs"])
def test_misaligned_operands_take_the_element_path_with_the_same_bits(ctx, which):
    """(4, 32) with Zs, Zd, G or G_Zs alone one float off 16-byte alignment and every leading dimension d + 3: the element
    path of both calls (each operand is one term of the launcher's float4 condition), the same bits on the same operands"""
    r = _run(ctx, "longT", 4, 32, off={which: 1}, pad=3)
    _assert_same_bits(r, which)
    aligned = _run(ctx, "longT", 4, 32)
    assert ref.relerr(r["plain"][0], aligned["plain"][0]) <= 1e-4                # another order of the same sums
    one = _run(ctx, "longT", 4, 32, off={which: 1})                             # the base alone, ld = d
    _assert_same_bits(one, (which, "ld = d"))


@pytest.mark.parametrize("spoil", [0, 1])
def test_the_record_is_what_the_kernel_reads(ctx, spoil):
    """one added to lse or D inside the record alone moves the record call's G_Zs: both floats come from it"""
    r = _run(ctx, "longT", 4, 32, spoil=spoil)
    assert (_bits(r["rec"][0]) != _bits(r["plain"][0])).any()
    np.testing.assert_array_equal(_bits(r["rec"][0]), _bits(r["again"][0]))


@pytest.mark.parametrize("K,dh", [(4, 32), (3, 7)])
def test_the_plain_arrays_are_not_read(ctx, K, dh):
    """lse and D filled with NaN after the pack: the record call still gives the plain call's bits"""
    r = _run(ctx, "longT", K, dh, nan_plain=True)
    _assert_same_bits(r, ("NaN in lse and D", K, dh))


@pytest.mark.parametrize("name,K,dh", [("longT", 4, 32), ("longT", 3, 7), ("rect", 2, 65)])
def test_a_row_range_gives_the_whole_calls_rows(ctx, name, K, dh):
    """rows [5, 13) of F^T passed as a record call of their own on a G_Zs pre-filled with 123.0: the rows of the range carry
    the whole call's bits and every other row keeps its 123.0"""
    r = _run(ctx, name, K, dh, t_rows=(5, 13))
    for key in ("rec", "again"):
        np.testing.assert_array_equal(_bits(r[key][0][5:13]), _bits(r["plain"][0][5:13]), err_msg=key)
        assert (np.delete(r[key][0], np.arange(5, 13), axis=0) == SENTINEL).all(), key
    assert np.abs(r["plain"][0][5:13]).max() > 0


def test_no_rows_launches_nothing(ctx):
    torch = _torch()
    lib, st = ctx.lib, ctx.stream(0)
    rec = torch.full((64,), SENTINEL, dtype=torch.float32, device="cuda")
    G_Zs = _dense(4, 16)
    torch.cuda.synchronize()
    lib.mggcn_gatv2_pack_dst_f32(st, None, None, 0, 4, rec.data_ptr())
    lib.mggcn_gatv2_backward_src_rec_f32(st, 0, 7, None, None, None, 16, None, 16, None, rec.data_ptr(), None, 16, 4, 4, ref.SLOPE,
                                         G_Zs.ptr, 16)
    ctx.sync()
    for t in (rec, G_Zs.flat):
        assert (t.cpu().numpy() == SENTINEL).all()


def test_ops_wrappers_give_the_plain_bits_and_refuse_a_bad_record(pkg, ctx):
    """ops.gatv2_pack_dst + ops.gatv2_backward_src_rec on dn_matrix operands against ops.gatv2_backward_src, on the halves
    layout; a misaligned record and one of the wrong length raise ValueError (the library would print and exit)"""
    torch = _torch()
    ops, dn = pkg.ops, pkg.dn_matrix
    K, dh = 4, 32
    d = K * dh
    indptr, indices, n_src = ref.edge_graphs()["longT"]
    n = indptr.size - 1
    Zs_h, Zd_h, G_h, att_h = v2.inputs(n, n_src, K, dh)
    F = pkg.csr_matrix(indptr.copy(), indices.copy(), np.ones(indices.size, dtype=np.float32), n_src)
    F_T = F.transpose()
    Z2, G, att = dn.from_numpy(np.concatenate([Zs_h, Zd_h], axis=1)), dn.from_numpy(G_h), dn.from_numpy(att_h)
    out, lse, D, P = dn(n, d), dn(n, K), dn(n, K), dn(n, d)
    plain, packed = dn(n, 2 * d), dn(n, 2 * d)
    rec = torch.empty(n * K * 2, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ops.gatv2_forward(ctx, F, Z2, Z2, att, out, lse, K)
    for G_Z2 in (plain, packed):
        ops.gatv2_backward_dst(ctx, F, Z2, Z2, att, lse, G, out, D, G_Z2, P, K)
    ops.gatv2_backward_src(ctx, F_T, Z2, Z2, att, lse, D, G, plain, K)
    ops.gatv2_pack_dst(ctx, lse, D, rec)
    ops.gatv2_backward_src_rec(ctx, F_T, Z2, Z2, att, rec, G, packed, K)
    ctx.sync()
    np.testing.assert_array_equal(_bits(packed.numpy()), _bits(plain.numpy()))
    assert np.abs(plain.numpy()[:, :d]).max() > 0 and np.abs(plain.numpy()[:, d:]).max() > 0
    off = torch.empty(n * K * 2 + 1, dtype=torch.float32, device="cuda")[1:]
    assert off.data_ptr() % 8 == 4
    short = torch.empty(n * K * 2 - 2, dtype=torch.float32, device="cuda")
    for bad, match in ((off, "aligned"), (short, "records")):
        with pytest.raises(ValueError, match=match):
            ops.gatv2_pack_dst(ctx, lse, D, bad)
        with pytest.raises(ValueError, match=match):
            ops.gatv2_backward_src_rec(ctx, F_T, Z2, Z2, att, bad, G, packed, K)
    ctx.sync()
