"""Edge features in the GAT score on the device (include/mggcn.h: mggcn_gat_*_efeat_f32 and their _drop twins; gat(edge_attr=E)):
(1) the three entries against the fp64 restatement of gat_efeat_ref.py at the bars fixed on the CPU, (2) a zero att_edge
gives the plain entries' bits, (3) every entry reads its own row of E (position probes), (4) row splits and repeated calls
give the same bits, (5) a padded, misaligned E, (6) G_att_edge, (7) the model against the reference model, (8) the default."""
import numpy as np
import pytest

import gat_efeat_ref as er
import gat_ref as ref
import layernorm_ref
from gat_ref import relerr
from guarded import Guarded
from test_gpu_gat import MODELS, N, TOL, _dense, _gat, _model_data, _u32, run_device
from test_gpu_gat_dropout import run_drop

pytestmark = pytest.mark.gpu

SHARED = ("out", "lse", "D", "ds_dst", "ds_src", "G_Z")          # what an efeat entry shares with its twin


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _sync_uploads():
    import torch
    torch.cuda.synchronize()


def run_efeat(ctx, indptr, indices, Z, att, K, G, E, E_T, U, drop=None, Z_dst=None, n_src=None, inject=None, split=None,
              t_split=None, E_dev=None, E_T_dev=None, chain=("scores", "forward", "backward_dst", "backward_src", "grad")):
    """scores, the three efeat entries and the column sum of P_e through the C ABI with raw pointers; returns every output.
    ``drop``: the tuple of the _drop twins; ``inject``: {name: array} replaces s_dst / s_src / lse / D / out before the
    stage that reads it; ``split`` / ``t_split``: a row at which the calls over F / over F^T are cut into two (indptr + r,
    the row operands moved by r rows, the same E pointer; under dropout dst0 / src0 move with the rows); ``E_dev`` /
    ``E_T_dev``: (pointer, lde) of the two copies where they are not packed."""
    lib, st = ctx.lib, ctx.stream(0)
    n = indptr.size - 1
    n_src = Z.shape[0] if n_src is None else n_src
    d, de = Z.shape[1], E.shape[1]
    dh = d // K
    square = Z_dst is None
    inject = inject or {}
    t_indptr, t_indices = ref.transpose_pattern(indptr, indices, n_src)
    ip, ix, tip, tix = _u32(indptr), _u32(indices), _u32(t_indptr), _u32(t_indices)
    Zs = _dense(n_src, d, host=Z)
    Zd = Zs if square else _dense(n, d, host=Z_dst)
    Gd, at, Ud = _dense(n, d, host=G), _dense(2, d, host=att), _dense(K, de, host=U)
    Ed, ETd = _dense(indices.size, de, host=E), _dense(indices.size, de, host=E_T)
    Ep, lde = E_dev if E_dev is not None else (Ed.ptr, de)
    ETp, ldet = E_T_dev if E_T_dev is not None else (ETd.ptr, de)
    out, G_Z = _dense(n, d, host=inject.get("out")), _dense(n_src, d)
    small = {k: _dense(n if k in ("s_dst", "lse", "D", "ds_dst") else n_src, K, host=inject.get(k)) for k in
             ("s_dst", "s_src", "lse", "D", "ds_dst", "ds_src")}
    P_e, G_U = _dense(n, K * de), _dense(1, K * de)
    _sync_uploads()
    dtail = lambda r0, t: () if drop is None else (drop[:4] + ((drop[4], drop[5] + r0) if t else (drop[4] + r0, drop[5])))
    sfx = "" if drop is None else "_drop"
    parts = lambda cut, rows: [(0, rows)] if cut is None else [(0, cut), (cut, rows)]
    if "scores" in chain:
        if square:
            lib.mggcn_gat_scores_f32(st, Zs.ptr, d, at.ptr, None if "s_dst" in inject else small["s_dst"].ptr,
                                     None if "s_src" in inject else small["s_src"].ptr, n_src, K, dh)
        else:
            if "s_dst" not in inject:
                lib.mggcn_gat_scores_f32(st, Zd.ptr, d, at.ptr, small["s_dst"].ptr, None, n, K, dh)
            if "s_src" not in inject:
                lib.mggcn_gat_scores_f32(st, Zs.ptr, d, at.ptr, None, small["s_src"].ptr, n_src, K, dh)
    for r0, r1 in parts(split, n):
        row = lambda M, w: M.ptr + 4 * r0 * w
        if "forward" in chain:
            getattr(lib, f"mggcn_gat_forward_efeat{sfx}_f32")(
                st, r1 - r0, n_src, ip.data_ptr() + 4 * r0, ix.data_ptr(), Zs.ptr, d, row(small["s_dst"], K), small["s_src"].ptr,
                K, dh, ref.SLOPE, row(out, d), d, row(small["lse"], K), *dtail(r0, False), Ep, lde, Ud.ptr, de)
        if "backward_dst" in chain:
            getattr(lib, f"mggcn_gat_backward_dst_efeat{sfx}_f32")(
                st, r1 - r0, n_src, ip.data_ptr() + 4 * r0, ix.data_ptr(), Zs.ptr, d, row(small["s_dst"], K), small["s_src"].ptr,
                row(small["lse"], K), row(Gd, d), d, row(out, d), d, K, dh, ref.SLOPE, row(small["D"], K),
                row(small["ds_dst"], K), *dtail(r0, False), Ep, lde, Ud.ptr, de, row(P_e, K * de), K * de)
    if "backward_src" in chain:
        for r0, r1 in parts(t_split, n_src):
            row = lambda M, w: M.ptr + 4 * r0 * w
            getattr(lib, f"mggcn_gat_backward_src_efeat{sfx}_f32")(
                st, r1 - r0, n, tip.data_ptr() + 4 * r0, tix.data_ptr(), row(Zs, d), d, small["s_dst"].ptr, row(small["s_src"], K),
                small["lse"].ptr, small["D"].ptr, Gd.ptr, d, at.ptr, row(small["ds_dst"], K) if square else None, K, dh,
                ref.SLOPE, row(small["ds_src"], K), row(G_Z, d), d, *dtail(r0, True), ETp, ldet, Ud.ptr, de)
    if "grad" in chain:
        lib.mggcn_gatv2_att_grad_f32(st, P_e.ptr, K * de, n, K * de, G_U.ptr)
    ctx.sync()
    res = {k: small[k].numpy() for k in small}
    res.update(out=out.numpy(), G_Z=G_Z.numpy(), P_e=P_e.numpy(), G_U=G_U.numpy().reshape(K, de))
    return res


def _run_case(ctx, c, K, **kw):
    kw.setdefault("U", c["U"])
    kw.setdefault("drop", c["drop"])
    return run_efeat(ctx, c["indptr"], c["indices"], c["Z"], c["att"], K, c["G"], c["E"], c["E_T"], Z_dst=c["Z_dst"],
                     n_src=c["n_src"], **kw)


# ---- (1) the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K,dh,de,p", er.efeat_cases())
def test_efeat_entry_points_against_the_restatement(ctx, name, K, dh, de, p):
    """out, lse, D, ds_dst, P_e, ds_src, G_Z and G_att_edge, each row on its own scale, at the bars of gat_efeat_ref.EFEAT_TOL:
    kernel_graph_long as F and transposed and the 200 x 320 block (dst0 = 1000, src0 = 70000 under dropout), the five head
    shapes, de = 1, 3, 8, 16, plain and at p = 0.5 and 0.9"""
    c = er.efeat_case(name, K, dh, de, p)
    got = _run_case(ctx, c, K)
    dt, dg = er.distances({k: c["twin"][k] for k in er.NAMES}, c), er.distances({k: got[k] for k in er.NAMES}, c)
    for nm in er.NAMES:
        bar = er.EFEAT_TOL[er.mode(p)][nm]
        print(f"[gat-efeat] {name} K={K} dh={dh} de={de} p={p} {nm}: row-scaled twin {dt[nm]:.3e} device {dg[nm]:.3e} (bar {bar:.1e})")
        assert dt[nm] <= bar / 8 * 1.0001, ("the input is ill-conditioned for this bar", nm, dt[nm])
    for nm in er.NAMES:
        assert dg[nm] <= er.EFEAT_TOL[er.mode(p)][nm], (nm, name, K, dh, de, p, dg[nm], "twin:", dt[nm])


@pytest.mark.parametrize("name,K,dh,de,p", [("long", 4, 32, 8, None), ("longT", 6, 7, 3, 0.5), ("longT", 1, 257, 8, 0.9)])
def test_each_entry_alone_on_injected_intermediates(ctx, name, K, dh, de, p):
    """each of the three entries called ALONE, its intermediates handed in as operands instead of taken from the stage
    before it on the device: forward on injected s_dst and s_src; backward_dst on those plus an injected lse and out (D
    must be G . out of the injected out); backward_src on injected s_dst, s_src, lse, D and ds_dst.  The injected values are
    the exact chain's, rounded to fp32; the restatement takes the same ones, so a stage's error is its own"""
    c = er.efeat_case(name, K, dh, de, p)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    inj = {k: f32(c["want"][k]) for k in ("s_dst", "s_src", "lse", "D", "ds_dst", "out")}
    args = (c["indptr"], c["indices"], c["Z"], c["att"], K, c["E"], c["U"])
    scores = dict(s_dst=inj["s_dst"], s_src=inj["s_src"])
    n, d = inj["out"].shape
    D_inj_out = (c["G"].astype(np.float64).reshape(n, K, dh) * inj["out"].astype(np.float64).reshape(n, K, dh)).sum(axis=2)
    stages = (
        (("forward",), scores, ("out", "lse"), dict(scores)),
        (("backward_dst", "grad"), dict(scores, lse=inj["lse"], out=inj["out"]), ("D", "ds_dst", "P_e", "G_U"),
         dict(scores, lse=inj["lse"], D=D_inj_out)),
        (("backward_src",), {k: inj[k] for k in ("s_dst", "s_src", "lse", "D", "ds_dst")}, ("ds_src", "G_Z"),
         dict(scores, lse=inj["lse"], D=inj["D"])),
    )
    for chain, operands, outputs, kw in stages:
        want = er.restate64(*args, G=c["G"], exact=True, scales=True, **c["kw"], **kw)
        twin = er.twin32(*args, G=c["G"], **c["kw"], **kw)
        if "G_Z" in outputs:                      # the rank-one term takes the injected ds_dst, as the entry does
            a0 = c["att"].astype(np.float64)[0].reshape(1, K, dh)
            fix = lambda r, ds: (r["G_Z"].astype(np.float64).reshape(n, K, dh)
                                 + (inj["ds_dst"].astype(np.float64) - np.asarray(ds, dtype=np.float64))[:, :, None] * a0).reshape(n, d)
            want["G_Z"], twin["G_Z"] = fix(want, want["ds_dst"]), fix(twin, twin["ds_dst"]).astype(np.float32)
        got = _run_case(ctx, c, K, chain=chain, inject=operands)
        case = dict(want=want, scale=want["scale"])
        dt, dg = er.distances({k: twin[k] for k in outputs}, case), er.distances({k: got[k] for k in outputs}, case)
        for nm in outputs:
            bar = er.EFEAT_TOL[er.mode(p)][nm]
            print(f"[gat-efeat] injected {name} K={K} dh={dh} de={de} p={p} {nm}: row-scaled twin {dt[nm]:.3e} device {dg[nm]:.3e} (bar {bar:.1e})")
            assert dt[nm] <= bar / 8 * 1.0001, ("the input is ill-conditioned for this bar", nm, dt[nm])
            assert dg[nm] <= bar, (nm, chain, dg[nm], "twin:", dt[nm])


# ---- (2) the zero vector ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,dh,de,p", [(4, 32, 8, None), (6, 7, 3, None), (4, 32, 8, 0.5), (16, 4, 8, 0.5), (1, 260, 8, None)])
def test_zero_att_edge_gives_the_plain_bits(ctx, K, dh, de, p):
    """att_edge = 0: t = +0.0 and x + 0.0 leaves lrelu and exp as they were, so every output an efeat entry shares with its
    twin has the twin's bits, the _drop forms included; P_e is whatever ds and E give and G_att_edge its column sum"""
    c = er.efeat_case("long", K, dh, de, p)
    got = _run_case(ctx, c, K, U=np.zeros_like(c["U"]))
    if p is None:
        plain = run_device(ctx, c["indptr"], c["indices"], c["Z"], c["att"], K, c["G"])
    else:
        plain = run_drop(ctx, c["indptr"], c["indices"], c["Z"], c["att"], K, c["G"], c["drop"])
    for nm in SHARED:
        np.testing.assert_array_equal(_bits(got[nm]), _bits(plain[nm]), err_msg=nm)


# ---- (3) the position probe ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ref.STRESS_KINDS)
def test_every_entry_reads_its_own_row_of_E(ctx, kind):
    """gat_ref.probe_block, every source in exactly one row: de = 1, att_edge = 1, s_dst = s_src = 0 and E[p] the crafted
    score of the entry at position p, against the plain entries with s_src[j] = the same score -- x = fmaf(E, 1, 0) = E on
    one side and 0 + s_src on the other, so the efeat entries must give the plain entries' bits across every chunk and
    prefetch boundary of rows of 64, 65, 129, 193 and 4097 entries; then the same for backward_src on the transposed block
    with the other copy of E, the score riding on s_dst on the plain side"""
    K, dh = 4, 32
    indptr, indices, n_src = ref.probe_block()
    n = indptr.size - 1
    lib, st = ctx.lib, ctx.stream(0)
    s = ref.stress_scores(kind, K)                                   # [n_src x K], the K columns equal
    E = np.ascontiguousarray(s[indices.astype(np.int64), :1])        # the score of the entry at position p
    ones = np.ones((K, 1), dtype=np.float32)
    rng = np.random.default_rng(51)
    Z, G = rng.standard_normal((n_src, K * dh), dtype=np.float32), rng.standard_normal((n, K * dh), dtype=np.float32)
    att = (0.1 * rng.standard_normal((2, K * dh))).astype(np.float32)
    zn, zs = np.zeros((n, K), dtype=np.float32), np.zeros((n_src, K), dtype=np.float32)
    # forward and backward_dst over the block as F
    ip, ix = _u32(indptr), _u32(indices)
    Zs, Gd, Ed, Ud = _dense(n_src, K * dh, host=Z), _dense(n, K * dh, host=G), _dense(indices.size, 1, host=E), _dense(K, 1, host=ones)
    sd0, ss0, ssx = _dense(n, K, host=zn), _dense(n_src, K, host=zs), _dense(n_src, K, host=s)
    o = {w: (_dense(n, K * dh), _dense(n, K), _dense(n, K), _dense(n, K), _dense(n, K * 1)) for w in ("efeat", "plain")}
    _sync_uploads()
    out, lse, D, ds, P_e = o["efeat"]
    lib.mggcn_gat_forward_efeat_f32(st, n, n_src, ip.data_ptr(), ix.data_ptr(), Zs.ptr, K * dh, sd0.ptr, ss0.ptr, K, dh, ref.SLOPE,
                                    out.ptr, K * dh, lse.ptr, Ed.ptr, 1, Ud.ptr, 1)
    lib.mggcn_gat_backward_dst_efeat_f32(st, n, n_src, ip.data_ptr(), ix.data_ptr(), Zs.ptr, K * dh, sd0.ptr, ss0.ptr, lse.ptr,
                                         Gd.ptr, K * dh, out.ptr, K * dh, K, dh, ref.SLOPE, D.ptr, ds.ptr, Ed.ptr, 1, Ud.ptr, 1,
                                         P_e.ptr, K)
    out, lse, D, ds, _ = o["plain"]
    lib.mggcn_gat_forward_f32(st, n, n_src, ip.data_ptr(), ix.data_ptr(), Zs.ptr, K * dh, sd0.ptr, ssx.ptr, K, dh, ref.SLOPE,
                              out.ptr, K * dh, lse.ptr)
    lib.mggcn_gat_backward_dst_f32(st, n, n_src, ip.data_ptr(), ix.data_ptr(), Zs.ptr, K * dh, sd0.ptr, ssx.ptr, lse.ptr, Gd.ptr,
                                   K * dh, out.ptr, K * dh, K, dh, ref.SLOPE, D.ptr, ds.ptr)
    ctx.sync()
    for nm, a, b in zip(("out", "lse", "D", "ds_dst"), o["efeat"], o["plain"]):
        np.testing.assert_array_equal(_bits(a.numpy()), _bits(b.numpy()), err_msg=f"{kind} {nm}")
    lse_host = o["plain"][1].numpy()
    assert np.isfinite(lse_host).all() and np.isfinite(o["plain"][0].numpy()).all()
    # backward_src over the block as F^T: 5 sources that list 4548 destinations, the crafted score on the destination side
    nT, nT_dst = n, n_src                                           # rows of F^T (sources), its columns (destinations)
    lseT = np.empty((nT_dst, K), dtype=np.float32)
    lseT[indices.astype(np.int64)] = np.repeat(lse_host, ref.PROBE_ROWS, axis=0)     # the row's lse, so that alpha <= 1
    DT = (0.1 * rng.standard_normal((nT_dst, K))).astype(np.float32)
    ZT, GT = rng.standard_normal((nT, K * dh), dtype=np.float32), rng.standard_normal((nT_dst, K * dh), dtype=np.float32)
    Zr, Gg, at = _dense(nT, K * dh, host=ZT), _dense(nT_dst, K * dh, host=GT), _dense(2, K * dh, host=att)
    sdx, sd00, ssT = _dense(nT_dst, K, host=s), _dense(nT_dst, K, host=zs), _dense(nT, K, host=zn)
    ls, Dd = _dense(nT_dst, K, host=lseT), _dense(nT_dst, K, host=DT)
    oT = {w: (_dense(nT, K), _dense(nT, K * dh)) for w in ("efeat", "plain")}
    _sync_uploads()
    lib.mggcn_gat_backward_src_efeat_f32(st, nT, nT_dst, ip.data_ptr(), ix.data_ptr(), Zr.ptr, K * dh, sd00.ptr, ssT.ptr, ls.ptr,
                                         Dd.ptr, Gg.ptr, K * dh, at.ptr, None, K, dh, ref.SLOPE, oT["efeat"][0].ptr,
                                         oT["efeat"][1].ptr, K * dh, Ed.ptr, 1, Ud.ptr, 1)
    lib.mggcn_gat_backward_src_f32(st, nT, nT_dst, ip.data_ptr(), ix.data_ptr(), Zr.ptr, K * dh, sdx.ptr, ssT.ptr, ls.ptr, Dd.ptr,
                                   Gg.ptr, K * dh, at.ptr, None, K, dh, ref.SLOPE, oT["plain"][0].ptr, oT["plain"][1].ptr, K * dh)
    ctx.sync()
    for nm, a, b in zip(("ds_src", "G_Z"), oT["efeat"], oT["plain"]):
        np.testing.assert_array_equal(_bits(a.numpy()), _bits(b.numpy()), err_msg=f"{kind} transposed {nm}")
    assert np.isfinite(oT["plain"][1].numpy()).all() and oT["plain"][1].numpy().any()


# ---- (4) row splits and repeated calls ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K,dh,de,p", [("long", 4, 32, 8, None), ("longT", 6, 7, 3, None), ("long", 4, 32, 16, 0.5),
                                           ("rect", 6, 7, 8, 0.9), ("longT", 1, 257, 8, None)])
def test_row_splits_and_repeated_calls_give_the_same_bits(ctx, name, K, dh, de, p):
    """the rows of F cut at row 13 and those of F^T at row 11 into two calls each (the same E pointer, indptr and the row
    operands moved, dst0 / src0 moved under dropout): every row-local output has the bits of the one call; and a second
    run of the one call gives the first run's bits in every output, G_att_edge included"""
    c = er.efeat_case(name, K, dh, de, p)
    whole, again = _run_case(ctx, c, K), _run_case(ctx, c, K)
    parts = _run_case(ctx, c, K, split=13, t_split=11)
    for nm in SHARED + ("P_e", "G_U"):
        np.testing.assert_array_equal(_bits(again[nm]), _bits(whole[nm]), err_msg=f"repeated {nm}")
        np.testing.assert_array_equal(_bits(parts[nm]), _bits(whole[nm]), err_msg=f"split {nm}")


# ---- (5) a padded, misaligned E ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,dh,de,p", [(4, 32, 8, None), (6, 7, 3, 0.5), (4, 32, 16, None)])
def test_padded_misaligned_E_gives_the_packed_bits(ctx, K, dh, de, p):
    """both copies of E at lde = de + 3 with NaN in the padding and the base one element past a 16-byte boundary (the
    element path also where de % 4 == 0): the bits of the packed call in every output, and the buffers as uploaded"""
    c = er.efeat_case("long", K, dh, de, p)
    packed = _run_case(ctx, c, K)
    gE, gT = Guarded(c["E"].shape[0], de, de + 3, 1, logical=c["E"]), Guarded(c["E"].shape[0], de, de + 3, 1, logical=c["E_T"])
    assert gE.ptr % 16 == 4
    got = _run_case(ctx, c, K, E_dev=(gE.ptr, gE.ld), E_T_dev=(gT.ptr, gT.ld))
    for nm in SHARED + ("P_e", "G_U"):
        assert np.isfinite(got[nm]).all(), nm
        np.testing.assert_array_equal(_bits(got[nm]), _bits(packed[nm]), err_msg=nm)
    gE.check_unchanged("E")
    gT.check_unchanged("E_T")


# ---- (6) G_att_edge ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K,dh,de,p", [("long", 4, 32, 8, None), ("longT", 6, 7, 16, 0.5), ("rect", 4, 32, 3, None),
                                           ("long", 16, 4, 8, None)])
def test_G_att_edge_is_the_fixed_order_column_sum(ctx, name, K, dh, de, p):
    """G_att_edge = the column sum of the device's own P_e in the order of the reduction layer, restated on the host in fp32:
    bit for bit; within its bar of the restatement; the same bits on two calls"""
    c = er.efeat_case(name, K, dh, de, p)
    a, b = _run_case(ctx, c, K), _run_case(ctx, c, K)
    np.testing.assert_array_equal(_bits(a["G_U"]), _bits(b["G_U"]))
    np.testing.assert_array_equal(_bits(a["G_U"]), _bits(er.fixed_order_colsum(a["P_e"]).reshape(K, de)))
    d = er.distances(dict(G_U=a["G_U"]), c)["G_U"]
    print(f"[gat-efeat] G_att_edge {name} K={K} dh={dh} de={de} p={p}: {d:.3e}")
    assert d <= er.EFEAT_TOL[er.mode(p)]["G_U"]


# ---- (7) the model -------------------------------------------------------------------------------------------------------------------------
DE = 3


def _edge_attr(csr, de=DE, seed=7):
    return (0.5 * np.random.default_rng(seed).standard_normal((csr[1].size, de))).astype(np.float32)


def _oracle(oracle, csr, sizes, heads, E, **kw):
    ip, ix, dv = csr
    per_layer = [heads] * (len(sizes) - 2) + [1]
    return er.oracle_gat_efeat(oracle, oracle.Csr(ip.copy(), ix.copy(), dv.copy(), N), sizes, per_layer, E, **kw)


def _owners(layer):
    """(name, device owner, parameter, gradient, m, v) of everything the layer trains, in params() order"""
    out = [("W", layer.lin, "W", "G_W", "mW", "vW"), ("b", layer.lin, "b", "G_b", "mb", "vb"),
           ("att", layer.attn, "att", "G_att", "m", "v")]
    if getattr(layer.attn, "att_edge", None) is not None:
        out.append(("att_edge", layer.attn, "att_edge", "G_att_edge", "m_edge", "v_edge"))
    if layer.res_lin is not None:
        out += [("W_r", layer.res_lin, "W", "G_W", "mW", "vW"), ("b_r", layer.res_lin, "b", "G_b", "mb", "vb")]
    if layer.gate is not None:
        out.append(("w", layer.gate, "w", "G_w", "m", "v"))
    if layer.norm is not None:
        out += [("gamma", layer.norm, "gamma", "G_gamma", "mg", "vg"), ("beta", layer.norm, "beta", "G_beta", "mb", "vb")]
    return out


def _oracle_slots(ol):
    slots = {"W": (ol.lin, "W", "G_W", "mW", "vW", "step"), "b": (ol.lin, "b", "G_b", "mb", "vb", "step"),
             "att": (ol, "att", "G_att", "m", "v", "step"), "att_edge": (ol, "att_edge", "G_att_edge", "em", "ev", "estep"),
             "w": (ol, "w", "G_w", "wm", "wv", "wstep")}
    if ol.res is not None:
        slots.update({"W_r": (ol.res, "W", "G_W", "mW", "vW", "step"), "b_r": (ol.res, "b", "G_b", "mb", "vb", "step")})
    if ol.norm is not None:
        slots.update({"gamma": (ol.norm, "gamma", "G_gamma", "mg", "vg", "step"), "beta": (ol.norm, "beta", "G_beta", "mb", "vb", "step")})
    return slots


def _sync_oracle_state(G, O):
    for layer, ol in zip(G.layers(), O.layers):
        slots = _oracle_slots(ol)
        for name, owner, p, _, m, v in _owners(layer):
            obj, op, _, om, ov, ostep = slots[name]
            setattr(obj, op, getattr(owner, p).numpy().copy())
            if getattr(owner, m) is not None:
                setattr(obj, om, getattr(owner, m).numpy().copy())
                setattr(obj, ov, getattr(owner, v).numpy().copy())
                setattr(obj, ostep, owner.step)


def _epochs(pkg, ctx, G, O, X, Y, what, epochs=3):
    """the rules of test_gpu_gat_skip._epochs over every trained tensor, att_edge included: loss at TOL, accuracy within
    3 / n, every gradient at TOL, every updated matrix parameter never more than a sign flip away and at TOL in the
    well-conditioned entries"""
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    lr = 1e-2
    for epoch in range(epochs):
        _sync_oracle_state(G, O)
        loss, acc = G.train_forward(ctx, Xd, Yd)
        G.backward(ctx)
        ctx.sync()
        grads = [{name: getattr(owner, g).numpy().copy() for name, owner, _, g, _, _ in _owners(l)} for l in G.layers()]
        G.adam_update(ctx, lr, 0.9, 0.999, 5e-4, 1e-8)
        ctx.sync()
        ol, oa = O.train_forward(X, Y)
        O.backward()
        ograds = [{name: np.array(getattr(obj, g)) for name, (obj, _, g, _, _, _) in _oracle_slots(l).items()
                   if name in grads[li]} for li, l in enumerate(O.layers)]
        O.adam_update()
        print(f"[gat-efeat] {what} epoch {epoch}: loss {loss!r} (reference {ol!r}), accuracy {acc!r} ({oa!r})")
        assert np.isfinite(ol)
        assert abs(loss - ol) <= TOL * abs(ol), (epoch, loss, ol)
        assert acc == oa or abs(acc - oa) <= 3.0 / N, (epoch, acc, oa)
        for li, (layer, olayer) in enumerate(zip(G.layers(), O.layers)):
            assert set(grads[li]) == set(ograds[li]) and "att_edge" in grads[li]
            slots = _oracle_slots(olayer)
            for name, owner, p, _, _, _ in _owners(layer):
                d = relerr(grads[li][name], ograds[li][name])
                print(f"[gat-efeat] {what} epoch {epoch} layer {li} G_{name}: {d:.3e}")
                assert d <= TOL, (what, epoch, li, name, d)
                if name in ("W", "att", "att_edge", "W_r", "w", "gamma"):
                    P, Po, g = getattr(owner, p).numpy(), getattr(slots[name][0], slots[name][1]), ograds[li][name]
                    assert np.abs(P - Po).max() <= 2.05 * lr, (epoch, li, name)          # never more than a sign flip
                    solid = np.abs(g) > 1e-2 * np.abs(g).max()                          # well-conditioned entries
                    assert np.abs(P - Po)[solid].max() <= TOL * np.abs(Po).max(), (epoch, li, name)


MODEL_CASES = [({}, {}), ({}, dict(dropout=0.5, attn_dropout=0.3)), (dict(skip="gate", norm="layer"), {})]


@pytest.mark.parametrize("options,drop", MODEL_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_epochs_match_the_reference(pkg, oracle, ctx, options, drop):
    """three full epochs (forward, loss, backward, Adam) of gat(edge_attr=E) against the reference model on identical
    inputs: plain, with both dropouts, and with skip="gate", norm="layer" """
    sizes, heads = MODELS[1]
    csr, X, Y = _model_data(pkg, sizes)
    E = _edge_attr(csr)
    G = _gat(pkg, csr, sizes, heads, edge_attr=E, **options, **drop)
    assert G.edge_dim == DE and G.E_A.shape() == G.E_F.shape() == (csr[1].size, DE)
    okw = {}
    if drop:
        G.set_dropout(drop["dropout"], seed=0xC0FFEE123, epoch=4, attn=drop["attn_dropout"])
        okw = dict(p=drop["dropout"], attn_p=drop["attn_dropout"], seed=0xC0FFEE123, epoch=4)
    O = _oracle(oracle, csr, sizes, heads, E, **options, **okw)
    for layer, ol in zip(G.layers(), O.layers):                     # same seed-99 init, bit for bit
        slots = _oracle_slots(ol)
        for name, owner, p, _, _, _ in _owners(layer):
            np.testing.assert_array_equal(getattr(owner, p).numpy(), getattr(slots[name][0], slots[name][1]), err_msg=name)
        assert layer.attn.att_edge.shape() == (layer.attn.heads, DE)
    for li, (layer, ol) in enumerate(zip(G.layers(), O.layers)):
        if layer.norm is not None:
            gamma, beta = layernorm_ref.params(layer.norm.gamma.m(), 5 + li)
            layer.norm.init(gamma, beta)
            ol.norm.gamma, ol.norm.beta = gamma.copy(), beta.copy()
    _epochs(pkg, ctx, G, O, X, Y, f"{options} {drop}")
    if drop:
        assert G.dropout_epoch == 7


def _state_bits(G):
    out = []
    for l in G.layers():
        for _, owner, p, g, m, v in _owners(l):
            out += [getattr(owner, a).numpy().view(np.uint32).copy() for a in (p, g, m, v)]
    return out


def _run_epochs(pkg, ctx, fused, step, epochs=3, **kw):
    sizes, heads = MODELS[0]
    csr, X, Y = _model_data(pkg, sizes)
    G = _gat(pkg, csr, sizes, heads, fused=fused, edge_attr=_edge_attr(csr), **kw)
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    res = []
    for _ in range(epochs):
        if step:
            res.append(G.train_step(ctx, Xd, Yd, 1e-2, 0.9, 0.999, 5e-4, 1e-8))
        else:
            res.append(G.train_forward(ctx, Xd, Yd))
            G.backward(ctx)
            G.adam_update(ctx, 1e-2, 0.9, 0.999, 5e-4, 1e-8)
            ctx.sync()
    return res, _state_bits(G), G


def test_fused_and_per_tensor_adam_give_the_same_bits(pkg, ctx):
    """fused=True against fused=False, and train_step against the three calls: the same losses and the same bits in every
    parameter, gradient and Adam moment, att_edge's included, after three epochs with both dropouts"""
    kw = dict(dropout=0.3, attn_dropout=0.2)
    base = _run_epochs(pkg, ctx, False, False, **kw)
    assert len(base[1]) == 4 * 3 * 4                                  # three layers of W, b, att, att_edge: 4 arrays each
    for fused, step in ((True, False), (True, True)):
        res, bits, _ = _run_epochs(pkg, ctx, fused, step, **kw)
        assert res == base[0], (fused, step)
        for a, b in zip(bits, base[1]):
            np.testing.assert_array_equal(a, b)
    assert base[0][-1][0] < base[0][0][0], base[0]                  # and it trains
    assert all(np.any(l.attn.att_edge.numpy() != 0) and np.any(l.attn.G_att_edge.numpy() != 0) for l in base[2].layers())


def test_set_dropout_replays_a_forward(pkg, ctx):
    """set_dropout(..., epoch=e) replays training forward e bit for bit, edge term and attention mask included"""
    sizes, heads = MODELS[0]
    csr, X, Y = _model_data(pkg, sizes)
    G = _gat(pkg, csr, sizes, heads, edge_attr=_edge_attr(csr), dropout=0.4, attn_dropout=0.3)
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    G.set_dropout(0.4, seed=77, epoch=5, attn=0.3)
    first = G.train_forward(ctx, Xd, Yd)
    ctx.sync()
    out1 = [l.out.numpy().view(np.uint32).copy() for l in G.layers()]
    other = G.train_forward(ctx, Xd, Yd)                             # epoch 6: another mask
    ctx.sync()
    assert other != first
    G.set_dropout(0.4, seed=77, epoch=5, attn=0.3)
    assert G.train_forward(ctx, Xd, Yd) == first
    ctx.sync()
    for a, l in zip(out1, G.layers()):
        np.testing.assert_array_equal(a, l.out.numpy().view(np.uint32))


def test_selector_restores_att_edge_and_the_refusals_fire(pkg, ctx, tmp_path):
    """model_selector.restore brings back the best epoch's parameters, att_edge among them, bit for bit; save, load, save_best,
    attention_weights and gat_layer.alpha raise ValueError naming edge_attr on the live model and create no file; evaluate
    and predict run"""
    sizes, heads = MODELS[0]
    csr, X, Y = _model_data(pkg, sizes)
    S = np.random.default_rng(4).choice(3, size=N).astype(np.int32)
    G = _gat(pkg, csr, sizes, heads, edge_attr=_edge_attr(csr))
    G.set_splits(S)
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    sel = pkg.model_selector(G, split="val", metric="loss")
    names = [name for name, _ in sel._params()]
    assert names[:4] == ["W0", "b0", "att0", "att_edge0"] and "att_edge2" in names
    snaps = []
    for _ in range(4):
        snaps.append({name: t.numpy().view(np.uint32).copy() for name, t in sel._params()})
        sel.step(ctx, Xd, Yd, 0.3 if len(snaps) > 2 else 1e-2, 0.9, 0.999, 5e-4, 1e-8)
    assert sel.best_epoch is not None
    assert np.any(snaps[-1]["att_edge0"] != snaps[0]["att_edge0"])
    sel.restore(ctx)
    for name, t in sel._params():
        np.testing.assert_array_equal(t.numpy().view(np.uint32), snaps[sel.best_epoch][name], err_msg=name)
    path = str(tmp_path / "model.ckpt")
    for call in (lambda: G.save(ctx, path), lambda: G.load(ctx, path), lambda: sel.save_best(ctx, path),
                 lambda: G.attention_weights(ctx, Xd), lambda: G.layers()[0].alpha(ctx)):
        with pytest.raises(ValueError, match="edge_attr"):
            call()
    assert not list(tmp_path.iterdir())
    res = G.evaluate(ctx, Xd, Yd)
    pred = G.predict(ctx, Xd)
    assert 0.0 <= res["all"] <= 1.0 and pred.shape == (N, 1)
    assert abs(res["all"] - float((pred == Y).mean())) <= 1e-6       # evaluate and predict run the same plain forward


# ---- (8) the default -----------------------------------------------------------------------------------------------------------------------
def test_default_is_what_it_was(pkg):
    """edge_attr=None spelled out: the timers, the parameters and the bits of a model built without the argument after three
    epochs; and the model with edge features registers the plain model's timers plus the column sum of P_e alone"""
    sizes, heads = MODELS[0]
    csr, X, Y = _model_data(pkg, sizes)
    runs = []
    for kw in ({}, dict(edge_attr=None, edge_weights=None), dict(edge_attr=_edge_attr(csr))):
        c = pkg.context(0)
        G = _gat(pkg, csr, sizes, heads, **kw)
        Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
        res = [G.train_step(c, Xd, Yd, 1e-2, 0.9, 0.999, 5e-4, 1e-8) for _ in range(3)]
        bits = [t.numpy().view(np.uint32).copy() for l in G.layers() for t in (l.W(), l.b(), l.att(), l.GW(), l.Gb(), l.Gatt())]
        runs.append((res, bits, sorted(c.timers), [type(l.attn).__name__ for l in G.layers()], G.edge_dim))
    (r0, b0, t0, a0, d0), (r1, b1, t1, a1, d1), (_, _, t2, a2, d2) = runs
    assert r0 == r1 and t0 == t1 and a0 == a1 == ["attention"] * 3 and d0 == d1 == 0
    for a, b in zip(b0, b1):
        np.testing.assert_array_equal(a, b)
    assert not any("edge" in t for t in t0)
    assert a2 == ["attention_efeat"] * 3 and d2 == DE
    assert sorted(set(t2) - set(t0)) == [f"{i}_1_gat-edge-grad" for i in range(3)] and set(t0) <= set(t2)
