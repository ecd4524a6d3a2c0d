"""The GATv2 kernels (include/mggcn.h: mggcn_gatv2_*) and gat(variant="v2") on the device, against the fp64 restatement and
the reference model of gatv2_ref.py.  Kernel level: the row-scaled measure of gat_ref.rowdist at the bars gatv2_ref.BAR, fixed
on the CPU (test_gatv2_cpu.py); model level: the rules and bars of test_gpu_gat.py's model tests.  Everything that is claimed
bitwise is compared as bits."""
import numpy as np
import pytest

import bce_ref
import gat_ref as ref
import gatv2_ref as v2
from gat_ref import relerr, rowerr
from test_gpu_gat import COLSUM_BLOCKS, N, TOL, _assert_grads, _dense, _grads, _model_data, _state_bits, _sync_oracle_state, _u32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class _half:
    """one half of a [rows x 2 d] device buffer, with the interface of test_gpu_gat._dense"""

    def __init__(self, whole, d, half):
        self.whole, self.d, self.ld, self.ptr, self.half = whole, d, whole.ld, whole.ptr + 4 * d * half, half

    def numpy(self):
        return self.whole.numpy()[:, self.half * self.d:(self.half + 1) * self.d].copy()


OPERANDS = ("Zs", "Zd", "G", "att", "out", "G_Zd", "P", "G_Zs")


def run_device(ctx, c, K, halves=False, off=None, pad=0, slope=ref.SLOPE, rows=None, t_rows=None, into=None):
    """the four entry points once, through the C ABI with raw pointers: forward, backward_dst, att_grad, backward_src;
    returns the outputs of gatv2_ref.NAMES as numpy arrays (``into``: and the operands, to be passed again).
    ``halves``: Zs | Zd and G_Zs | G_Zd as the halves of one [n x 2 d] buffer each (square cases); ``off``: {operand: floats}
    moves the base of that operand alone off its 16-byte alignment; ``pad``: every leading dimension is d + pad;
    ``rows`` / ``t_rows`` = (r0, r1): the calls over F's rows / over F^T's rows take that row range only, as a call of its own
    on the operands of ``into`` (a previous whole call: the range reads its lse, D and out, and overwrites nothing else)"""
    import torch
    lib, st = ctx.lib, ctx.stream(0)
    indptr, indices, n, n_src = c["indptr"], c["indices"], c["n"], c["n_src"]
    d = K * (c["Zs"].shape[1] // K)
    dh = d // K
    o = dict(dict.fromkeys(OPERANDS, 0), **(off or {}))
    if into is not None and "ops" in into:
        m = into["ops"]
    else:
        t_indptr, t_indices = ref.transpose_pattern(indptr, indices, n_src)
        m = dict(ip=_u32(indptr), ix=_u32(indices), tip=_u32(t_indptr), tix=_u32(t_indices))
        if halves:
            assert n == n_src
            Z2 = _dense(n, 2 * d, 0, 0, np.concatenate([c["Zs"], c["Zd"]], axis=1))
            G_Z2 = _dense(n, 2 * d)
            m.update(Zs=_half(Z2, d, 0), Zd=_half(Z2, d, 1), G_Zs=_half(G_Z2, d, 0), G_Zd=_half(G_Z2, d, 1))
        else:
            m.update(Zs=_dense(n_src, d, o["Zs"], pad, c["Zs"]), Zd=_dense(n, d, o["Zd"], pad, c["Zd"]),
                     G_Zs=_dense(n_src, d, o["G_Zs"], pad), G_Zd=_dense(n, d, o["G_Zd"], pad))
        m.update(G=_dense(n, d, o["G"], pad, c["G"]), att=_dense(1, d, o["att"], 0, c["att"]), out=_dense(n, d, o["out"], pad),
                 P=_dense(n, d, o["P"], pad), lse=_dense(n, K), D=_dense(n, K), G_att=_dense(1, d))
        if into is not None:
            into["ops"] = m
    torch.cuda.synchronize()                        # the operands are filled on torch's stream, the library runs on the context's
    r0, r1 = rows if rows is not None else (0, n)
    t0, t1 = t_rows if t_rows is not None else (0, n_src)

    def at(x, r):                                   # the address of row r
        return x.ptr + 4 * r * x.ld
    Zs, Zd, G, out, lse, D, P, G_Zd, G_Zs = (m[k] for k in ("Zs", "Zd", "G", "out", "lse", "D", "P", "G_Zd", "G_Zs"))
    lib.mggcn_gatv2_forward_f32(st, r1 - r0, n_src, m["ip"].data_ptr() + 4 * r0, m["ix"].data_ptr(), Zs.ptr, Zs.ld, at(Zd, r0),
                                Zd.ld, m["att"].ptr, K, dh, slope, at(out, r0), out.ld, at(lse, r0))
    lib.mggcn_gatv2_backward_dst_f32(st, r1 - r0, n_src, m["ip"].data_ptr() + 4 * r0, m["ix"].data_ptr(), Zs.ptr, Zs.ld,
                                     at(Zd, r0), Zd.ld, m["att"].ptr, at(lse, r0), at(G, r0), G.ld, at(out, r0), out.ld, K, dh,
                                     slope, at(D, r0), at(G_Zd, r0), G_Zd.ld, at(P, r0), P.ld)
    lib.mggcn_gatv2_att_grad_f32(st, P.ptr, P.ld, n, d, m["G_att"].ptr)
    lib.mggcn_gatv2_backward_src_f32(st, t1 - t0, n, m["tip"].data_ptr() + 4 * t0, m["tix"].data_ptr(), at(Zs, t0), Zs.ld,
                                     Zd.ptr, Zd.ld, m["att"].ptr, lse.ptr, D.ptr, G.ptr, G.ld, K, dh, slope, at(G_Zs, t0),
                                     G_Zs.ld)
    ctx.sync()
    return {k: m[k].numpy() for k in v2.NAMES}


def _assert_case(what, c, got, names=v2.NAMES):
    for name in names:
        rt, dt = rowerr(c["twin"][name], c["want"][name], c["scale"][name]) if "twin" in c else (-1, 0.0)
        rg, dg = rowerr(got[name], c["want"][name], c["scale"][name])
        print(f"[gatv2] {what} {name}: twin {dt:.3e} (row {rt}) device {dg:.3e} (row {rg}) (bar {v2.BAR[name]:.0e})")
        assert dg <= v2.BAR[name], (what, name, rg, dg, "twin:", dt)


# ---- (1) every entry point against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K,dh", v2.cases())
def test_every_entry_point_against_the_restatement(ctx, name, K, dh):
    """out, lse, D, G_Zd, P, G_att and G_Zs within the bar on kernel_graph_long() as F and transposed (so each kernel walks the
    long rows) at one (K, dh) per compiled variant plus the masked-tile cases, and on the 200 x 320 block"""
    c = v2.case(name, K, dh)
    _assert_case(f"{name} K={K} dh={dh}", c, run_device(ctx, c, K))


# ---- (2) the model's layout -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,dh", [(4, 32), (3, 7)])
def test_halves_of_one_buffer_give_the_bits_of_separate_buffers(ctx, K, dh):
    """Zs | Zd as the halves of one [n x 2 out] buffer with ld = 2 out, and G_Zs | G_Zd as halves of one buffer"""
    c = v2.case("long", K, dh)
    a, b = run_device(ctx, c, K), run_device(ctx, c, K, halves=True)
    for name in v2.NAMES:
        np.testing.assert_array_equal(_bits(a[name]), _bits(b[name]), err_msg=name)
    _assert_case(f"halves K={K} dh={dh}", c, b)


# ---- (3) misalignment ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", OPERANDS + ("ld",))
def test_misaligned_operands_take_the_element_path(ctx, which):
    """(4, 32) with one operand alone one float off 16-byte alignment, or every leading dimension d + 3: every kernel that
    touches it leaves the float4 path, stays within the bar of the restatement and within 1e-4 of the aligned run"""
    c = v2.case("long", 4, 32)
    aligned = run_device(ctx, c, 4)
    got = run_device(ctx, c, 4, pad=3) if which == "ld" else run_device(ctx, c, 4, off={which: 1})
    _assert_case(f"misaligned {which}", c, got)
    for name in v2.NAMES:                            # two reduction orders of the same numbers
        assert relerr(got[name], aligned[name]) <= 1e-4, name


# ---- (4) empty and one-entry rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,dh", [(4, 32), (3, 7)])
def test_empty_rows_one_entry_rows_and_unreferenced_sources(ctx, K, dh):
    """rows without entries write lse = 0, out = +0.0, G_Zd = 0 and P = 0 over the 123.0 the buffers held; the one-entry
    row's out is its source's row bit for bit; an unreferenced source gets G_Zs = 0"""
    c = v2.case("long", K, dh)
    indptr, indices = c["indptr"], c["indices"]
    got = run_device(ctx, c, K)
    for r in (0, 319):
        assert indptr[r] == indptr[r + 1]
        np.testing.assert_array_equal(_bits(got["out"][r]), np.zeros(K * dh, dtype=np.uint32))
        np.testing.assert_array_equal(_bits(got["lse"][r]), np.zeros(K, dtype=np.uint32))
        np.testing.assert_array_equal(got["G_Zd"][r], np.zeros(K * dh, dtype=np.float32))
        np.testing.assert_array_equal(got["P"][r], np.zeros(K * dh, dtype=np.float32))
    assert indptr[2] - indptr[1] == 1
    np.testing.assert_array_equal(_bits(got["out"][1]), _bits(c["Zs"][indices[indptr[1]]]))
    np.testing.assert_array_equal(got["G_Zs"][ref.UNREFERENCED], np.zeros(K * dh, dtype=np.float32))


# ---- (5) crafted probes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,dh", [(4, 32), (3, 7)])
def test_the_source_that_wins_by_40_at_every_chunk_edge(ctx, K, dh):
    """gatv2_ref.forward_probe_case: the source at position 0, 63, 64, 127, 128, L - 2 or L - 1 of each row scores 40, every
    other 0, all exactly.  out[row] is that source's row to the last bit wherever the exact restatement rounds to it, and
    within the bar everywhere; lse is 40 to the last bit"""
    for t in range(ref.PROBE_SLOTS):
        c = v2.forward_probe_case(t, K, dh)
        got = run_device(ctx, dict(c, G=np.zeros((c["n"], K * dh), dtype=np.float32)), K)
        hot = c["Zs"][c["hot"]]
        exact = c["want"]["out"].astype(np.float32) == hot
        assert exact.mean() >= 0.99
        np.testing.assert_array_equal(_bits(got["out"])[exact], _bits(hot)[exact], err_msg=f"slot {t} positions {c['pos']}")
        np.testing.assert_array_equal(got["lse"], np.full((c["n"], K), 40.0, dtype=np.float32))
        assert rowerr(got["out"], c["want"]["out"], c["want"]["scale"]["out"])[1] <= v2.BAR["out"]


@pytest.mark.parametrize("K,dh", [(4, 32), (3, 7)])
def test_scores_in_the_hundreds_stay_finite_and_convex(ctx, K, dh):
    """gatv2_ref.stress_case: scores that reach the hundreds (exact in fp32).  Every output is finite, every out[i, c] lies
    between the smallest and the largest gathered Zs[j, c] widened by 1e-5 max|Zs|, and the weights add up to one:
    |sum_j exp(e_ijk - lse[i, k]) - 1| <= 1e-5 with the exact scores and the DEVICE's lse"""
    c = v2.stress_case(K, dh)
    indptr, indices = c["indptr"], c["indices"]
    e = c["want"]["e"]
    tops = [e[int(indptr[r]):int(indptr[r + 1])].max() for r in range(c["n"])]
    assert 100 < min(tops) and max(tops) < 256, tops
    got = run_device(ctx, c, K, slope=v2.STRESS_SLOPE)
    for name in v2.NAMES:
        assert np.isfinite(got[name]).all(), name
    slack = 1e-5 * np.abs(c["Zs"]).max()
    for r in range(c["n"]):
        rows = c["Zs"][indices[int(indptr[r]):int(indptr[r + 1])]]
        assert (got["out"][r] >= rows.min(axis=0) - slack).all() and (got["out"][r] <= rows.max(axis=0) + slack).all(), r
    sums = v2.alpha_row_sums(indptr, e, got["lse"])
    print(f"[gatv2] stress K={K} dh={dh}: top scores {np.round(tops, 1).tolist()}, |sum alpha - 1| <= {np.abs(sums - 1).max():.2e}")
    assert np.abs(sums - 1).max() <= 1e-5
    for name in ("out", "lse", "D"):
        assert rowerr(got[name], c["want"][name], c["want"]["scale"][name])[1] <= v2.BAR[name], name


# ---- (6) dynamic attention ------------------------------------------------------------------------------------------------------------------
def test_two_destinations_prefer_different_sources(ctx):
    """gatv2_ref.dynamic_probe() on the device: out[i] = alpha_i0 (2, 2), so alpha_i0 = out[i, 0] / 2"""
    indptr, indices, Zs, Zd, att = v2.dynamic_probe()
    c = dict(indptr=indptr, indices=indices, n=2, n_src=2, Zs=Zs, Zd=Zd, att=att, G=np.ones((2, 2), dtype=np.float32))
    got = run_device(ctx, c, 1)
    want = v2.restate64(indptr, indices, Zs, Zd, att, 1, exact=True, scales=True)
    assert rowerr(got["out"], want["out"], want["scale"]["out"])[1] <= v2.BAR["out"]
    assert rowerr(got["lse"], want["lse"], want["scale"]["lse"])[1] <= v2.BAR["lse"]
    a0 = got["out"][:, 0] / 2
    assert a0[0] > 0.5 > a0[1], a0                   # destination 0 prefers source 0, destination 1 source 1


# ---- (7) reproducibility and row slices ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K,dh,off", [("long", 4, 32, 0), ("longT", 4, 32, 0), ("long", 3, 7, 0), ("longT", 1, 260, 0),
                                           ("long", 1, 257, 0), ("long", 4, 32, 1)])
def test_two_calls_give_the_same_bits(ctx, name, K, dh, off):
    c = v2.case(name, K, dh)
    kw = dict(off=dict.fromkeys(OPERANDS, off))
    a, b = run_device(ctx, c, K, **kw), run_device(ctx, c, K, **kw)
    for nm in v2.NAMES:
        np.testing.assert_array_equal(_bits(a[nm]), _bits(b[nm]), err_msg=nm)


@pytest.mark.parametrize("name,K,dh", [("long", 4, 32), ("longT", 4, 32), ("long", 3, 7), ("longT", 2, 65)])
def test_a_row_range_gives_the_whole_calls_rows(ctx, name, K, dh):
    """rows [5, 13) of F, and rows [5, 13) of F^T, passed as calls of their own on buffers pre-filled with 123.0: the rows of
    the range carry the whole call's bits and every other row keeps its 123.0"""
    c = v2.case(name, K, dh)
    whole = run_device(ctx, c, K)
    keep = {}
    run_device(ctx, c, K, into=keep)                                   # lse, D and out of the whole call, for backward_src
    m = keep["ops"]
    import torch
    for k in ("out", "G_Zd", "P", "G_Zs"):
        m[k].flat.fill_(123.0)
    saved = {k: m[k].numpy() for k in ("lse", "D")}
    part = run_device(ctx, c, K, rows=(5, 13), t_rows=(5, 13), into=keep)
    torch.cuda.synchronize()
    for nm, r0, r1 in (("out", 5, 13), ("G_Zd", 5, 13), ("P", 5, 13), ("G_Zs", 5, 13)):
        np.testing.assert_array_equal(_bits(part[nm][r0:r1]), _bits(whole[nm][r0:r1]), err_msg=nm)
        rest = np.delete(part[nm], np.arange(r0, r1), axis=0)
        assert (rest == 123.0).all(), nm
    for nm in ("lse", "D"):                                            # rewritten in place with the same bits
        np.testing.assert_array_equal(_bits(part[nm]), _bits(saved[nm]), err_msg=nm)
        np.testing.assert_array_equal(_bits(part[nm]), _bits(whole[nm]), err_msg=nm)


def test_no_rows_launches_nothing_and_writes_nothing(ctx):
    c = v2.case("long", 4, 32)
    got = run_device(ctx, c, 4, rows=(0, 0), t_rows=(0, 0))
    for nm in ("out", "lse", "D", "G_Zd", "P", "G_Zs"):
        assert (got[nm] == 123.0).all(), nm
    # att_grad of no rows writes zeros
    G_att = _dense(1, 12)
    import torch
    torch.cuda.synchronize()
    ctx.lib.mggcn_gatv2_att_grad_f32(ctx.stream(0), None, 12, 0, 12, G_att.ptr)
    ctx.sync()
    np.testing.assert_array_equal(_bits(G_att.numpy()), np.zeros((1, 12), dtype=np.uint32))


# ---- (8) att_grad ------------------------------------------------------------------------------------------------------------------------------
# (width, rows, pad): rows that are no multiple of the rows a workgroup takes at a time (256 / the power of two covering the
# width); at width 1 a workgroup takes 256 rows and the grid is capped at COLSUM_BLOCKS, so one pass covers 131072 rows
ATT_GRAD = [(1, 2 * 256 * COLSUM_BLOCKS + 77, 0), (1, 1003, 2), (12, 1003, 0), (255, 1003, 1), (256, 1003, 0), (257, 1003, 3),
            (1024, 1003, 0), (1024, 3, 0)]


@pytest.mark.parametrize("width,n,pad", ATT_GRAD)
def test_att_grad_column_sums(ctx, width, n, pad):
    """G_att[c] = sum_i P[i, c] per column against sum_i |P[i, c]| at the bar, the same bits on a second call, and -- where
    the rows exceed one pass of the capped grid -- from the rows beyond the first pass alone"""
    import torch
    rng = np.random.default_rng(width + n)
    P = rng.standard_normal((n, width), dtype=np.float32)
    beyond = n > 256 * COLSUM_BLOCKS
    if beyond:
        P[:256 * COLSUM_BLOCKS] = 0
    Pd, G_att, again = _dense(n, width, 0, pad, P), _dense(1, width), _dense(1, width)
    torch.cuda.synchronize()
    for g in (G_att, again):
        ctx.lib.mggcn_gatv2_att_grad_f32(ctx.stream(0), Pd.ptr, Pd.ld, n, width, g.ptr)
    ctx.sync()
    P64 = P.astype(np.float64)
    d = rowerr(G_att.numpy().T, P64.sum(axis=0)[:, None], np.abs(P64).sum(axis=0)[:, None])
    print(f"[gatv2] att_grad width={width} rows={n} ld={width + pad}: worst column {d[0]} at {d[1]:.3e}")
    assert d[1] <= v2.BAR["G_att"]
    assert not beyond or np.abs(G_att.numpy()).min() > 0
    np.testing.assert_array_equal(_bits(G_att.numpy()), _bits(again.numpy()))


# ---- (9) the model -----------------------------------------------------------------------------------------------------------------------------
MODELS = [([20, 16, 12, 5], 4), ([48, 32, 32, 7], 4)]


def _gat(pkg, csr, sizes, heads, **kw):
    ip, ix, dv = csr
    return pkg.gat(pkg.csr_matrix(ip.copy(), ix.copy(), dv.copy(), N), sizes, heads=heads, **kw)


def _oracle(oracle, csr, sizes, heads, **kw):
    ip, ix, dv = csr
    per_layer = [heads] * (len(sizes) - 2) + [1]
    return v2.oracle_gatv2(oracle, oracle.Csr(ip.copy(), ix.copy(), dv.copy(), N), sizes, per_layer, **kw)


def _epochs_against_the_reference(pkg, oracle, ctx, G, O, sizes, X, Y, what):
    for layer, ol in zip(G.layers(), O.layers):                     # same seed-99 init, bit for bit
        np.testing.assert_array_equal(layer.W().numpy(), ol.lin.W)
        np.testing.assert_array_equal(layer.b().numpy(), ol.lin.b)
        np.testing.assert_array_equal(layer.att().numpy(), ol.att)
        assert layer.W().shape() == (ol.lin.W.shape[0], 2 * ol.out_width) and layer.att().shape() == (1, ol.out_width)
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    lr = 1e-2
    for epoch in range(3):
        _sync_oracle_state(G, O)
        loss, acc = G.train_forward(ctx, Xd, Yd)
        G.backward(ctx)
        ctx.sync()
        grads = _grads(G)
        G.adam_update(ctx, lr, 0.9, 0.999, 5e-4, 1e-8)
        ctx.sync()
        ol, oa = O.train_forward(X, Y)
        O.backward()
        ograds = [(l.lin.G_W.copy(), l.lin.G_b.copy(), l.G_att.copy()) for l in O.layers]
        O.adam_update()
        print(f"[gatv2] {what} epoch {epoch}: loss {loss!r} (reference {ol!r}), acc {acc!r} ({oa!r})")
        assert np.isfinite(ol), "the reference overflowed: the input is outside its range"
        assert abs(loss - ol) <= TOL * abs(ol), (epoch, loss, ol)
        assert abs(acc - oa) <= 3.0 / N, (epoch, acc, oa)
        _assert_grads(f"{what} epoch {epoch}", grads, ograds)
        for li, (layer, olayer) in enumerate(zip(G.layers(), O.layers)):
            for name, P, Po, g in (("W", layer.W().numpy(), olayer.lin.W, ograds[li][0]),
                                   ("att", layer.att().numpy(), olayer.att, ograds[li][2])):
                assert np.abs(P - Po).max() <= 2.05 * lr, (epoch, li, name)          # never more than a sign flip
                solid = np.abs(g) > 1e-2 * np.abs(g).max()                          # well-conditioned entries
                assert np.abs(P - Po)[solid].max() <= TOL * np.abs(Po).max(), (epoch, li, name)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("sizes,heads", MODELS)
def test_gatv2_epochs_match_the_reference(pkg, oracle, ctx, fused, sizes, heads):
    """three full epochs (forward, loss, backward, Adam) against the reference model on identical inputs, by the rules of
    test_gpu_gat.test_gat_epochs_match_the_reference"""
    csr, X, Y = _model_data(pkg, sizes)
    G = _gat(pkg, csr, sizes, heads, fused=fused, variant="v2")
    O = _oracle(oracle, csr, sizes, heads)
    _epochs_against_the_reference(pkg, oracle, ctx, G, O, sizes, X, Y, f"sizes={sizes} fused={fused}")


def test_gatv2_dropout_epochs_match_the_reference(pkg, oracle, ctx):
    """dropout=0.5 against the reference model with the numpy mask, from epoch 4 of seed 0xC0FFEE123"""
    sizes, heads = MODELS[0]
    csr, X, Y = _model_data(pkg, sizes)
    G = _gat(pkg, csr, sizes, heads, dropout=0.5, variant="v2")
    G.set_dropout(0.5, seed=0xC0FFEE123, epoch=4)
    O = _oracle(oracle, csr, sizes, heads, p=0.5, seed=0xC0FFEE123, epoch=4)
    _epochs_against_the_reference(pkg, oracle, ctx, G, O, sizes, X, Y, f"sizes={sizes} dropout=0.5")
    assert G.dropout_epoch == 7 and G.attn_dropout_p == 0.0


def _run_epochs(pkg, ctx, sizes, heads, fused, step, epochs=3, **kw):
    csr, X, Y = _model_data(pkg, sizes)
    G = _gat(pkg, csr, sizes, heads, fused=fused, **kw)
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
    return res, _state_bits(G)


@pytest.mark.parametrize("sizes,heads", MODELS)
def test_fused_adam_per_tensor_adam_and_train_step_give_the_same_bits(pkg, ctx, sizes, heads):
    base = _run_epochs(pkg, ctx, sizes, heads, fused=False, step=False, variant="v2")
    for fused, step in ((True, False), (True, True), (False, True)):
        res, bits = _run_epochs(pkg, ctx, sizes, heads, fused=fused, step=step, variant="v2")
        assert res == base[0], (fused, step)
        for a, b in zip(bits, base[1]):
            np.testing.assert_array_equal(a, b)
    assert base[0][-1][0] < base[0][0][0], base[0]                 # and it trains


def test_bce_with_splits_matches_the_reference(pkg, oracle, ctx):
    """loss="bce" with set_splits: one epoch against the reference model with the fp32 restatement of the multi-label loss
    over the training rows"""
    sizes, heads = MODELS[1]
    csr, X, _ = _model_data(pkg, sizes)
    T = (np.random.default_rng(3).random((N, sizes[-1])) < 0.2).astype(np.int32)
    S = np.random.default_rng(4).choice(4, size=N, p=(0.5, 0.2, 0.25, 0.05)).astype(np.int32)
    train = S == 0
    n_train = int(train.sum())
    G = _gat(pkg, csr, sizes, heads, loss="bce", variant="v2")
    G.set_splits(S)

    def loss(H):
        Gr = np.ascontiguousarray(bce_ref.grad32(H, T, 1.0 / (float(n_train) * H.shape[1])))
        Gr[~train] = 0
        return Gr, (float(bce_ref.loss32(H, T).astype(np.float64)[train].sum() / (n_train * H.shape[1])),
                    bce_ref.micro_f1(*bce_ref.counts(H[train], T[train])[0]))
    O = _oracle(oracle, csr, sizes, heads, loss=loss)
    got = G.train_forward(ctx, pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(T))
    assert got == G.split_metrics()["train"] and G.split_metrics()["counts"]["train"] == n_train
    G.backward(ctx)
    ctx.sync()
    want = O.train_forward(X, None)
    O.backward()
    print(f"[gatv2] bce with splits: (loss, micro-F1) {got!r} (reference {want!r})")
    assert abs(got[0] - want[0]) <= TOL * abs(want[0])
    assert got[1] == want[1] or abs(got[1] - want[1]) <= 3.0 / n_train
    _assert_grads("bce with splits", _grads(G), [(l.lin.G_W, l.lin.G_b, l.G_att) for l in O.layers])


def test_evaluate_agrees_with_a_plain_forward(pkg, ctx):
    sizes, heads = MODELS[1]
    csr, X, Y = _model_data(pkg, sizes)
    S = np.random.default_rng(4).choice(3, size=N).astype(np.int32)
    G = _gat(pkg, csr, sizes, heads, variant="v2", dropout=0.5)
    Xd, Yd, Sd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y), pkg.dn_matrix.from_numpy(S.reshape(-1, 1))
    res = G.evaluate(ctx, Xd, Yd, Sd)
    out = G(ctx, Xd)
    ctx.sync()
    hit = out.numpy().argmax(axis=1) == Y.reshape(-1)
    assert res["all"] == float(hit.mean()) and G.dropout_epoch == 0       # neither drops
    for k, name in enumerate(("train", "val", "test")):
        assert res[name] == float(hit[S == k].mean())


def test_set_dropout_replays_an_epoch(pkg, ctx):
    sizes, heads = MODELS[0]
    csr, X, Y = _model_data(pkg, sizes)
    G = _gat(pkg, csr, sizes, heads, dropout=0.5, variant="v2")
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)

    def epoch():
        res = G.train_forward(ctx, Xd, Yd)
        G.backward(ctx)
        ctx.sync()
        return res, [_bits(t) for g in _grads(G) for t in g]
    G.set_dropout(0.5, seed=11, epoch=2)
    first = epoch()
    assert G.dropout_epoch == 3
    second = epoch()
    assert second[0] != first[0] and any((a != b).any() for a, b in zip(first[1], second[1]))
    G.set_dropout(0.5, seed=11, epoch=2)
    again = epoch()
    assert again[0] == first[0]
    for a, b in zip(first[1], again[1]):
        np.testing.assert_array_equal(a, b)
    with pytest.raises(ValueError, match="attention dropout"):
        G.set_dropout(0.5, seed=11, epoch=9, attn=0.1)
    assert G.attn_dropout_p == 0.0 and G.dropout_epoch == 3             # a refused call stores nothing


def test_variant_v1_is_the_model_as_it_was(pkg):
    """gat(variant="v1") gives the bits of gat() after three epochs, and a v1 model registers no gatv2-* timer; a v2 model
    registers its four and none of v1's attention timers"""
    sizes, heads = MODELS[0]
    ctx = pkg.context(0)
    a = _run_epochs(pkg, ctx, sizes, heads, fused=True, step=True)
    b = _run_epochs(pkg, ctx, sizes, heads, fused=True, step=True, variant="v1")
    assert a[0] == b[0]
    for x, y in zip(a[1], b[1]):
        np.testing.assert_array_equal(x, y)
    assert not [t for t in ctx.timers if "gatv2" in t], sorted(ctx.timers)
    ctx2 = pkg.context(0)
    c = _run_epochs(pkg, ctx2, sizes, heads, fused=True, step=True, epochs=1, variant="v2")
    assert c[0] != a[0][:1]
    mine = sorted(t for t in ctx2.timers if "gat" in t)
    assert mine == sorted(f"{li}_{s}" for li in range(3) for s in ("0_gatv2-forward", "1_gatv2-backward-dst",
                                                                  "1_gatv2-att-grad", "1_gatv2-backward-src")), mine
