"""The GAT kernels (include/mggcn.h: mggcn_gat_*) and the gat model on the device, against the fp64 restatement and the
reference model of gat_ref.py.  The bar is the project's TOL = 1e-4 on the matrix-normalised distance; the fp32 twin's own
distance is printed next to the device's and must be within a third of the bar first, so that a failure says whether the
input or a kernel is at fault.  Everything that is claimed bitwise is compared as bits."""
import numpy as np
import pytest

import bce_ref
import gat_ref as ref
from gat_ref import relerr

pytestmark = pytest.mark.gpu

TOL = 1e-4
SHAPES = [(1, 1), (5, 1), (3, 7), (1, 41), (4, 32), (2, 65), (1, 128), (8, 32), (16, 64)]
COLSUM_BLOCKS = 512          # csrc/gat.hip kGatColsumBlocks: the grid cap of the G_att partial pass


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


@pytest.fixture(scope="module")
def graph():
    return ref.kernel_graph()


def _torch():
    import torch
    return torch


class _dense:
    """a device matrix of ``rows x d`` floats at leading dimension d + pad, its base ``offset`` floats past a 16-byte
    aligned allocation; pre-filled with ``fill``"""

    def __init__(self, rows, d, offset=0, pad=0, host=None, fill=123.0):
        torch = _torch()
        self.rows, self.d, self.ld = rows, d, d + pad
        self.flat = torch.full((rows * self.ld + offset + 4,), fill, dtype=torch.float32, device="cuda")
        self.view = self.flat[offset:offset + rows * self.ld].view(rows, self.ld)[:, :d] if rows else self.flat[:0].view(0, d)
        if host is not None and rows:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(host, dtype=np.float32)))
        self.ptr = self.flat.data_ptr() + 4 * offset

    def numpy(self):
        return self.view.cpu().numpy().copy()


def _u32(a):
    return _torch().from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def run_device(ctx, indptr, indices, Z, att, K, G, Z_dst=None, offset=0, pad=0, slope=ref.SLOPE, n_src=None, off=None):
    """every entry point once, through the C ABI with raw pointers; returns the outputs of ref.NAMES as numpy arrays.
    ``off``: {"Z" | "G" | "out" | "G_Z" | "att": floats} moves the base of that operand alone, in place of ``offset``"""
    torch = _torch()
    lib, st = ctx.lib, ctx.stream(0)
    n = indptr.size - 1
    n_src = Z.shape[0] if n_src is None else n_src
    d = Z.shape[1]
    dh = d // K
    square = Z_dst is None
    t_indptr, t_indices = ref.transpose_pattern(indptr, indices, n_src)
    ip, ix, tip, tix = _u32(indptr), _u32(indices), _u32(t_indptr), _u32(t_indices)
    o = dict(dict.fromkeys(("Z", "G", "out", "G_Z", "att"), offset), **(off or {}))
    Zs = _dense(n_src, d, o["Z"], pad, Z)
    Zd = Zs if square else _dense(n, d, o["Z"], pad, Z_dst)
    Gd = _dense(n, d, o["G"], pad, G)
    at = _dense(2, d, o["att"], 0, att)
    out, G_Z = _dense(n, d, o["out"], pad), _dense(n_src, d, o["G_Z"], pad)
    small = {k: _dense(n if k in ("s_dst", "lse", "D", "ds_dst") else n_src, K) for k in
             ("s_dst", "s_src", "lse", "D", "ds_dst", "ds_src")}
    G_att = _dense(2, d)
    torch.cuda.synchronize()
    if square:
        lib.mggcn_gat_scores_f32(st, Zs.ptr, Zs.ld, at.ptr, small["s_dst"].ptr, small["s_src"].ptr, n_src, K, dh)
    else:
        lib.mggcn_gat_scores_f32(st, Zd.ptr, Zd.ld, at.ptr, small["s_dst"].ptr, None, n, K, dh)
        lib.mggcn_gat_scores_f32(st, Zs.ptr, Zs.ld, at.ptr, None, small["s_src"].ptr, n_src, K, dh)
    lib.mggcn_gat_forward_f32(st, n, n_src, ip.data_ptr(), ix.data_ptr(), Zs.ptr, Zs.ld, small["s_dst"].ptr,
                              small["s_src"].ptr, K, dh, slope, out.ptr, out.ld, small["lse"].ptr)
    lib.mggcn_gat_backward_dst_f32(st, n, n_src, ip.data_ptr(), ix.data_ptr(), Zs.ptr, Zs.ld, small["s_dst"].ptr,
                                   small["s_src"].ptr, small["lse"].ptr, Gd.ptr, Gd.ld, out.ptr, out.ld, K, dh, slope,
                                   small["D"].ptr, small["ds_dst"].ptr)
    lib.mggcn_gat_backward_src_f32(st, n_src, n, tip.data_ptr(), tix.data_ptr(), Zs.ptr, Zs.ld, small["s_dst"].ptr,
                                   small["s_src"].ptr, small["lse"].ptr, small["D"].ptr, Gd.ptr, Gd.ld, at.ptr,
                                   small["ds_dst"].ptr if square else None, K, dh, slope, small["ds_src"].ptr, G_Z.ptr, G_Z.ld)
    lib.mggcn_gat_scores_backward_f32(st, small["ds_dst"].ptr, Zd.ptr, Zd.ld, n, small["ds_src"].ptr, Zs.ptr, Zs.ld, n_src,
                                      K, dh, G_att.ptr)
    ctx.sync()
    res = {k: small[k].numpy() for k in ("s_dst", "s_src", "lse", "D", "ds_dst", "ds_src")}
    res.update(out=out.numpy(), G_Z=G_Z.numpy(), G_att=G_att.numpy())
    return res


def _tolerance_case(ctx, indptr, indices, K, dh, n_src=320, offset=0, pad=0, what=""):
    n = indptr.size - 1
    Z, Z_dst, G, att = ref.tolerance_inputs(n, n_src, K, dh)
    Zd = None if n == n_src else Z_dst
    got = run_device(ctx, indptr, indices, Z, att, K, G, Z_dst=Zd, offset=offset, pad=pad)
    want = ref.restate64(indptr, indices, Z, att, K, G=G, Z_dst=Zd)
    twin = ref.twin32(indptr, indices, Z, att, K, G=G, Z_dst=Zd)
    for name in ref.NAMES:
        dt, dg = relerr(twin[name], want[name]), relerr(got[name], want[name])
        print(f"[gat] {what}K={K} dh={dh} offset={offset} pad={pad} {name}: twin {dt:.3e} device {dg:.3e} (bar {TOL:.0e})")
        assert dt <= TOL / 3, ("the input is ill-conditioned for this bar", name, K, dh, dt)
        assert dg <= TOL, (name, K, dh, offset, pad, dg, "twin:", dt)
    return got, (Z, G, att)


# ---- kernel level ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,dh", SHAPES)
def test_every_entry_point_against_the_restatement(ctx, graph, K, dh):
    """(1) s_dst, s_src, out, lse, D, ds_dst, ds_src, G_Z and G_att within the bar on the kernel-test graph"""
    _tolerance_case(ctx, *graph, K, dh)


def test_misaligned_operands_take_the_element_path(ctx, graph):
    """(2) base pointers one float off 16-byte alignment and a leading dimension of d + 3 at (4, 32)"""
    aligned, _ = _tolerance_case(ctx, *graph, 4, 32)
    off, _ = _tolerance_case(ctx, *graph, 4, 32, offset=1, pad=3)
    for name in ref.NAMES:                          # two reduction orders of the same numbers
        assert relerr(off[name], aligned[name]) <= TOL, name


def test_rectangular_block(ctx):
    """(3) 200 destinations x 320 sources: separate index spaces, no ds_dst term in G_Z"""
    indptr, indices = ref.kernel_graph(200, 320)
    _tolerance_case(ctx, indptr, indices, 4, 32, what="200 x 320 ")
    _tolerance_case(ctx, indptr, indices, 3, 7, what="200 x 320 ")


@pytest.mark.parametrize("K,dh", [(4, 32), (3, 7)])
def test_empty_rows_one_entry_rows_and_unreferenced_columns(ctx, graph, K, dh):
    """(4) rows without entries give out = +0.0 and lse = 0, written over the 123.0 the buffers held; an unreferenced
    column's G_Z row is ds_dst * att[0] alone.  (5) the one-entry row copies its source row bit for bit (alpha = 1)"""
    indptr, indices = graph
    got, (Z, G, att) = _tolerance_case(ctx, indptr, indices, K, dh)
    for r in (0, 319):
        assert indptr[r] == indptr[r + 1]
        np.testing.assert_array_equal(got["out"][r].view(np.uint32), np.zeros(K * dh, dtype=np.uint32))
        np.testing.assert_array_equal(got["lse"][r].view(np.uint32), np.zeros(K, dtype=np.uint32))
        np.testing.assert_array_equal(got["ds_dst"][r], np.zeros(K, dtype=np.float32))
    u = ref.UNREFERENCED
    np.testing.assert_array_equal(got["ds_src"][u], np.zeros(K, dtype=np.float32))
    np.testing.assert_array_equal(got["G_Z"][u], (np.repeat(got["ds_dst"][u], dh) * att[0]).astype(np.float32))
    assert indptr[2] - indptr[1] == 1
    np.testing.assert_array_equal(got["out"][1].view(np.uint32), Z[indices[indptr[1]]].view(np.uint32))


@pytest.mark.parametrize("K,dh", [(4, 32), (3, 7)])
def test_scores_in_the_thousands_stay_finite_and_convex(ctx, graph, K, dh):
    """(6) att x 300: |score| in the hundreds to thousands.  Every output is finite, and every out[i, c] lies between the
    smallest and the largest gathered Z[j, c], widened by 1e-5 max|Z| -- a convex combination, whatever the scores are"""
    indptr, indices = graph
    Z, _, G, att = ref.tolerance_inputs(320, 320, K, dh, att_scale=30.0)        # 300 x the tolerance inputs' 0.1
    got = run_device(ctx, indptr, indices, Z, att, K, G)
    assert np.abs(got["s_dst"]).max() > 100
    for name in ref.NAMES:
        assert np.isfinite(got[name]).all(), name
    slack = 1e-5 * np.abs(Z).max()
    for r in range(320):
        b, e = int(indptr[r]), int(indptr[r + 1])
        if b == e:
            continue
        rows = Z[indices[b:e]]
        assert (got["out"][r] >= rows.min(axis=0) - slack).all() and (got["out"][r] <= rows.max(axis=0) + slack).all(), r


@pytest.mark.parametrize("K,dh,offset", [(4, 32, 0), (3, 7, 0), (16, 64, 0), (4, 32, 1)])
def test_two_calls_give_the_same_bits(ctx, graph, K, dh, offset):
    """(7) every output, G_att included"""
    indptr, indices = graph
    Z, _, G, att = ref.tolerance_inputs(320, 320, K, dh)
    a = run_device(ctx, indptr, indices, Z, att, K, G, offset=offset)
    b = run_device(ctx, indptr, indices, Z, att, K, G, offset=offset)
    for name in ref.NAMES:
        np.testing.assert_array_equal(a[name].view(np.uint32), b[name].view(np.uint32), err_msg=name)


def test_no_rows(ctx):
    """(8) n_rows = 0 returns; the backward still writes G_att as zeros"""
    indptr, indices = np.zeros(1, dtype=np.uint32), np.zeros(0, dtype=np.uint32)
    Z = np.zeros((0, 12), dtype=np.float32)
    att = np.ones((2, 12), dtype=np.float32)
    got = run_device(ctx, indptr, indices, Z, att, 3, Z)
    np.testing.assert_array_equal(got["G_att"].view(np.uint32), np.zeros((2, 12), dtype=np.uint32))
    assert got["out"].shape == (0, 12)


def test_more_rows_than_one_pass_of_the_column_sums(ctx):
    """(9) the one capped grid is the partial pass of G_att: at (4, 32) a workgroup takes 2 rows at a time and the cap is
    COLSUM_BLOCKS, so one pass covers 1024 rows.  2500 rows of two entries each: every row output is compared row by row,
    and G_att from rows beyond the first pass alone must still arrive"""
    n, K, dh = 2500, 4, 32
    assert n > 2 * COLSUM_BLOCKS * 2
    rng = np.random.default_rng(5)
    indptr = (2 * np.arange(n + 1)).astype(np.uint32)
    indices = rng.integers(0, n, size=2 * n).astype(np.uint32)
    Z, _, G, att = ref.tolerance_inputs(n, n, K, dh)
    got = run_device(ctx, indptr, indices, Z, att, K, G)
    want = ref.restate64(indptr, indices, Z, att, K, G=G)
    for name in ref.NAMES:
        w = want[name].astype(np.float64)
        rows = np.abs(got[name] - w).max(axis=1) / np.abs(w).max()
        print(f"[gat] 2500 rows {name}: worst row {int(rows.argmax())} at {rows.max():.3e}")
        assert rows.max() <= TOL, (name, int(rows.argmax()), rows.max())
    # the column sums of the rows past the first pass only
    lib, st = ctx.lib, ctx.stream(0)
    ds = rng.standard_normal((n, K)).astype(np.float32)
    ds[:2 * COLSUM_BLOCKS] = 0
    dsd, Zd, G_att = _dense(n, K, host=ds), _dense(n, K * dh, host=Z), _dense(2, K * dh)
    lib.mggcn_gat_scores_backward_f32(st, dsd.ptr, Zd.ptr, Zd.ld, n, dsd.ptr, Zd.ptr, Zd.ld, n, K, dh, G_att.ptr)
    ctx.sync()
    w = (np.repeat(ds.astype(np.float64), dh, axis=1) * Z).sum(axis=0)
    assert relerr(G_att.numpy()[0], w) <= TOL and relerr(G_att.numpy()[1], w) <= TOL


# ---- model level -------------------------------------------------------------------------------------------------------------------
N = 1024
MODELS = [([48, 32, 32, 7], 4), ([16, 64, 8, 5], 2), ([608, 128, 128, 41], 8)]


def _model_data(pkg, sizes, seed=0):
    ip, ix, dv = pkg.datasets.synth_powerlaw_csr(N, N * 24, 1200, seed=len(sizes) + sizes[0])
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, sizes[0]), dtype=np.float32)
    Y = rng.integers(0, sizes[-1], size=(N, 1)).astype(np.int32)
    return (ip, ix, dv), X, Y


def _gat(pkg, csr, sizes, heads, **kw):
    ip, ix, dv = csr
    return pkg.gat(pkg.csr_matrix(ip.copy(), ix.copy(), dv.copy(), N), sizes, heads=heads, **kw)


def _oracle(oracle, csr, sizes, heads, **kw):
    ip, ix, dv = csr
    per_layer = [heads] * (len(sizes) - 2) + [1]
    return ref.oracle_gat(oracle, oracle.Csr(ip.copy(), ix.copy(), dv.copy(), N), sizes, per_layer, **kw)


def _sync_oracle_state(G, O):
    """identical inputs for the next epoch, as test_gpu_gcn.py does: the reference takes over the device's parameters and
    Adam moments"""
    for layer, ol in zip(G.layers(), O.layers):
        ol.lin.W, ol.lin.b = layer.W().numpy().copy(), layer.b().numpy().copy()
        ol.att = layer.att().numpy().copy()
        if layer.lin.mW is not None:
            ol.lin.mW, ol.lin.vW = layer.lin.mW.numpy().copy(), layer.lin.vW.numpy().copy()
            ol.lin.mb, ol.lin.vb = layer.lin.mb.numpy().copy(), layer.lin.vb.numpy().copy()
            ol.lin.step = layer.lin.step
        if layer.attn.m is not None:
            ol.m, ol.v, ol.step = layer.attn.m.numpy().copy(), layer.attn.v.numpy().copy(), layer.attn.step


def _grads(G):
    return [(l.GW().numpy().copy(), l.Gb().numpy().copy(), l.Gatt().numpy().copy()) for l in G.layers()]


def _assert_grads(what, mine, theirs):
    for li, (g, o) in enumerate(zip(mine, theirs)):
        for name, a, b in zip(("G_W", "G_b", "G_att"), g, o):
            d = relerr(a, b)
            print(f"[gat] {what} layer {li} {name}: {d:.3e}")
            assert d <= TOL, (what, li, name, d)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("sizes,heads", MODELS)
def test_gat_epochs_match_the_reference(pkg, oracle, ctx, fused, sizes, heads):
    """three full epochs (forward, loss, backward, Adam) against the reference model on identical inputs, the rules of
    test_gcn_epochs_match_oracle: loss at TOL, accuracy within 3 / n, every G_W, G_b and G_att at TOL, every updated W and
    att never more than a sign flip away and at TOL in the well-conditioned entries"""
    csr, X, Y = _model_data(pkg, sizes)
    G = _gat(pkg, csr, sizes, heads, fused=fused)
    O = _oracle(oracle, csr, sizes, heads)
    for layer, ol in zip(G.layers(), O.layers):                     # same seed-99 init, bit for bit
        np.testing.assert_array_equal(layer.W().numpy(), ol.lin.W)
        np.testing.assert_array_equal(layer.b().numpy(), ol.lin.b)
        np.testing.assert_array_equal(layer.att().numpy(), ol.att)
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
        print(f"[gat] sizes={sizes} fused={fused} epoch {epoch}: loss {loss!r} (reference {ol!r}), acc {acc!r} ({oa!r})")
        assert abs(loss - ol) <= TOL * abs(ol), (epoch, loss, ol)
        assert abs(acc - oa) <= 3.0 / N, (epoch, acc, oa)
        _assert_grads(f"sizes={sizes} fused={fused} epoch {epoch}", grads, ograds)
        for li, (layer, olayer) in enumerate(zip(G.layers(), O.layers)):
            for name, P, Po, g in (("W", layer.W().numpy(), olayer.lin.W, ograds[li][0]),
                                   ("att", layer.att().numpy(), olayer.att, ograds[li][2])):
                assert np.abs(P - Po).max() <= 2.05 * lr, (epoch, li, name)          # never more than a sign flip
                solid = np.abs(g) > 1e-2 * np.abs(g).max()                          # well-conditioned entries
                assert np.abs(P - Po)[solid].max() <= TOL * np.abs(Po).max(), (epoch, li, name)


def _state_bits(G):
    out = []
    for l in G.layers():
        for t in (l.W(), l.b(), l.att(), l.GW(), l.Gb(), l.Gatt(), l.lin.mW, l.lin.vW, l.lin.mb, l.lin.vb, l.attn.m, l.attn.v):
            out.append(t.numpy().view(np.uint32).copy())
    return out


def _run_epochs(pkg, ctx, sizes, heads, fused, step, epochs=3):
    csr, X, Y = _model_data(pkg, sizes)
    G = _gat(pkg, csr, sizes, heads, fused=fused)
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


@pytest.mark.parametrize("sizes,heads", MODELS[:2])
def test_fused_and_train_step_give_the_same_bits(pkg, ctx, sizes, heads):
    """fused=True against fused=False, and train_step against train_forward + backward + adam_update: the same losses and
    the same bits in every parameter, gradient and Adam moment after three epochs"""
    base = _run_epochs(pkg, ctx, sizes, heads, fused=False, step=False)
    for fused, step in ((True, False), (True, True), (False, True)):
        res, bits = _run_epochs(pkg, ctx, sizes, heads, fused=fused, step=step)
        assert res == base[0], (fused, step)
        for a, b in zip(bits, base[1]):
            np.testing.assert_array_equal(a, b)
    assert base[0][-1][0] < base[0][0][0], base[0]                 # and it trains


def test_bce_epoch_matches_the_reference(pkg, oracle, ctx):
    """loss="bce": one epoch against the reference model with the fp32 restatement of the multi-label loss"""
    sizes, heads = [48, 32, 32, 7], 4
    csr, X, _ = _model_data(pkg, sizes)
    T = (np.random.default_rng(3).random((N, sizes[-1])) < 0.2).astype(np.int32)
    G = _gat(pkg, csr, sizes, heads, loss="bce")

    def loss(H):
        return (np.ascontiguousarray(bce_ref.grad32(H, T, 1.0 / (float(N) * H.shape[1]))),
                (float(bce_ref.loss32(H, T).astype(np.float64).sum() / (N * H.shape[1])), bce_ref.micro_f1(*bce_ref.counts(H, T)[0])))
    O = _oracle(oracle, csr, sizes, heads, loss=loss)
    got = G.train_forward(ctx, pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(T))
    G.backward(ctx)
    ctx.sync()
    want = O.train_forward(X, None)
    O.backward()
    print(f"[gat] bce: (loss, micro-F1) {got!r} (reference {want!r})")
    assert abs(got[0] - want[0]) <= TOL * abs(want[0])
    assert got[1] == want[1] or abs(got[1] - want[1]) <= 3.0 / N
    _assert_grads("bce", _grads(G), [(l.lin.G_W, l.lin.G_b, l.G_att) for l in O.layers])


def test_splits_epoch_matches_the_reference(pkg, oracle, ctx):
    """set_splits: one epoch against the reference model with the loss over the training rows only (the oracle's softmax
    cross-entropy scaled by 1 / n_train, the gradient rows of the other sets zeroed)"""
    sizes, heads = [48, 32, 32, 7], 4
    csr, X, Y = _model_data(pkg, sizes)
    S = np.random.default_rng(4).choice(4, size=N, p=(0.5, 0.2, 0.25, 0.05)).astype(np.int32)
    train = S == 0
    G = _gat(pkg, csr, sizes, heads)
    G.set_splits(S)

    def loss(H):
        _, _, Gr, Pr = oracle.softmax_cross_entropy(H, Y, n_global=int(train.sum()))
        Gr[~train] = 0
        y = Y.reshape(-1)
        nll = np.abs(np.log(Pr.astype(np.float64)[np.arange(N), y]))
        hit = Pr.argmax(axis=1) == y
        return Gr, (float(nll[train].sum() / train.sum()), float(hit[train].sum() / train.sum()))
    O = _oracle(oracle, csr, sizes, heads, loss=loss)
    got = G.train_forward(ctx, pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y))
    assert got == G.split_metrics()["train"] and G.split_metrics()["counts"]["train"] == int(train.sum())
    G.backward(ctx)
    ctx.sync()
    want = O.train_forward(X, Y)
    O.backward()
    print(f"[gat] splits: (loss, acc) {got!r} (reference {want!r})")
    assert abs(got[0] - want[0]) <= TOL * abs(want[0])
    assert abs(got[1] - want[1]) <= 3.0 / int(train.sum())
    _assert_grads("splits", _grads(G), [(l.lin.G_W, l.lin.G_b, l.G_att) for l in O.layers])


def test_evaluate_agrees_with_a_plain_forward(pkg, ctx):
    sizes, heads = [48, 32, 32, 7], 4
    csr, X, Y = _model_data(pkg, sizes)
    S = np.random.default_rng(4).choice(3, size=N).astype(np.int32)
    G = _gat(pkg, csr, sizes, heads)
    Xd, Yd, Sd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y), pkg.dn_matrix.from_numpy(S.reshape(-1, 1))
    res = G.evaluate(ctx, Xd, Yd, Sd)
    out = G(ctx, Xd)
    ctx.sync()
    hit = out.numpy().argmax(axis=1) == Y.reshape(-1)
    assert res["all"] == float(hit.mean())
    for k, name in enumerate(("train", "val", "test")):
        assert res[name] == float(hit[S == k].mean())


def test_attention_is_not_a_no_op(pkg, ctx):
    """with att = 0 a layer's output is the plain mean of Z over each row's entries, within the bar; with the trained att it
    is more than 100 x the bar away from that mean"""
    sizes, heads = [48, 32, 7], 4
    csr, X, Y = _model_data(pkg, sizes)
    G = _gat(pkg, csr, sizes, heads)
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    for _ in range(3):
        G.train_step(ctx, Xd, Yd, 1e-2, 0.9, 0.999, 5e-4, 1e-8)
    L = G.layers()[0]
    F = G.A_T
    trained = L.att().numpy().copy()
    dist = {}
    for name, att in (("zero", np.zeros_like(trained)), ("trained", trained)):
        L.attn.init(att)
        G(ctx, Xd)
        ctx.sync()
        dist[name] = relerr(L.out.numpy(), ref.row_mean(F.indptr, F.indices, L.Z.numpy()))
        print(f"[gat] att {name}: distance of the layer output to the row mean {dist[name]:.3e}")
    assert dist["zero"] <= TOL
    assert dist["trained"] > 100 * TOL
