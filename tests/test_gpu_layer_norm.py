"""Layer normalisation on the device: mggcn_layer_norm_forward_f32 / _backward_f32 against the fp64 restatement
(layernorm_ref.py) on both kernel paths, the rows where eps decides, the flag against separate launches, in place,
misaligned, shard by shard and beyond one grid pass; the model against the wrapped oracle; timers, evaluation and the CLI.

Grid cap of both kernels: kLayerNormBlocks = 4 x 256 CUs = 1024 workgroups of 256 threads.  A row belongs to a group of L
lanes, R rows in flight per group, so a pass of the capped grid covers 1024 x (256 / L) x R rows:
  m = 128, float4 path (L = 16, R = 1) and m = 41, element path (L = 16, R = 1): 16 384 rows
  m = 128 behind a misaligned pointer, element path (L = 64, R = 2):                 8 192 rows"""
import io
import os
import subprocess

import numpy as np
import pytest

import dropout_ref
import layernorm_ref as ref
from test_gpu_agg_bf16 import GRAD_BAR, GRAD_BAR_REST, _bf16_oracle
from test_gpu_gcn import TOL, _graph, relerr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mg-gcn_amd", "bin")
ADAM = ref.ADAM
LEAKY = 1
WIDTHS = [16, 41, 64, 128, 130, 256, 1024]
NAMES = ("y", "xhat", "rstd", "G_in", "G_gamma", "G_beta")


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


def _torch():
    import torch
    return torch


# ---- the kernels --------------------------------------------------------------------------------------------------------
def _dev(a, offset=0, fill=None):
    """a device copy of ``a`` (or ``fill`` everywhere) whose first element sits ``offset`` floats into an aligned
    allocation (offset = 1: no 16-byte alignment, the element path at any m); returns the view"""
    torch = _torch()
    a = np.ascontiguousarray(a, dtype=np.float32)
    t = torch.full((offset + a.size,), 123.0 if fill is None else fill, dtype=torch.float32, device="cuda")
    if fill is None:
        t[offset:] = torch.from_numpy(a.reshape(-1)).cuda()
    return t[offset:]


def _host(t, shape):
    return t.cpu().numpy().reshape(shape)


def _forward(ctx, x, gamma, beta, flags, offset=0, in_place=False):
    n, m = x.shape
    X, g, b = _dev(x, offset), _dev(gamma), _dev(beta)
    Y = X if in_place else _dev(x, offset, fill=123.0)
    xhat, rstd = _dev(x, offset, fill=123.0), _dev(np.zeros(n), fill=123.0)
    _torch().cuda.synchronize()
    ctx.lib.mggcn_layer_norm_forward_f32(ctx.stream(0), X.data_ptr(), Y.data_ptr(), xhat.data_ptr(), rstd.data_ptr(),
                                         g.data_ptr(), b.data_ptr(), n, m, ref.EPS, flags)
    ctx.sync()
    return _host(Y, (n, m)), _host(xhat, (n, m)), _host(rstd, (n,))


def _backward(ctx, G, act, xhat, rstd, gamma, flags, offset=0, in_place=None):
    """in_place: None, "G" or "act" -- the operand G_in aliases"""
    n, m = G.shape
    Gd, A, xh = _dev(G, offset), _dev(act, offset), _dev(xhat, offset)
    rs, g = _dev(rstd), _dev(gamma)
    G_in = {None: _dev(G, offset, fill=123.0), "G": Gd, "act": A}[in_place]
    Gg, Gb = _dev(np.zeros(m), fill=123.0), _dev(np.zeros(m), fill=123.0)
    _torch().cuda.synchronize()
    ctx.lib.mggcn_layer_norm_backward_f32(ctx.stream(0), Gd.data_ptr(), A.data_ptr(), xh.data_ptr(), rs.data_ptr(),
                                          g.data_ptr(), G_in.data_ptr(), Gg.data_ptr(), Gb.data_ptr(), n, m, flags)
    ctx.sync()
    return _host(G_in, (n, m)), _host(Gg, (1, m)), _host(Gb, (1, m))


def _both(ctx, x, G, gamma, beta, flags, offset=0):
    """forward, then backward with the forward's y as the sign source: the six results in the order of NAMES"""
    y, xhat, rstd = _forward(ctx, x, gamma, beta, flags, offset)
    return (y, xhat, rstd) + _backward(ctx, G, y, xhat, rstd, gamma, flags, offset)


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    bad = np.flatnonzero(got.view(np.uint32).reshape(-1) != want.view(np.uint32).reshape(-1))
    assert bad.size == 0, (what, bad[:8], got.reshape(-1)[bad[:8]], want.reshape(-1)[bad[:8]], bad.size)


def _case(n, m, shift=0.0, scale=1.0):
    rng = np.random.default_rng(1000 * m + n)
    x = (shift + scale * rng.standard_normal((n, m))).astype(np.float32)
    G = rng.standard_normal((n, m)).astype(np.float32)
    gamma, beta = ref.params(m, m)
    return x, G, gamma, beta


def _references(x, G, act, gamma, beta, leaky):
    """(the fp64 restatement, the fp32 twin) of the six results, both with ``act`` as the sign source"""
    want = ref.forward64(x, gamma, beta, leaky) + ref.backward64(G, act, x, gamma, leaky)
    y, xhat, rstd = ref.forward32(x, gamma, beta, leaky)
    return want, (y, xhat, rstd) + ref.backward32(G, act, xhat, rstd, gamma, leaky)


def _tolerance_case(ctx, m, bar, dist, shift=0.0, n=37, offset=0):
    """the twin within a third of the bar first (so a failure says whether the input or the kernel is at fault), then the
    device within the bar; both distances are printed"""
    x, G, gamma, beta = _case(n, m, shift)
    got = _both(ctx, x, G, gamma, beta, LEAKY, offset)
    want, twin = _references(x, G, got[0], gamma, beta, True)
    for what, g, t, w in zip(NAMES, got, twin, want):
        dt, dg = dist(t, w), dist(g, w)
        print(f"[layer norm] m={m} shift={shift} offset={offset} {what}: twin {dt:.3e} device {dg:.3e} (bar {bar:.0e})")
        assert dt <= bar / 3, ("the input is ill-conditioned for this bar", what, m, dt)
        assert dg <= bar, (what, m, shift, offset, dg, "twin:", dt)
    return got


@pytest.mark.parametrize("m", WIDTHS)
def test_standard_normal_rows(ctx, m):
    _tolerance_case(ctx, m, 1e-5, ref.rowdist)


@pytest.mark.parametrize("m", WIDTHS)
def test_rows_far_from_zero_need_the_two_pass_variance(ctx, m):
    """rows 100 + N(0, 1): E[x^2] - mean^2 in fp32 is off by >= 1.5e-3 here (test_layer_norm_cpu.py shows it on the host)"""
    _tolerance_case(ctx, m, TOL, ref.rowdist, shift=100.0)


@pytest.mark.parametrize("m", [3, 4])
def test_tiny_widths(ctx, m):
    """row-normalised G_in is ill-conditioned at these widths (the twin reaches 8.5e-4 at m = 3): matrix-normalised"""
    _tolerance_case(ctx, m, TOL, relerr)


def test_misaligned_pointers_take_the_element_path(ctx):
    aligned = _tolerance_case(ctx, 128, 1e-5, ref.rowdist)
    off = _tolerance_case(ctx, 128, 1e-5, ref.rowdist, offset=1)
    for what, a, b in zip(NAMES, aligned, off):                     # two reduction orders of the same numbers
        assert ref.rowdist(b, a) <= 1e-5, what


@pytest.mark.parametrize("flags", [0, LEAKY])
def test_width_one(ctx, flags):
    x, G, gamma, beta = _case(37, 1)
    y, xhat, rstd, G_in, G_gamma, G_beta = _both(ctx, x, G, gamma, beta, flags)
    _same_bits(xhat, np.zeros_like(x), "xhat == 0")
    _same_bits(G_in, np.zeros_like(x), "G_in == 0")
    assert np.abs(rstd - np.float32(1 / np.sqrt(ref.EPS))).max() <= 1e-6 * rstd.max()
    if not flags:
        _same_bits(y, np.broadcast_to(beta, x.shape), "y == beta")
        assert relerr(G_beta, G.astype(np.float64).sum(axis=0, keepdims=True)) <= 1e-5
    _same_bits(G_gamma, np.zeros((1, 1), dtype=np.float32), "G_gamma == 0")


@pytest.mark.parametrize("m", [41, 128])
def test_constant_rows(ctx, m):
    x = np.full((37, m), 3.0, dtype=np.float32)
    _, G, gamma, beta = _case(37, m)
    y, xhat, rstd = _forward(ctx, x, gamma, beta, 0)
    assert ((xhat.view(np.uint32) & 0x7FFFFFFF) == 0).all()                          # +-0
    _same_bits(y, np.broadcast_to(beta, x.shape), "y == beta")
    assert np.abs(rstd - np.float32(1 / np.sqrt(ref.EPS))).max() <= 1e-6 * np.float32(1 / np.sqrt(ref.EPS))


@pytest.mark.parametrize("m", [41, 128])
def test_variance_near_eps(ctx, m):
    """rows 1 + 1e-3 N(0, 1): the variance is about eps / 10, so leaving eps out or misplacing it is off by a factor"""
    x, G, gamma, beta = _case(37, m, shift=1.0, scale=1e-3)
    var = x.astype(np.float64).var(axis=1)
    assert (var < ref.EPS / 5).all() and (var > ref.EPS / 20).all()
    _, _, rstd = _forward(ctx, x, gamma, beta, 0)
    want, twin = ref.forward64(x, gamma, beta)[2], ref.forward32(x, gamma, beta)[2]
    print(f"[layer norm] m={m} variance near eps: twin {relerr(twin, want):.3e} device {relerr(rstd, want):.3e}")
    assert relerr(twin, want) <= 1e-5 / 3
    assert np.abs(rstd - want).max() <= 1e-5 * want.max() and (np.abs(rstd / want - 1) <= 1e-5).all()
    assert (np.abs(1 / np.sqrt(var) / want - 1) > 0.5).all()                          # what a missing eps would give


@pytest.mark.parametrize("m,offset", [(41, 0), (128, 0), (128, 1)])
def test_flag_equals_separate_launches(ctx, m, offset):
    """forward with the flag == forward without it + mggcn_leaky_relu_forward_f32; backward with the flag ==
    mggcn_leaky_relu_backward_f32 + backward without it: bit for bit"""
    n = 37
    x, G, gamma, beta = _case(n, m)
    y1, xhat1, rstd1 = _forward(ctx, x, gamma, beta, LEAKY, offset)
    z, xhat0, rstd0 = _forward(ctx, x, gamma, beta, 0, offset)
    Z = _dev(z, offset)
    _torch().cuda.synchronize()                                               # the library's streams do not wait for torch's
    ctx.lib.mggcn_leaky_relu_forward_f32(ctx.stream(0), Z.data_ptr(), Z.data_ptr(), n * m, 0.01)
    ctx.sync()
    _same_bits(y1, _host(Z, (n, m)), "y")
    _same_bits(xhat1, xhat0, "xhat")
    _same_bits(rstd1, rstd0, "rstd")
    assert (y1 != z).any()
    fused = _backward(ctx, G, y1, xhat1, rstd1, gamma, LEAKY, offset)
    A, Gd = _dev(y1, offset), _dev(G, offset)
    _torch().cuda.synchronize()
    ctx.lib.mggcn_leaky_relu_backward_f32(ctx.stream(0), A.data_ptr(), Gd.data_ptr(), Gd.data_ptr(), n * m, 0.01)
    ctx.sync()
    split = _backward(ctx, _host(Gd, (n, m)), y1, xhat1, rstd1, gamma, 0, offset)
    for what, a, b in zip(NAMES[3:], fused, split):
        _same_bits(a, b, what)


@pytest.mark.parametrize("m,offset", [(41, 0), (128, 0), (128, 1)])
def test_in_place(ctx, m, offset):
    x, G, gamma, beta = _case(37, m)
    y, xhat, rstd = _forward(ctx, x, gamma, beta, LEAKY, offset)
    yi, xhati, rstdi = _forward(ctx, x, gamma, beta, LEAKY, offset, in_place=True)
    for what, a, b in zip(NAMES, (yi, xhati, rstdi), (y, xhat, rstd)):
        _same_bits(a, b, ("x is y", what))
    out = _backward(ctx, G, y, xhat, rstd, gamma, LEAKY, offset)
    for alias in ("act", "G"):
        for what, a, b in zip(NAMES[3:], _backward(ctx, G, y, xhat, rstd, gamma, LEAKY, offset, in_place=alias), out):
            _same_bits(a, b, ("G_in is " + alias, what))


@pytest.mark.parametrize("m,offset", [(41, 0), (128, 0), (128, 1)])
def test_rows_alone_equal_the_slice_of_the_whole_call(ctx, m, offset):
    n = 101
    x, G, gamma, beta = _case(n, m)
    whole = _both(ctx, x, G, gamma, beta, LEAKY, offset)
    cuts = [0, 13, 14, 60, 101]
    for a, b in zip(cuts[:-1], cuts[1:]):
        part = _both(ctx, x[a:b], G[a:b], gamma, beta, LEAKY, offset)
        for what, p, w in zip(NAMES[:4], part, whole):
            _same_bits(p, w[a:b], ("rows", a, b, what))


@pytest.mark.parametrize("m", [41, 128])
def test_column_sums_are_reproducible(ctx, m):
    x, G, gamma, beta = _case(3001, m)
    y, xhat, rstd = _forward(ctx, x, gamma, beta, LEAKY)
    first = _backward(ctx, G, y, xhat, rstd, gamma, LEAKY)
    second = _backward(ctx, G, y, xhat, rstd, gamma, LEAKY)
    for what, a, b in zip(NAMES[3:], first, second):
        _same_bits(a, b, what)


def test_no_rows(ctx):
    """an empty call returns; the backward still writes zeros to G_gamma / G_beta"""
    m = 41
    x, _, gamma, beta = _case(1, m)
    bufs = [_dev(x, fill=123.0) for _ in range(4)]                              # x / y, xhat, G / G_in, act: never touched
    rstd, g, b = _dev(np.zeros(1), fill=123.0), _dev(gamma), _dev(beta)
    Gg, Gb = _dev(np.zeros(m), fill=123.0), _dev(np.zeros(m), fill=123.0)
    _torch().cuda.synchronize()
    ctx.lib.mggcn_layer_norm_forward_f32(ctx.stream(0), bufs[0].data_ptr(), bufs[0].data_ptr(), bufs[1].data_ptr(),
                                         rstd.data_ptr(), g.data_ptr(), b.data_ptr(), 0, m, ref.EPS, LEAKY)
    ctx.lib.mggcn_layer_norm_backward_f32(ctx.stream(0), bufs[2].data_ptr(), bufs[3].data_ptr(), bufs[1].data_ptr(),
                                          rstd.data_ptr(), g.data_ptr(), bufs[2].data_ptr(), Gg.data_ptr(), Gb.data_ptr(), 0, m,
                                          LEAKY)
    ctx.sync()
    for t in bufs + [rstd]:
        assert (t.cpu().numpy() == 123.0).all()
    _same_bits(_host(Gg, (1, m)), np.zeros((1, m), dtype=np.float32), "G_gamma")
    _same_bits(_host(Gb, (1, m)), np.zeros((1, m), dtype=np.float32), "G_beta")


@pytest.mark.parametrize("m,offset,per_pass", [(128, 0, 16384), (41, 0, 16384), (128, 1, 8192)])
def test_beyond_one_grid_pass(ctx, m, offset, per_pass):
    """n = two full passes of the capped grid (see the module docstring) plus 37 rows, so every workgroup carries rows of
    several passes into its partial: row for row the bits of the same call in chunks below one pass, and the column sums
    against the fp64 sums at 1e-5.  The largest operand is 16.8 MB."""
    n = 2 * per_pass + 37
    assert n * m * 4 < 20e6
    x, G, gamma, beta = _case(n, m)
    got = _both(ctx, x, G, gamma, beta, LEAKY, offset)
    step = per_pass * 5 // 8                                              # rows per chunk: below one pass
    parts = [_both(ctx, x[a:a + step], G[a:a + step], gamma, beta, LEAKY, offset) for a in range(0, n, step)]
    for k, what in enumerate(NAMES[:4]):
        _same_bits(got[k], np.concatenate([p[k] for p in parts]), ("chunks", what, m, offset))
    want = ref.forward64(x, gamma, beta, True) + ref.backward64(G, got[0], x, gamma, True)
    for what, g, w in list(zip(NAMES, got, want))[4:]:
        d = relerr(g, w)
        print(f"[layer norm] beyond one pass m={m} offset={offset} {what}: {d:.3e}")
        assert d <= 1e-5, (what, m, offset, d)


def test_ops_layer_norm_is_that_call(pkg, ctx):
    x, G, gamma, beta = _case(37, 41)
    want = _both(ctx, x, G, gamma, beta, LEAKY)
    dn = pkg.dn_matrix
    X, Gd, g, b = dn.from_numpy(x), dn.from_numpy(G), dn.from_numpy(gamma), dn.from_numpy(beta)
    xhat, rstd, Gg, Gb = dn(37, 41), dn(37, 1), dn(1, 41), dn(1, 41)
    assert pkg.ops.LAYER_NORM_EPS == ref.EPS
    pkg.ops.layer_norm(ctx, X, X, xhat, rstd, g, b, pkg.ops.LAYER_NORM_LEAKY_RELU)
    pkg.ops.layer_norm_backward(ctx, Gd, X, xhat, rstd, g, X, Gg, Gb, pkg.ops.LAYER_NORM_LEAKY_RELU)
    ctx.sync()
    for what, a, w in zip(NAMES[1:], (xhat.numpy(), rstd.numpy().reshape(-1), X.numpy(), Gg.numpy(), Gb.numpy()), want[1:]):
        _same_bits(a, w, what)


# ---- the model ----------------------------------------------------------------------------------------------------------
N, SIZES = 1536, [20, 16, 16, 5]


def _data(pkg, sizes):
    ip, ix, dv = _graph(pkg, N, N * 20, 900, seed=41)
    rng = np.random.default_rng(3)
    X = rng.standard_normal((N, sizes[0]), dtype=np.float32)
    Y = rng.integers(0, sizes[-1], size=(N, 1)).astype(np.int32)
    return (ip, ix, dv), X, Y


def _sync_oracle_state(G, O):
    """identical inputs for the next epoch: the oracle takes over the device's parameters and Adam moments"""
    for layer, ol in zip(G.layers(), O.layers):
        for lin, olin in zip(layer.linears(), ol.linears()):
            olin.W, olin.b = lin.W.numpy().copy(), lin.b.numpy().copy()
            if lin.mW is not None:
                olin.mW, olin.vW = lin.mW.numpy().copy(), lin.vW.numpy().copy()
                olin.mb, olin.vb = lin.mb.numpy().copy(), lin.vb.numpy().copy()
                olin.step = lin.step
        if layer.norm is not None:
            dn, on = layer.norm, ol.norm
            on.gamma, on.beta = dn.gamma.numpy().copy(), dn.beta.numpy().copy()
            if dn.mg is not None:
                on.mg, on.vg, on.mb, on.vb = (t.numpy().copy() for t in (dn.mg, dn.vg, dn.mb, dn.vb))
                on.step = dn.step


def _model_case(pkg, oracle, ctx, fused=True, residual=False, agg="f32", sizes=SIZES, dropout=0.0):
    """three epochs of gcn(norm="layer") against the wrapped oracle from identical state every epoch; next to every figure
    the distance of the fp32 oracle to its exact-accumulation twin is kept, as in the dropout tests"""
    (ip, ix, dv), X, Y = _data(pkg, sizes)
    G = pkg.gcn(pkg.csr_matrix(ip, ix, dv, N), sizes, residual_layer=residual, fused=fused, agg_dtype=agg, dropout=dropout,
                norm="layer")
    if dropout:
        G.set_dropout(dropout, seed=2024)
    oracles = []
    for f64acc in ((True,) if agg == "bf16" else (False, True)):
        O = (_bf16_oracle(oracle, ip, ix, dv, N, sizes, residual) if agg == "bf16"
             else oracle.Gcn(oracle.Csr(ip, ix, dv, N), sizes, f64acc=f64acc, residual_layer=residual))
        ref.oracle_layer_norm(oracle, O)
        if dropout:
            dropout_ref.oracle_dropout(O, dropout, seed=2024)              # on top of the norm wrapper
        oracles.append(O)
    O, twin = oracles[0], oracles[-1]
    assert [l.norm is not None for l in G.layers()] == [True] * (len(sizes) - 2) + [False]
    for layer, ol in zip(G.layers()[:-1], O.layers[:-1]):
        assert np.array_equal(layer.norm.gamma.numpy(), np.ones((1, layer.AHW.m()), dtype=np.float32))     # the defaults
        assert np.array_equal(layer.norm.beta.numpy(), np.zeros((1, layer.AHW.m()), dtype=np.float32))
        layer.norm.gamma.init(ol.norm.gamma)
        layer.norm.beta.init(ol.norm.beta)
    bar = (lambda li, what: GRAD_BAR.get(li, GRAD_BAR_REST) if what == "G_W" else GRAD_BAR_REST) if agg == "bf16" \
        else (lambda li, what: TOL)
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    lr = ADAM[0]

    def grads_of(layers, is_dev):
        out = []
        for l in layers:
            lin = l.lin
            row = {"G_W": lin.G_W, "G_b": lin.G_b}
            if getattr(l, "norm", None) is not None:
                row.update(G_gamma=l.norm.G_gamma, G_beta=l.norm.G_beta)
            if l.res_lin is not None:
                row.update(res_G_W=l.res_lin.G_W, res_G_b=l.res_lin.G_b)
            out.append({k: (v.numpy().copy() if is_dev else np.array(v, copy=True)) for k, v in row.items()})
        return out
    for epoch in range(3):
        for o in oracles:
            _sync_oracle_state(G, o)
        loss, acc = G.train_forward(ctx, Xd, Yd)
        G.backward(ctx)
        ctx.sync()
        got = grads_of(G.layers(), True)
        G.adam_update(ctx, *ADAM)
        ctx.sync()
        runs = []
        for o in oracles:
            ol, oa = o.train_forward(X, Y)
            o.backward()
            og = grads_of(o.layers, False)
            o.adam_update()
            runs.append((ol, oa, og))
        (ol, oa, og), (tl, _, tg) = runs[0], runs[-1]
        print(f"[layer norm] fused={fused} residual={residual} agg={agg} sizes={sizes} dropout={dropout} epoch {epoch}: "
              f"loss {loss!r} oracle {ol!r} twin {tl!r}")
        assert abs(loss - ol) <= TOL * abs(ol), (epoch, loss, ol, "oracle fp32 vs f64acc:", abs(ol - tl) / abs(tl))
        assert abs(acc - oa) <= 3.0 / N, (epoch, acc, oa)
        for li in range(len(got)):
            assert set(got[li]) == set(og[li])
            for what in got[li]:
                err, own = relerr(got[li][what], og[li][what]), relerr(og[li][what], tg[li][what])
                print(f"[layer norm]   layer {li} {what}: {err:.3e} (oracle fp32 vs f64acc {own:.3e})")
                assert err <= bar(li, what.replace("res_", "")), (epoch, li, what, err, "oracle fp32 vs f64acc:", own)
        for li, (layer, olayer) in enumerate(zip(G.layers()[:-1], O.layers[:-1])):
            assert np.abs(layer.norm.gamma.numpy() - olayer.norm.gamma).max() <= 2.05 * lr, (epoch, li)   # a sign flip at most
            assert np.abs(layer.norm.beta.numpy() - olayer.norm.beta).max() <= 2.05 * lr, (epoch, li)
    return G


def _timer_names(ctx):
    out = io.StringIO()
    ctx.dump_timers(out, "")
    return {line.split(":")[0] for line in out.getvalue().splitlines()}


@pytest.mark.parametrize("fused", [True, False])
def test_model_matches_the_wrapped_oracle(pkg, oracle, fused):
    ctx = pkg.context(0)                                                      # its own timers: the names below are this run's
    G = _model_case(pkg, oracle, ctx, fused=fused)
    names = _timer_names(ctx)
    for li in (0, 1):
        assert f"{li}_0_norm" in names and f"{li}_1_norm" in names, sorted(names)
    assert "2_0_norm" not in names and "2_1_norm" not in names               # the last layer has no activation, so no norm
    assert G.layers()[-1].norm is None


def test_residual_model_matches_the_wrapped_oracle(pkg, oracle, ctx):
    _model_case(pkg, oracle, ctx, residual=True)


def test_spmm_first_stack_matches_the_wrapped_oracle(pkg, oracle, ctx):
    _model_case(pkg, oracle, ctx, sizes=[12, 24, 16, 5])


def test_bf16_model_matches_the_wrapped_bf16_oracle(pkg, oracle, ctx):
    _model_case(pkg, oracle, ctx, agg="bf16")


def test_norm_composes_with_dropout(pkg, oracle, ctx):
    _model_case(pkg, oracle, ctx, dropout=0.5)


def test_layer_norm_is_not_a_no_op(pkg, oracle):
    """the wrapped oracle and the plain one differ by far more than the parity bar: the comparison above can tell"""
    (ip, ix, dv), X, Y = _data(pkg, SIZES)
    plain = oracle.Gcn(oracle.Csr(ip, ix, dv, N), SIZES)
    normed = oracle.Gcn(oracle.Csr(ip, ix, dv, N), SIZES)
    ref.oracle_layer_norm(oracle, normed)
    for O in (plain, normed):
        O.train_forward(X, Y)
        O.backward()
    for a, b in zip(plain.layers, normed.layers):
        assert relerr(b.lin.G_W, a.lin.G_W) > 100 * TOL, relerr(b.lin.G_W, a.lin.G_W)


def test_without_a_norm_nothing_new_is_launched(pkg, ctx):
    (ip, ix, dv), X, Y = _data(pkg, SIZES)
    ctx2 = pkg.context(0)                                                     # its own timers
    G = pkg.gcn(pkg.csr_matrix(ip, ix, dv, N), SIZES)
    assert G.norm is None and all(l.norm is None for l in G.layers())
    G.train_step(ctx2, pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y), *ADAM)
    assert not [t for t in _timer_names(ctx2) if "norm" in t]
    assert [l.params() for l in G.layers()] == [l.linears() for l in G.layers()]


@pytest.mark.parametrize("hoist", [False, True])
def test_evaluate_agrees_with_a_training_forward(pkg, ctx, hoist):
    """layer norm has no training mode: evaluate(), a plain call and train_forward run the same kernels (also with the
    first aggregation hoisted, where layer 0's norm runs after the hoisted GEMM) and splits on"""
    (ip, ix, dv), X, Y = _data(pkg, SIZES)
    rng = np.random.default_rng(9)
    S = rng.integers(0, 3, size=(N, 1)).astype(np.int32)
    G = pkg.gcn(pkg.csr_matrix(ip, ix, dv, N), SIZES, norm="layer", hoist_first_aggregation=hoist)
    assert G.layers()[0].hoist_input == hoist
    for li, layer in enumerate(G.layers()[:-1]):
        g, b = ref.params(layer.AHW.m(), 5 + li)
        layer.norm.gamma.init(g)
        layer.norm.beta.init(b)
    Xd, Yd, Sd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y), pkg.dn_matrix.from_numpy(S)
    loss, acc = G.train_forward(ctx, Xd, Yd)
    res = G.evaluate(ctx, Xd, Yd, Sd)
    assert abs(res["all"] - acc) <= 0.5 / N, (res, acc)
    H = G(ctx, Xd)
    ctx.sync()
    plain = H.numpy().copy()
    G.set_splits(S)
    tl, ta = G.train_forward(ctx, Xd, Yd)
    assert abs(ta - res["train"]) <= 0.5 / N, (ta, res)
    H = G(ctx, Xd)
    ctx.sync()
    _same_bits(H.numpy(), plain, "the forward does not depend on the mode")
    if hoist:                                                                 # the hoisted model computes the plain model's logits
        G0 = pkg.gcn(pkg.csr_matrix(ip, ix, dv, N), SIZES, norm="layer")
        for l0, l in zip(G0.layers()[:-1], G.layers()[:-1]):
            l0.norm.gamma.init(l.norm.gamma.numpy())
            l0.norm.beta.init(l.norm.beta.numpy())
        H0 = G0(ctx, Xd)
        ctx.sync()
        assert relerr(plain, H0.numpy()) <= TOL


# ---- the CLI ------------------------------------------------------------------------------------------------------------
def test_cli_layer_norm_matches_the_python_model(pkg, ctx, tmp_path):
    """MGGCN_LAYER_NORM=1 mg_gcn -P 1 -E 3: every epoch's loss is the Python model's from the parameters (gamma and beta
    included) the CLI started that epoch with; without the variable the run is another one"""
    n, F, C = 2000, 16, 5
    ip, ix, dv = pkg.datasets.synth_powerlaw_csr(n, n * 12, 300, seed=11)
    rng = np.random.default_rng(12)
    X = rng.standard_normal((n, F), dtype=np.float32)
    Y = rng.integers(0, C, size=(n, 1)).astype(np.int32)
    Y[0, 0] = C - 1
    d = tmp_path / "permuted" / "toy"
    pkg.datasets.write_dataset(str(d), ip, ix, dv, X, Y)
    exe = os.path.join(BIN, "mg_gcn")

    def run(tag, **env_add):
        env = dict(os.environ, MGGCN_DUMP_WEIGHTS=str(tmp_path / tag), **env_add)
        r = subprocess.run([exe, "-P", "1", "-E", "3", "train", str(d), "2", "16", "16"], cwd=str(tmp_path), env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        got = [tuple(float(x) for x in ln.split()) for ln in r.stderr.strip().splitlines()[3:6]]
        assert [int(g[0]) for g in got] == [0, 1, 2]
        return got
    got, plain = run("w", MGGCN_LAYER_NORM="1"), run("w0")
    assert abs(got[0][1] - plain[0][1]) > 100 * TOL * abs(plain[0][1])        # the norm is in the run
    sizes = [F, 16, 16, C]
    read = lambda e, what, li: pkg.datasets.read_dense(str(tmp_path / "w" / f"e{e}_{what}{li}.bin"), "<f4")
    assert not os.path.exists(tmp_path / "w" / "e0_gamma2.bin") and not os.path.exists(tmp_path / "w0" / "e0_gamma0.bin")
    assert np.array_equal(read(0, "gamma", 0), np.ones((1, 16), dtype=np.float32))
    assert np.array_equal(read(0, "beta", 1), np.zeros((1, 16), dtype=np.float32))
    assert np.abs(read(2, "gamma", 0) - 1).max() > 1e-3                       # Adam trains them
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    G = pkg.gcn(pkg.csr_matrix(ip, ix, dv, n), sizes, norm="layer")
    for e in range(3):
        for li, layer in enumerate(G.layers()):
            layer.W().init(read(e, "W", li))
            layer.b().init(read(e, "b", li))
            if layer.norm is not None:
                layer.norm.gamma.init(read(e, "gamma", li))
                layer.norm.beta.init(read(e, "beta", li))
        loss, acc = G.train_forward(ctx, Xd, Yd)
        assert abs(got[e][1] - loss) <= TOL * abs(loss), (e, got[e], loss)
        assert abs(got[e][2] - acc) <= 3.0 / n, (e, got[e], acc)
