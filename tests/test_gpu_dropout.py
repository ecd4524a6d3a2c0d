"""Dropout on the device: mggcn_dropout_f32 bit for bit against the numpy restatement (dropout_ref.py) on both kernel
paths, past 2^32 rows, beyond one grid pass and shard by shard; the model against the wrapped oracle; evaluation mode;
and the CLI against the Python model.

Grid cap of both kernels: stream_grid = 2048 workgroups of 256 threads = 524 288 threads, one float4 (four columns) or one
element each per pass: 16 384 rows of m = 128 on the float4 path, 12 787.5 rows of m = 41 on the element path."""
import os
import subprocess

import numpy as np
import pytest

import dropout_ref
from test_gpu_agg_bf16 import GRAD_BAR, GRAD_BAR_REST, W_SOLID_BAR, _bf16_oracle
from test_gpu_gcn import TOL, _graph, relerr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mg-gcn_amd", "bin")
GRID_THREADS = 2048 * 256
ADAM = (1e-2, 0.9, 0.999, 5e-4, 1e-8)
SPECIALS = np.array([0x7FC00000, 0x7F800000, 0xFF800000, 0x80000000], dtype=np.uint32).view(np.float32)   # NaN, +-inf, -0.0


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


def _torch():
    import torch
    return torch


# ---- the kernel ---------------------------------------------------------------------------------------------------------
def _run(pkg, ctx, x, p, seed, stream, row0=0, in_place=False, offset=0):
    """mggcn_dropout_f32 on a copy of x whose first element sits ``offset`` elements into a 256-byte aligned allocation
    (offset = 1: no 16-byte alignment, the element path at any m); returns (out, the input buffer afterwards)"""
    torch = _torch()
    n, m = x.shape
    threshold, scale = pkg.ops.dropout_params(p)
    src = torch.zeros(offset + n * m, dtype=torch.float32, device="cuda")
    src[offset:] = torch.from_numpy(x.reshape(-1)).cuda()
    dst = src if in_place else torch.full((offset + n * m,), 123.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.lib.mggcn_dropout_f32(ctx.stream(0), src[offset:].data_ptr(), dst[offset:].data_ptr(), n * m, m, row0, threshold,
                              scale, seed, stream)
    ctx.sync()
    return dst[offset:].cpu().numpy().reshape(n, m), src[offset:].cpu().numpy().reshape(n, m)


def _same_bits(got, want, what):
    """bit for bit; where the expected value is a NaN (a kept NaN times scale) a NaN, its payload not compared"""
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), what
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)) & ~nan)
    assert bad.size == 0, (what, bad[:8], got.reshape(-1)[bad[:8]], want.reshape(-1)[bad[:8]], bad.size)


def _input(n, m, p, seed, stream, row0=0):
    """random values with NaN, +-inf and -0.0 planted at positions this call's mask drops and at positions it keeps"""
    x = np.random.default_rng(1000 * m + n).standard_normal((n, m), dtype=np.float32)
    keep = dropout_ref.mask(n, m, row0, p, seed, stream).reshape(-1)
    flat = x.reshape(-1)
    for idx in (np.flatnonzero(~keep), np.flatnonzero(keep)):
        k = min(len(idx), SPECIALS.size)
        flat[idx[:k]] = SPECIALS[:k]
    return x, keep.reshape(n, m)


@pytest.mark.parametrize("p", [0.0, 0.5, 0.999])
@pytest.mark.parametrize("m", [1, 3, 4, 41, 128, 130])
def test_kernel_matches_numpy_bit_for_bit(pkg, ctx, m, p):
    n, seed, stream = 37, 0x1234567890ABCDEF, 3 * m + 1
    x, keep = _input(n, m, p, seed, stream)
    want = dropout_ref.apply(x, 0, p, seed, stream)
    if 0.0 < p and n * m >= 64:
        assert (~keep).any() and np.isnan(x[~keep]).any()                # a dropped NaN ...
        assert (want[~keep].view(np.uint32) == 0).all()                   # ... becomes +0.0, like every dropped element
    out, src_after = _run(pkg, ctx, x, p, seed, stream)
    _same_bits(out, want, ("out of place", m, p))
    _same_bits(src_after, x, ("the input of an out-of-place call is untouched", m, p))
    assert (out[~keep].view(np.uint32) == 0).all()                        # +0.0 exactly, whatever was there
    inp, _ = _run(pkg, ctx, x, p, seed, stream, in_place=True)
    _same_bits(inp, want, ("in place", m, p))
    off, _ = _run(pkg, ctx, x, p, seed, stream, offset=1)                 # m = 4, 128: the element path this time
    _same_bits(off, want, ("pointer offset by one element", m, p))
    _same_bits(off, out, ("element path == float4 path", m, p))
    off_in, _ = _run(pkg, ctx, x, p, seed, stream, in_place=True, offset=1)
    _same_bits(off_in, want, ("offset, in place", m, p))
    if p == 0.0:                                                          # a bitwise copy (a NaN stays a NaN)
        assert keep.all()
        _same_bits(out, x, ("p = 0 copies", m))


def test_ops_dropout_is_that_call(pkg, ctx):
    x, _ = _input(37, 41, 0.25, 5, 6, row0=11)
    X, out = pkg.dn_matrix.from_numpy(x), pkg.dn_matrix(37, 41)
    pkg.ops.dropout(ctx, X, out, 0.25, 5, 6, row0=11)
    ctx.sync()
    _same_bits(out.numpy(), dropout_ref.apply(x, 11, 0.25, 5, 6), "ops.dropout")
    pkg.ops.dropout(ctx, X, X, 0.25, 5, 6, row0=11)
    ctx.sync()
    _same_bits(X.numpy(), out.numpy(), "ops.dropout in place")


@pytest.mark.parametrize("row0", [2 ** 32 + 5, 2 ** 32 - 3])
def test_rows_past_2_32(pkg, ctx, row0):
    """the high counter word, and the carry into it inside one call"""
    x = np.random.default_rng(7).standard_normal((16, 8), dtype=np.float32)
    want = dropout_ref.apply(x, row0, 0.5, 99, 4)
    first = max(2 ** 32 - row0, 0)                                        # the rows whose index needs the high word
    assert 0 <= first < 16
    assert not np.array_equal(want[first:], dropout_ref.apply(x[first:], row0 + first - 2 ** 32, 0.5, 99, 4))   # it matters
    for offset in (0, 1):
        out, _ = _run(pkg, ctx, x, 0.5, 99, 4, row0=row0, offset=offset)
        _same_bits(out, want, (row0, offset))


@pytest.mark.parametrize("m,n,offset", [(128, 2 * 16384 + 37, 0), (41, 2 * 12788 + 5, 0), (128, 2 * 4096 + 37, 1)])
def test_beyond_one_grid_pass(pkg, ctx, m, n, offset):
    """two full passes of the capped grid and a ragged third (float4 path; element path at m = 41 and at m = 128 behind a
    misaligned pointer): every element against numpy, and bitwise equal to the same call in chunks below one pass"""
    per_unit = 4 if (m % 4 == 0 and offset == 0) else 1                   # elements per thread and pass
    assert 2 * GRID_THREADS < n * m // per_unit < 3 * GRID_THREADS
    p, seed, stream, row0 = 0.5, 31, 9, 1000
    x = np.random.default_rng(m).standard_normal((n, m), dtype=np.float32)
    want = dropout_ref.apply(x, row0, p, seed, stream)
    out, _ = _run(pkg, ctx, x, p, seed, stream, row0=row0, offset=offset)
    _same_bits(out, want, ("one call", m, n))
    step = 10_000 if offset == 0 else 4000                                 # rows per chunk: below one pass on either path
    assert step * m // per_unit < GRID_THREADS
    parts = [_run(pkg, ctx, x[a:a + step], p, seed, stream, row0=row0 + a, offset=offset)[0] for a in range(0, n, step)]
    _same_bits(np.concatenate(parts), out, ("chunks with row0 advanced", m, n))


@pytest.mark.parametrize("m", [41, 128])
def test_shard_equals_slice(pkg, ctx, m):
    n, p, seed, stream = 101, 0.3, 2 ** 63 + 1, 2 ** 32 - 1
    x = np.random.default_rng(m + 1).standard_normal((n, m), dtype=np.float32)
    whole, _ = _run(pkg, ctx, x, p, seed, stream)
    _same_bits(whole, dropout_ref.apply(x, 0, p, seed, stream), ("whole", m))
    cuts = [0, 13, 14, 60, 101]
    for a, b in zip(cuts[:-1], cuts[1:]):
        shard, _ = _run(pkg, ctx, x[a:b], p, seed, stream, row0=a)
        _same_bits(shard, whole[a:b], ("rows", a, b, m))


def test_streams_and_seeds_give_different_masks(pkg, ctx):
    x = np.ones((64, 128), dtype=np.float32)
    seed, stream = 12345, 7
    masks = [_run(pkg, ctx, x, 0.5, s, t)[0] != 0 for s, t in ((seed, stream), (seed, stream + 1), (seed + 1, stream))]
    for i in range(3):
        assert abs(masks[i].mean() - 0.5) < 0.05
        for j in range(i + 1, 3):
            assert (masks[i] != masks[j]).mean() > 0.25, (i, j)


# ---- the model ----------------------------------------------------------------------------------------------------------
def _sync_oracle_state(G, O):
    """identical inputs for the next epoch (test_gpu_gcn.py): the oracle takes over the device's weights and Adam moments"""
    for layer, ol in zip(G.layers(), O.layers):
        for lin, olin in zip(layer.linears(), ol.linears()):
            olin.W, olin.b = lin.W.numpy().copy(), lin.b.numpy().copy()
            if lin.mW is not None:
                olin.mW, olin.vW = lin.mW.numpy().copy(), lin.vW.numpy().copy()
                olin.mb, olin.vb = lin.mb.numpy().copy(), lin.vb.numpy().copy()
                olin.step = lin.step


def _model_case(pkg, oracle, ctx, fused, residual, agg, seed):
    """three epochs of gcn(dropout=0.5) against the wrapped oracle from identical state every epoch.  Next to every figure
    the distance of the fp32 oracle to its exact-accumulation twin (both with the same masks) is kept: an assertion that
    fails reports it, as the full-size tests do."""
    n, sizes, p = 1536, [20, 16, 16, 5], 0.5
    ip, ix, dv = _graph(pkg, n, n * 20, 900, seed=41)
    rng = np.random.default_rng(3)
    X = rng.standard_normal((n, sizes[0]), dtype=np.float32)
    Y = rng.integers(0, sizes[-1], size=(n, 1)).astype(np.int32)
    G = pkg.gcn(pkg.csr_matrix(ip, ix, dv, n), sizes, residual_layer=residual, fused=fused, agg_dtype=agg, dropout=p)
    G.set_dropout(p, seed=seed)
    assert G.dropout_epoch == 0
    oracles = []
    for f64acc in ((True,) if agg == "bf16" else (False, True)):
        O = (_bf16_oracle(oracle, ip, ix, dv, n, sizes, residual) if agg == "bf16"          # the dropout wrapper on top
             else oracle.Gcn(oracle.Csr(ip, ix, dv, n), sizes, f64acc=f64acc, residual_layer=residual))
        dropout_ref.oracle_dropout(O, p, seed=seed)
        oracles.append(O)
    O, twin = oracles[0], oracles[-1]
    grad_bar = (lambda li, what: GRAD_BAR.get(li, GRAD_BAR_REST) if what == "G_W" else GRAD_BAR_REST) if agg == "bf16" \
        else (lambda li, what: TOL)
    solid_bar = (lambda li: W_SOLID_BAR.get(li, TOL)) if agg == "bf16" else (lambda li: TOL)
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    lr = ADAM[0]
    for epoch in range(3):
        for o in oracles:
            _sync_oracle_state(G, o)
        loss, acc = G.train_forward(ctx, Xd, Yd)
        assert G.dropout_epoch == epoch + 1
        G.backward(ctx)
        ctx.sync()
        grads = [[(lin.G_W.numpy().copy(), lin.G_b.numpy().copy()) for lin in l.linears()] for l in G.layers()]
        G.adam_update(ctx, *ADAM)
        ctx.sync()
        runs = []
        for o in oracles:
            ol, oa = o.train_forward(X, Y)
            o.backward()
            og = [[(lin.G_W.copy(), lin.G_b.copy()) for lin in l.linears()] for l in o.layers]
            o.adam_update()
            runs.append((ol, oa, og))
        (ol, oa, og), (tl, _, tg) = runs[0], runs[-1]
        print(f"[dropout] fused={fused} residual={residual} agg={agg} epoch {epoch}: loss {loss!r} oracle {ol!r} twin {tl!r}")
        assert abs(loss - ol) <= TOL * abs(ol), (epoch, loss, ol, "oracle fp32 vs f64acc:", abs(ol - tl) / abs(tl))
        assert abs(acc - oa) <= 3.0 / n, (epoch, acc, oa)
        for li, (layer, olayer) in enumerate(zip(G.layers(), O.layers)):
            for k, (lin, olin) in enumerate(zip(layer.linears(), olayer.linears())):
                for what, got, want, ref in (("G_W", grads[li][k][0], og[li][k][0], tg[li][k][0]),
                                             ("G_b", grads[li][k][1], og[li][k][1], tg[li][k][1])):
                    err = relerr(got, want)
                    print(f"[dropout]   layer {li} linear {k} {what}: {err:.3e} (oracle fp32 vs f64acc {relerr(want, ref):.3e})")
                    assert err <= grad_bar(li, what), (epoch, li, k, what, err, "oracle fp32 vs f64acc:", relerr(want, ref))
                if residual:
                    continue                                          # test_gpu_gcn's residual case stops at the gradients
                # test_gpu_gcn.py holds W to these bars, test_gpu_agg_bf16.py W and b
                for P, Po, g in ((lin.W.numpy(), olin.W, og[li][k][0]), (lin.b.numpy(), olin.b, og[li][k][1]))[:2 if agg == "bf16" else 1]:
                    assert np.abs(P - Po).max() <= 2.05 * lr, (epoch, li)                 # never more than a sign flip
                    solid = np.abs(g) > 1e-2 * np.abs(g).max()                           # well-conditioned entries
                    assert np.abs(P - Po)[solid].max() <= solid_bar(li) * np.abs(Po).max(), (epoch, li, P.shape)
    return G


@pytest.mark.parametrize("fused,residual", [(True, False), (False, False), (True, True)])
def test_model_matches_the_wrapped_oracle(pkg, oracle, ctx, fused, residual):
    G = _model_case(pkg, oracle, ctx, fused, residual, "f32", seed=2024)
    import io
    out = io.StringIO()
    ctx.dump_timers(out, "")
    names = {line.split(":")[0] for line in out.getvalue().splitlines()}
    for li in (1, 2):
        assert f"{li}_0_dropout" in names and f"{li}_1_dropout" in names, sorted(names)
    assert "0_0_dropout" not in names and "0_1_dropout" not in names        # the features are never dropped
    assert [l.dropout is None for l in G.layers()] == [True, False, False]


def test_bf16_model_matches_the_wrapped_bf16_oracle(pkg, oracle, ctx):
    _model_case(pkg, oracle, ctx, True, False, "bf16", seed=77)


def test_dropout_is_not_a_no_op_in_training(pkg, oracle, ctx):
    """the wrapped oracle and the plain one differ by far more than the parity bar: the comparison above can tell"""
    n, sizes = 1536, [20, 16, 16, 5]
    ip, ix, dv = _graph(pkg, n, n * 20, 900, seed=41)
    rng = np.random.default_rng(3)
    X = rng.standard_normal((n, sizes[0]), dtype=np.float32)
    Y = rng.integers(0, sizes[-1], size=(n, 1)).astype(np.int32)
    plain = oracle.Gcn(oracle.Csr(ip, ix, dv, n), sizes)
    dropped = oracle.Gcn(oracle.Csr(ip, ix, dv, n), sizes)
    dropout_ref.oracle_dropout(dropped, 0.5, seed=2024)
    for O in (plain, dropped):
        O.train_forward(X, Y)
        O.backward()
    for a, b in zip(plain.layers, dropped.layers):
        assert relerr(b.lin.G_W, a.lin.G_W) > 100 * TOL, relerr(b.lin.G_W, a.lin.G_W)


def test_evaluation_never_drops_and_epochs_replay(pkg, ctx):
    n, sizes = 1536, [20, 16, 16, 5]
    ip, ix, dv = _graph(pkg, n, n * 20, 900, seed=41)
    rng = np.random.default_rng(5)
    Xd = pkg.dn_matrix.from_numpy(rng.standard_normal((n, sizes[0]), dtype=np.float32))
    Yd = pkg.dn_matrix.from_numpy(rng.integers(0, sizes[-1], size=(n, 1)).astype(np.int32))
    Sd = pkg.dn_matrix.from_numpy(rng.integers(0, 3, size=(n, 1)).astype(np.int32))
    G = pkg.gcn(pkg.csr_matrix(ip, ix, dv.copy(), n), sizes)                  # the same seed-99 weights in both
    G0 = pkg.gcn(pkg.csr_matrix(ip, ix, dv.copy(), n), sizes)
    G.set_dropout(0.5, seed=11)
    def plain(M):
        H = M(ctx, Xd)
        ctx.sync()
        return H.numpy().copy()
    out, out0 = plain(G), plain(G0)
    assert np.array_equal(out.view(np.uint32), out0.view(np.uint32))
    assert G.evaluate(ctx, Xd, Yd, Sd) == G0.evaluate(ctx, Xd, Yd, Sd)
    assert G.dropout_epoch == 0                                                 # none of these was a training forward
    clean = G0.train_forward(ctx, Xd, Yd)[0]
    first = G.train_forward(ctx, Xd, Yd)[0]
    second = G.train_forward(ctx, Xd, Yd)[0]
    assert G.dropout_epoch == 2 and first != second and first != clean and second != clean
    G.set_dropout(0.5, seed=11, epoch=0)
    assert G.train_forward(ctx, Xd, Yd)[0] == first                             # the same masks, the same sums
    G.set_dropout(0.5, seed=11, epoch=1)
    assert G.train_forward(ctx, Xd, Yd)[0] == second
    G.set_dropout(0.5, seed=12, epoch=0)
    assert G.train_forward(ctx, Xd, Yd)[0] != first
    out = plain(G)                                                              # and a plain call after training is clean
    assert np.array_equal(out.view(np.uint32), out0.view(np.uint32))
    G.set_dropout(0.0)                                                          # p = 0: the model without dropout
    assert G.train_forward(ctx, Xd, Yd)[0] == clean and G.dropout_epoch == 0


# ---- the CLI ------------------------------------------------------------------------------------------------------------
def test_cli_dropout_matches_the_python_model(pkg, ctx, tmp_path):
    """MGGCN_DROPOUT=0.5 MGGCN_DROPOUT_SEED=7 mg_gcn -P 1: CLI epoch e is dropout epoch e -- its losses are the Python
    model's from the weights the CLI started the epoch with, and its epoch-1 weights are those of the Python model's step
    with the same p and seed, not those of another seed or of no dropout"""
    n, F, C = 2000, 16, 5
    ip, ix, dv = pkg.datasets.synth_powerlaw_csr(n, n * 12, 300, seed=11)
    rng = np.random.default_rng(12)
    X = rng.standard_normal((n, F), dtype=np.float32)
    Y = rng.integers(0, C, size=(n, 1)).astype(np.int32)
    Y[0, 0] = C - 1
    d = tmp_path / "permuted" / "toy"
    pkg.datasets.write_dataset(str(d), ip, ix, dv, X, Y)
    exe = os.path.join(BIN, "mg_gcn")
    env = dict(os.environ, MGGCN_DROPOUT="0.5", MGGCN_DROPOUT_SEED="7", MGGCN_DUMP_WEIGHTS=str(tmp_path / "w"))
    r = subprocess.run([exe, "-P", "1", "-E", "2", "train", str(d), "2", "16", "16"], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = [tuple(float(x) for x in ln.split()) for ln in r.stderr.strip().splitlines()[3:5]]
    assert [int(g[0]) for g in got] == [0, 1]
    sizes = [F, 16, 16, C]

    def load(M, e):
        for li, layer in enumerate(M.layers()):
            layer.W().init(pkg.datasets.read_dense(str(tmp_path / "w" / f"e{e}_W{li}.bin"), "<f4"))
            layer.b().init(pkg.datasets.read_dense(str(tmp_path / "w" / f"e{e}_b{li}.bin"), "<f4"))
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    G = pkg.gcn(pkg.csr_matrix(ip, ix, dv, n), sizes)
    for e in range(2):
        load(G, e)
        G.set_dropout(0.5, seed=7, epoch=e)
        loss, acc = G.train_forward(ctx, Xd, Yd)
        assert abs(got[e][1] - loss) <= TOL * abs(loss), (e, got[e], loss)
        assert abs(got[e][2] - acc) <= 3.0 / n, (e, got[e], acc)
    want1 = [pkg.datasets.read_dense(str(tmp_path / "w" / f"e1_W{li}.bin"), "<f4") for li in range(len(sizes) - 1)]
    moved = {}
    for name, p, seed in (("same", 0.5, 7), ("other seed", 0.5, 8), ("none", 0.0, 0)):
        M = pkg.gcn(pkg.csr_matrix(ip, ix, dv, n), sizes)
        load(M, 0)
        M.set_dropout(p, seed=seed)
        M.train_step(ctx, Xd, Yd, *ADAM)
        moved[name] = sum(int((np.abs(layer.W().numpy().reshape(w.shape) - w) > 1e-3).sum())
                          for layer, w in zip(M.layers(), want1))
    assert moved["same"] < moved["other seed"] and moved["same"] < moved["none"], moved
    # refused before any device work: one line on stderr, a non-zero exit
    for args, env_add, msg in (([], {"MGGCN_DROPOUT": "1.5"}, "MGGCN_DROPOUT must be in [0, 1)"),
                               ([], {"MGGCN_DROPOUT": "x"}, "MGGCN_DROPOUT must be a number"),
                               (["-R", "1"], {"MGGCN_DROPOUT": "0.5"}, "MGGCN_DROPOUT is single-GPU only")):
        r = subprocess.run([exe, "-P", "1"] + args + ["-E", "1", "train", str(d), "2", "16", "16"], cwd=str(tmp_path),
                           env=dict(os.environ, **env_add), capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and msg in r.stderr, (args, env_add, r.stderr)
        assert len(r.stderr.strip().splitlines()) == 1, r.stderr
