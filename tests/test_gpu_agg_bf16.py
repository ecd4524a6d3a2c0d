"""bf16 aggregation on the device: the conversion against torch's cast, the bf16 SpMM against the fp32 SpMM on the
widened operand (bit for bit, every form the fp32 entry dispatches to), the full Reddit-shape calls, the model against
the bf16-wrapped exact-accumulation oracle, and the CLI against the Python model."""
import os
import subprocess

import numpy as np
import pytest

from bf16_ref import GRAD_BAR, GRAD_BAR_REST, W_SOLID_BAR, bf16_bits, bf16_oracle as _bf16_oracle, round_bf16, widen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mg-gcn_amd", "bin")
TOL = 1e-4
WIDTHS = [1, 3, 8, 16, 41, 48, 64, 96, 128, 130, 256, 608]


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


def _torch():
    import torch
    return torch


# ---- conversion --------------------------------------------------------------------------------------------------
def _special_matrix(n, m, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, m)) * np.exp(rng.uniform(-40, 40, (n, m)))).astype(np.float32)
    bits = np.array([0x3F808000, 0x3F818000, 0x00008000, 0x00018000, 0x80028000, 0x7F7F8000, 0x7F7FFFFF, 0xFF7FFFFF,
                     0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7F800001, 0xFFFFFFFF, 0x7FC00000, 0xFFC00001,
                     0x3F807FFF, 0x3F808001, 0x00000000, 0x80000000], dtype=np.uint32).view(np.float32)
    flat = x.reshape(-1)
    flat[:bits.size] = bits
    flat[-bits.size:] = bits[::-1]
    return x


@pytest.mark.parametrize("m,pad_s,pad_d", [(128, 0, 0), (41, 0, 0), (41, 7, 23), (96, 4, 8), (3, 1, 0), (608, 0, 16)])
def test_conversion_is_bit_exact(pkg, ctx, m, pad_s, pad_d):
    torch = _torch()
    n = 1031
    x = _special_matrix(n, m, seed=m + pad_s)
    src = torch.zeros((n, m + pad_s), dtype=torch.float32, device="cuda")
    src[:, :m] = torch.from_numpy(x).cuda()
    dst = torch.full((n, m + pad_d), 0x1234, dtype=torch.int16, device="cuda")
    pkg.ops.convert_bf16(ctx, src[:, :m], dst[:, :m])
    ctx.sync()
    got = dst.cpu().numpy().view(np.uint16)
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(x)
    assert nan.any()
    np.testing.assert_array_equal(got[:, :m][~nan], want[~nan])
    assert np.isnan(widen(got[:, :m][nan])).all()                       # NaN stays NaN (payload not compared)
    np.testing.assert_array_equal(got[:, :m][~nan], bf16_bits(x)[~nan])
    assert (got[:, m:] == 0x1234).all()                                   # padding columns untouched


# ---- SpMM: bf16 entry == fp32 entry on the widened operand -----------------------------------------------------------
SWEEP_KNOBS = {                       # the force_sweep fixture of test_gpu_kernels.py, restated
    "MGGCN_SPMM_SWEEP_MIN_NNZ": "1", "MGGCN_SPMM_PANEL_ROWS": "64", "MGGCN_SPMM_PANEL_ROWS_NARROW": "96",
    "MGGCN_SPMM_SLICE_ROWS": "400", "MGGCN_SPMM_SWEEP_MIN_RUN_X10": "0",
}
PLANS = {
    # name: (environment, d_hint, expected plan form)
    "null": (None, 0, None),
    "rowsplit": ({"MGGCN_SPMM_ALGO": "rowsplit"}, 0, "form=rowsplit"),
    "sweep-as-given": (dict(SWEEP_KNOBS, MGGCN_SPMM_PERMUTE_COLUMNS="0"), 0, "form=sweep "),
    "sweep-permuted": (dict(SWEEP_KNOBS, MGGCN_SPMM_PERMUTE_COLUMNS="1"), 0, "permuted=1"),
    "sweep-general-pairs": (dict(SWEEP_KNOBS, MGGCN_SPMM_PERMUTE_COLUMNS="0", MGGCN_SPMM_FAST_PAIRS="0"), 0, "form=sweep "),
    "narrow-41": (dict(SWEEP_KNOBS, MGGCN_SPMM_PERMUTE_COLUMNS="0"), 41, "form=sweep-narrow"),
    "narrow-16": (dict(SWEEP_KNOBS, MGGCN_SPMM_PERMUTE_COLUMNS="0"), 16, "form=sweep-narrow"),
    "narrow-41-permuted": (dict(SWEEP_KNOBS, MGGCN_SPMM_PERMUTE_COLUMNS="1"), 41, "permuted=1"),
}


def _plan(pkg, ctx, A, name, monkeypatch):
    env, hint, form = PLANS[name]
    if env is None:
        return None
    for k in ("MGGCN_SPMM_ALGO", "MGGCN_SPMM_FAST_PAIRS", "MGGCN_SPMM_PERMUTE_COLUMNS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    plan = pkg.ops.spmm_plan_for(ctx, A, max(WIDTHS), hint)
    assert form in plan.describe(), plan.describe()
    return plan


def _spmm_f32(ctx, A, plan, Bw, C, alpha, beta, flags, slope=0.01):
    """the fp32 entry on a torch operand (row stride = leading dimension)"""
    ip, ix, dv = A.device(ctx.device)
    ctx.lib.mggcn_spmm_csr_f32(ctx.stream(0), plan.handle if plan else None, A.n(), A.m(), ip.data_ptr(), ix.data_ptr(),
                               dv.data_ptr(), Bw.data_ptr(), Bw.stride(0), C.buffer(), C.m(), C.m(), alpha, beta, flags,
                               slope)


@pytest.mark.parametrize("plan_kind", list(PLANS))
def test_spmm_bf16_equals_fp32_on_the_widened_operand(pkg, oracle, ctx, monkeypatch, plan_kind):
    torch = _torch()
    n = 1500
    ip, ix, dv = pkg.datasets.synth_powerlaw_csr(n, 60_000, 4000, seed=7)
    dv = np.random.default_rng(1).random(dv.shape[0], dtype=np.float32)
    A = pkg.csr_matrix(ip, ix, dv, n)
    plan = _plan(pkg, ctx, A, plan_kind, monkeypatch)
    Ao = oracle.Csr(ip, ix, dv, n)
    for d in WIDTHS:
        rng = np.random.default_rng(d)
        pad = 5 if d in (41, 130) else 0                          # a padded leading dimension (same one for both)
        bits = bf16_bits(rng.standard_normal((n, d), dtype=np.float32))
        B16 = torch.zeros((n, d + pad), dtype=torch.int16, device="cuda")
        B16[:, :d] = torch.from_numpy(bits.view(np.int16)).cuda()
        Bw = torch.zeros((n, d + pad), dtype=torch.float32, device="cuda")
        Bw[:, :d] = torch.from_numpy(widen(bits)).cuda()
        C0 = rng.standard_normal((n, d), dtype=np.float32)
        for beta in (0.0, 1.0):
            for flags in (0, 1):
                alpha = 0.75
                Cb, Cf, Cb2 = (pkg.dn_matrix.from_numpy(C0) for _ in range(3))
                pkg.ops.spmm_bf16(ctx, A, B16[:, :d], Cb, plan, alpha, beta, flags, 0.01)
                _spmm_f32(ctx, A, plan, Bw[:, :d], Cf, alpha, beta, flags)
                pkg.ops.spmm_bf16(ctx, A, B16[:, :d], Cb2, plan, alpha, beta, flags, 0.01)
                ctx.sync()
                got, want = Cb.numpy(), Cf.numpy()
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
                    (plan_kind, d, beta, flags, float(np.abs(got - want).max()))
                assert np.array_equal(got.view(np.uint32), Cb2.numpy().view(np.uint32)), (plan_kind, d, beta, flags)
                if beta == 0.0 and flags == 0:                      # and the product is the right one
                    ref = oracle.spmm(Ao, widen(bits), alpha=alpha, f64acc=True)
                    assert np.abs(got - ref).max() <= TOL * np.abs(ref).max(), (plan_kind, d)


def test_plan_bytes_grow_only_on_first_bf16_use(pkg, ctx, monkeypatch):
    """one plan serves both entries; a narrow / relabelled plan allocates its bf16 scratch on the first bf16 call"""
    torch = _torch()
    n = 1500
    ip, ix, dv = pkg.datasets.synth_powerlaw_csr(n, 60_000, 4000, seed=8)
    A = pkg.csr_matrix(ip, ix, dv, n)
    plan = _plan(pkg, ctx, A, "narrow-41", monkeypatch)
    before, line = plan.nbytes(), plan.describe()
    C = pkg.dn_matrix(n, 41)
    Bw = torch.randn((n, 41), device="cuda")
    _spmm_f32(ctx, A, plan, Bw, C, 1.0, 0.0, 0)
    ctx.sync()
    assert plan.nbytes() == before and plan.describe() == line
    B16 = Bw.to(torch.bfloat16)
    pkg.ops.spmm_bf16(ctx, A, B16, C, plan)
    ctx.sync()
    assert plan.nbytes() == before + n * 64 * 2           # 41 bf16 columns at a 128-byte pitch


# ---- the full Reddit shape ----------------------------------------------------------------------------------------
def test_full_reddit_shape_calls(pkg, ctx):
    """one d = 128 forward call (the pair kernel) and one d = 41 call (the narrow form) on the symmetric stand-in"""
    from conftest import reddit_standin
    torch = _torch()
    data = reddit_standin(pkg, "sym")
    n = data["n"]
    A = pkg.csr_matrix(data["ip"], data["ix"], data["dv"], n)
    for d in (128, 41):
        plan = pkg.ops.spmm_plan_for(ctx, A, 128, d)
        assert "form=sweep" in plan.describe(), plan.describe()
        g = torch.Generator(device="cuda").manual_seed(d)
        B16 = torch.randn((n, d), device="cuda", generator=g).to(torch.bfloat16)
        Bw = B16.float()
        Cb, Cf = pkg.dn_matrix(n, d), pkg.dn_matrix(n, d)
        pkg.ops.spmm_bf16(ctx, A, B16, Cb, plan, 1.0, 0.0, 1, 0.01)
        _spmm_f32(ctx, A, plan, Bw, Cf, 1.0, 0.0, 1)
        ctx.sync()
        assert torch.equal(Cb.t.view(torch.int32), Cf.t.view(torch.int32)), d


# ---- the model ----------------------------------------------------------------------------------------------------
def _relerr(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / (np.abs(want).max() + 1e-30))


def _sync_oracle_state(G, O):
    """identical inputs for the next epoch (as in test_gpu_gcn.py): weights and Adam moments of the device model"""
    for layer, ol in zip(G.layers(), O.layers):
        for lin, olin in zip(layer.linears(), [ol.lin] + ([ol.res_lin] if ol.res_lin is not None else [])):
            olin.W, olin.b = lin.W.numpy().copy(), lin.b.numpy().copy()
            if lin.mW is not None:
                olin.mW, olin.vW = lin.mW.numpy().copy(), lin.vW.numpy().copy()
                olin.mb, olin.vb = lin.mb.numpy().copy(), lin.vb.numpy().copy()
                olin.step = lin.step


@pytest.mark.parametrize("fused,residual", [(True, False), (False, False), (True, True)])
def test_bf16_model_matches_the_bf16_oracle(pkg, oracle, ctx, fused, residual):
    """three epochs (forward, backward, Adam) of gcn(agg_dtype="bf16") against oracle.Gcn(f64acc=True) with every SpMM
    wrapped as A . bf16(B): loss and accuracy at the fp32 parity tests' bars (test_gpu_gcn.py), W and b within one
    Adam sign flip, their well-conditioned entries at TOL (first layer: W_SOLID_BAR), gradients at GRAD_BAR"""
    n, sizes = 50_000, [128, 128, 128, 41]
    ip, ix, dv = pkg.datasets.synth_powerlaw_csr(n, n * 24, 2000, seed=5)
    rng = np.random.default_rng(0)
    X = rng.standard_normal((n, sizes[0]), dtype=np.float32)
    Y = rng.integers(0, sizes[-1], size=(n, 1)).astype(np.int32)
    G = pkg.gcn(pkg.csr_matrix(ip, ix, dv, n), sizes, residual_layer=residual, fused=fused, agg_dtype="bf16")
    O = _bf16_oracle(oracle, ip, ix, dv, n, sizes, residual)
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    lr = 1e-2
    for epoch in range(3):
        _sync_oracle_state(G, O)
        loss, acc = G.train_forward(ctx, Xd, Yd)
        G.backward(ctx)
        ctx.sync()
        grads = [(l.GW().numpy().copy(), l.Gb().numpy().copy()) for l in G.layers()]
        G.adam_update(ctx, lr, 0.9, 0.999, 5e-4, 1e-8)
        ctx.sync()
        ol, oa = O.train_forward(X, Y)
        O.backward()
        ograds = [(l.lin.G_W.copy(), l.lin.G_b.copy()) for l in O.layers]
        O.adam_update()
        assert abs(loss - ol) <= TOL * abs(ol), (epoch, loss, ol)
        assert abs(acc - oa) <= 3.0 / n, (epoch, acc, oa)
        for li, (layer, olayer) in enumerate(zip(G.layers(), O.layers)):
            assert _relerr(grads[li][0], ograds[li][0]) <= GRAD_BAR.get(li, GRAD_BAR_REST), (epoch, li, "G_W")
            assert _relerr(grads[li][1], ograds[li][1]) <= GRAD_BAR_REST, (epoch, li, "G_b")
            for P, Po, g in ((layer.W().numpy(), olayer.lin.W, ograds[li][0]), (layer.b().numpy(), olayer.lin.b, ograds[li][1])):
                assert np.abs(P - Po).max() <= 2.05 * lr, (epoch, li)            # never more than a sign flip
                solid = np.abs(g) > 1e-2 * np.abs(g).max()                      # well-conditioned entries
                assert np.abs(P - Po)[solid].max() <= W_SOLID_BAR.get(li, TOL) * np.abs(Po).max(), (epoch, li, P.shape)


def test_hoisting_is_fp32_only(pkg, ctx):
    ip, ix, dv = pkg.datasets.synth_uniform_csr(512, 8, seed=2)
    with pytest.raises(ValueError, match="hoist_first_aggregation"):
        pkg.gcn(pkg.csr_matrix(ip, ix, dv, 512), [16, 8, 4], agg_dtype="bf16", hoist_first_aggregation=True)
    G = pkg.gcn(pkg.csr_matrix(ip, ix, dv, 512), [16, 8, 4], agg_dtype="bf16")
    with pytest.raises(ValueError, match="hoist_first_aggregation"):
        G.set_hoist_first_aggregation(True)


# ---- the CLI ------------------------------------------------------------------------------------------------------
def test_cli_bf16_matches_the_python_model(pkg, ctx, tmp_path):
    """MGGCN_AGG_DTYPE=bf16 mg_gcn -P 1: per-epoch losses of the Python bf16 model at 1e-4 (every epoch from the
    weights the CLI started it with: free-running Adam trajectories are not comparable at 1e-4, see test_gpu_host_cpp)"""
    n, F, C = 20_000, 64, 7
    ip, ix, dv = pkg.datasets.synth_powerlaw_csr(n, n * 20, 1500, seed=11)
    rng = np.random.default_rng(12)
    X = rng.standard_normal((n, F), dtype=np.float32)
    Y = rng.integers(0, C, size=(n, 1)).astype(np.int32)
    Y[0, 0] = C - 1
    d = tmp_path / "permuted" / "synth"
    pkg.datasets.write_dataset(str(d), ip, ix, dv, X, Y)
    env = dict(os.environ, MGGCN_AGG_DTYPE="bf16", MGGCN_DUMP_WEIGHTS=str(tmp_path / "w"))
    r = subprocess.run([os.path.join(BIN, "mg_gcn"), "-P", "1", "-E", "3", "train", str(d), "3", "128", "128", "128"],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stderr.strip().splitlines()
    got = [tuple(float(x) for x in ln.split()) for ln in lines[3:6]]
    assert [int(g[0]) for g in got] == [0, 1, 2]
    sizes = [F, 128, 128, 128, C]
    G = pkg.gcn(pkg.csr_matrix(ip, ix, dv, n), sizes, agg_dtype="bf16")
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    f32 = []
    for e in range(3):
        for li, layer in enumerate(G.layers()):
            layer.W().init(pkg.datasets.read_dense(str(tmp_path / "w" / f"e{e}_W{li}.bin"), "<f4"))
            layer.b().init(pkg.datasets.read_dense(str(tmp_path / "w" / f"e{e}_b{li}.bin"), "<f4"))
        loss, acc = G.train_forward(ctx, Xd, Yd)
        assert abs(got[e][1] - loss) <= TOL * abs(loss), (e, got[e], loss)
        assert abs(got[e][2] - acc) <= 3.0 / n, (e, got[e], acc)
        f32.append(loss)
    # and it is the bf16 model, not the fp32 one.  The losses cannot tell (the two differ by ~1e-5); the first Adam step
    # can: it moves every weight by lr * sign(g), and the first layer's small gradients differ in sign between the two
    # aggregations (see GRAD_BAR) -- the CLI's epoch-1 weights are those of the bf16 model's step.
    want1 = [pkg.datasets.read_dense(str(tmp_path / "w" / f"e1_W{li}.bin"), "<f4") for li in range(len(sizes) - 1)]
    moved = {}
    for agg in ("bf16", "f32"):
        M = pkg.gcn(pkg.csr_matrix(ip, ix, dv, n), sizes, agg_dtype=agg)
        for li, layer in enumerate(M.layers()):
            layer.W().init(pkg.datasets.read_dense(str(tmp_path / "w" / f"e0_W{li}.bin"), "<f4"))
            layer.b().init(pkg.datasets.read_dense(str(tmp_path / "w" / f"e0_b{li}.bin"), "<f4"))
        M.train_step(ctx, Xd, Yd, 1e-2, 0.9, 0.999, 5e-4, 1e-8)
        moved[agg] = sum(int((np.abs(layer.W().numpy().reshape(w.shape) - w) > 1e-3).sum())
                         for layer, w in zip(M.layers(), want1))
    assert moved["bf16"] < moved["f32"], moved
