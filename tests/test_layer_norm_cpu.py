"""Layer normalisation (mggcn_layer_norm_forward_f32 / _backward_f32), the parts that need no GPU: the fp64 restatement
the GPU tests compare against agrees with torch's layer_norm and autograd, the fp32 twin stays within the GPU tests' bars
of it, the C ABI and its binding, and the errors raised before any device work."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import layernorm_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(n, m, seed, shift=0.0):
    rng = np.random.default_rng(seed)
    x = (shift + rng.standard_normal((n, m))).astype(np.float32)
    G = rng.standard_normal((n, m)).astype(np.float32)
    gamma, beta = ref.params(m, seed + 1)
    return x, G, gamma, beta


@pytest.mark.parametrize("leaky", [False, True])
@pytest.mark.parametrize("m", [1, 3, 4, 41, 128, 130])
def test_restatement_agrees_with_torch_in_float64(m, leaky):
    """forward and all three gradients against torch.nn.functional.layer_norm (+ leaky_relu) and autograd, to 1e-12"""
    import torch
    x, G, gamma, beta = _case(37, m, 100 + m)
    tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tg = torch.tensor(gamma.reshape(-1), dtype=torch.float64, requires_grad=True)
    tb = torch.tensor(beta.reshape(-1), dtype=torch.float64, requires_grad=True)
    z = torch.nn.functional.layer_norm(tx, (m,), tg, tb, eps=ref.EPS)
    y = torch.nn.functional.leaky_relu(z, ref.SLOPE) if leaky else z
    y.backward(torch.tensor(G, dtype=torch.float64))
    got_y, xhat, rstd = ref.forward64(x, gamma, beta, leaky, exact=True)
    G_in, G_gamma, G_beta = ref.backward64(G, got_y, x, gamma, leaky, exact=True)       # sign source: the activated output
    mean = x.astype(np.float64).mean(axis=1, keepdims=True)
    var = x.astype(np.float64).var(axis=1, keepdims=True)
    for what, got, want in (("y", got_y, y.detach().numpy()), ("G_in", G_in, tx.grad.numpy()),
                            ("G_gamma", G_gamma.reshape(-1), tg.grad.numpy()), ("G_beta", G_beta.reshape(-1), tb.grad.numpy()),
                            ("xhat", xhat, (x - mean) / np.sqrt(var + ref.EPS)), ("rstd", rstd, 1 / np.sqrt(var + ref.EPS).reshape(-1))):
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (what, m, leaky)


@pytest.mark.parametrize("shift,bar", [(0.0, 1e-5), (100.0, 1e-4)])
@pytest.mark.parametrize("m", [16, 41, 128, 1024])
def test_twin_is_within_a_third_of_the_bars(m, shift, bar):
    """the fp32 twin (the kernel's formulas) against the restatement, on the two inputs of the GPU tests"""
    x, G, gamma, beta = _case(37, m, 200 + m, shift)
    y, xhat, rstd = ref.forward32(x, gamma, beta, True)
    wy, wxhat, wrstd = ref.forward64(x, gamma, beta, True)
    got = (y, xhat, rstd) + ref.backward32(G, wy, xhat, rstd, gamma, True)       # one sign source for both
    want = (wy, wxhat, wrstd) + ref.backward64(G, wy, x, gamma, True)
    for what, g, w in zip(("y", "xhat", "rstd", "G_in", "G_gamma", "G_beta"), got, want):
        assert ref.rowdist(g, w) <= bar / 3, (what, m, shift, ref.rowdist(g, w))


def test_one_pass_variance_would_fail_the_shifted_case():
    """E[x^2] - mean^2 in fp32 on rows 100 + N(0, 1) is off by more than the bar: the shifted case can tell"""
    x, _, gamma, beta = _case(37, 128, 7, 100.0)
    mean = x.mean(axis=1, keepdims=True, dtype=np.float32)
    var = (x * x).mean(axis=1, keepdims=True, dtype=np.float32) - mean * mean
    xhat = (x - mean) / np.sqrt(var + np.float32(ref.EPS))
    assert ref.rowdist(xhat, ref.forward64(x, gamma, beta)[1]) > 1e-4


def _decl(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mggcn.h")).read(), flags=re.S)
    decl = re.search(r"void\s+" + name + r"\s*\(([^;]*)\);", text)
    assert decl, name
    return [" ".join(a.split()) for a in decl.group(1).split(",")]


def test_header_declares_the_entry_points():
    fwd = _decl("mggcn_layer_norm_forward_f32")
    assert fwd == ["mggcn_stream_t stream", "const float *x", "float *y", "float *xhat", "float *rstd", "const float *gamma",
                   "const float *beta", "size_t n_rows", "size_t m", "float eps", "uint32_t flags"]
    bwd = _decl("mggcn_layer_norm_backward_f32")
    assert bwd == ["mggcn_stream_t stream", "const float *G", "const float *act", "const float *xhat", "const float *rstd",
                   "const float *gamma", "float *G_in", "float *G_gamma", "float *G_beta", "size_t n_rows", "size_t m",
                   "uint32_t flags"]
    text = open(os.path.join(ROOT, "include", "mggcn.h")).read()
    assert re.search(r"#define\s+MGGCN_LN_LEAKY_RELU\s+1u", text) and re.search(r"#define\s+MGGCN_LN_MAX_WIDTH\s+1024u", text)
    assert re.search(r"MGGCN_ABI_VERSION\s+1\b", text)                       # an addition


def test_library_exports_and_binding_types_them(pkg):
    lib = ctypes.CDLL(pkg._lib.LIB_PATH)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    for name, want in (("mggcn_layer_norm_forward_f32", [vp] * 7 + [sz, sz, ctypes.c_float, ctypes.c_uint32]),
                       ("mggcn_layer_norm_backward_f32", [vp] * 9 + [sz, sz, ctypes.c_uint32])):
        assert hasattr(lib, name)
        restype, argtypes = pkg._lib.PROTOTYPES[name]
        assert restype is None and argtypes == want, name
    assert pkg.ops.LAYER_NORM_EPS == ref.EPS == 1e-5 and pkg.ops.LAYER_NORM_MAX_WIDTH == 1024
    assert pkg.ops.LAYER_NORM_LEAKY_RELU == 1


class _shape:
    """a shape-only stand-in for a dn_matrix: touching a buffer is an error"""

    def __init__(self, n, m): self._n, self._m = n, m
    def n(self): return self._n
    def m(self): return self._m
    def size(self): return self._n * self._m
    def shape(self): return (self._n, self._m)
    def buffer(self): raise AssertionError("the library was about to be called")


@pytest.mark.parametrize("m", [0, 1025, 4096])
def test_width_errors_raise_before_the_library(pkg, m):
    n = 8
    M, r, g = _shape(n, m), _shape(n, 1), _shape(1, m)
    with pytest.raises(ValueError, match="1024"):
        pkg.ops.layer_norm(None, M, M, M, r, g, g)
    with pytest.raises(ValueError, match="1024"):
        pkg.ops.layer_norm_backward(None, M, M, M, r, g, M, g, g, 1)


def test_shape_errors_raise_before_the_library(pkg):
    n, m = 8, 16
    M, r, g = _shape(n, m), _shape(n, 1), _shape(1, m)
    bad = [dict(Y=_shape(n, m + 1)), dict(xhat=_shape(n + 1, m)), dict(rstd=_shape(n + 1, 1)), dict(gamma=_shape(1, m + 1)),
           dict(beta=_shape(2, m))]
    for kw in bad:
        args = dict(X=M, Y=M, xhat=M, rstd=r, gamma=g, beta=g)
        args.update(kw)
        with pytest.raises(ValueError):
            pkg.ops.layer_norm(None, **args)
    bad = [dict(G_in=_shape(n, m + 1)), dict(xhat=_shape(n + 1, m)), dict(rstd=_shape(n - 1, 1)), dict(G_gamma=_shape(1, m - 1)),
           dict(G_beta=_shape(2, m)), dict(act=None, flags=1), dict(act=_shape(n, m + 4), flags=1)]
    for kw in bad:
        args = dict(G=M, act=M, xhat=M, rstd=r, gamma=g, G_in=M, G_gamma=g, G_beta=g)
        args.update(kw)
        with pytest.raises(ValueError):
            pkg.ops.layer_norm_backward(None, **args)


@pytest.mark.parametrize("norm", ["batch", "Layer", True, 1, ""])
def test_bad_norms_raise_before_any_device_work(pkg, norm):
    """no context, buffer or graph is touched: None stands in for all of them"""
    import sys
    mod = sys.modules[pkg.gcn.__module__]
    with pytest.raises(ValueError, match="norm"):
        mod.check_norm(norm)
    with pytest.raises(ValueError, match="norm"):
        pkg.gcn(None, [8, 8, 3], norm=norm)
    with pytest.raises(ValueError, match="norm"):
        pkg.dist.dist_gcn(None, None, None, [8, 8, 3], norm=norm)
    assert mod.check_norm(None) is None and mod.check_norm("layer") == "layer"


def test_cli_refuses_bad_layer_norm_options(tmp_path):
    exe = os.path.join(ROOT, "mg-gcn_amd", "bin", "mg_gcn")

    def run(args, **env):
        return subprocess.run([exe] + args + ["train", str(tmp_path / "nope"), "1", "8"], cwd=str(tmp_path),
                              env=dict(os.environ, **env), capture_output=True, text=True, timeout=60)
    for value in ("2", "yes", "layer", "", "1 "):
        r = run([], MGGCN_LAYER_NORM=value)
        assert r.returncode != 0 and "MGGCN_LAYER_NORM must be 0 or 1" in r.stderr, (value, r.stderr)
        assert len(r.stderr.strip().splitlines()) == 1, r.stderr              # before any device work or output
    for args in (["-P", "2"], ["-P", "1", "-R", "1"]):
        r = run(args, MGGCN_LAYER_NORM="1")
        assert r.returncode != 0 and "MGGCN_LAYER_NORM is single-GPU only" in r.stderr, (args, r.stderr)
        assert len(r.stderr.strip().splitlines()) == 1, r.stderr
    r = run(["-P", "2"], MGGCN_LAYER_NORM="0")                                # off is not refused anywhere
    assert "MGGCN_LAYER_NORM" not in r.stderr, r.stderr


def test_the_model_case_is_well_conditioned(pkg, oracle):
    """the GPU model tests' case on the host: over three epochs the wrapped fp32 oracle and its exact-accumulation twin
    differ by <= 1.5e-6 in every gradient and the smallest row sigma is 0.308 (0.31), so TOL = 1e-4 has room; and the wrapped
    oracle differs from the plain one by >= 0.19 in every G_W, so the comparison can tell"""
    n, sizes = 1536, [20, 16, 16, 5]
    ip, ix, dv = pkg.datasets.synth_powerlaw_csr(n, n * 20, 900, seed=41)
    rng = np.random.default_rng(3)
    X = rng.standard_normal((n, sizes[0]), dtype=np.float32)
    Y = rng.integers(0, sizes[-1], size=(n, 1)).astype(np.int32)
    pair = [oracle.Gcn(oracle.Csr(ip, ix, dv, n), sizes, f64acc=f) for f in (False, True)]
    for O in pair:
        ref.oracle_layer_norm(oracle, O)
    plain = oracle.Gcn(oracle.Csr(ip, ix, dv, n), sizes)
    plain.train_forward(X, Y)
    plain.backward()
    for epoch in range(3):
        for O in pair:
            O.train_forward(X, Y)
            O.backward()
        for a, b in zip(pair[0].layers, pair[1].layers):
            grads = [(a.lin.G_W, b.lin.G_W), (a.lin.G_b, b.lin.G_b)]
            if hasattr(a, "norm"):
                grads += [(a.norm.G_gamma, b.norm.G_gamma), (a.norm.G_beta, b.norm.G_beta)]
                assert (1 / a.norm.rstd).min() >= 0.305, (epoch, (1 / a.norm.rstd).min())        # 0.31 to two figures
            for g32, g64 in grads:
                assert ref.relerr(g32, g64) <= 1.5e-6, (epoch, ref.relerr(g32, g64))
        if epoch == 0:
            for a, p in zip(pair[0].layers, plain.layers):
                assert ref.relerr(a.lin.G_W, p.lin.G_W) >= 0.19
        for O in pair:
            O.adam_update()
    for N in pair[0].layers[0].norm, pair[0].layers[1].norm:                 # Adam moved gamma and beta, by lr a step at most
        g0, b0 = ref.params(N.gamma.shape[1], 5 + (N is pair[0].layers[1].norm))
        assert 0 < np.abs(N.gamma - g0).max() <= 3.05e-2 and 0 < np.abs(N.beta - b0).max() <= 3.05e-2
