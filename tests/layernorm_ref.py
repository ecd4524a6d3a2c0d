"""Layer normalisation on the host, for the layer-norm tests: the contract of mggcn_layer_norm_forward_f32 /
mggcn_layer_norm_backward_f32 (include/mggcn.h) restated in fp64 with outputs rounded to fp32, an fp32 numpy twin that
follows the kernel's formulas (two-pass variance included; only the order of the sums differs), the distances the tests
use, and a wrapper that puts the norm into an oracle.Gcn without touching anything under oracle/."""
import types

import numpy as np

EPS = 1e-5
SLOPE = 0.01
ADAM = (1e-2, 0.9, 0.999, 5e-4, 1e-8)


def params(m, seed):
    """a non-trivial gamma and beta (ones and zeros would hide a missing multiply or add)"""
    rng = np.random.default_rng(seed)
    return ((1 + 0.5 * rng.standard_normal(m)).astype(np.float32).reshape(1, m),
            (0.3 * rng.standard_normal(m)).astype(np.float32).reshape(1, m))


# ---- fp64 restatement ---------------------------------------------------------------------------------------------------
def _stats64(x, eps):
    x = np.asarray(x, dtype=np.float64)
    mean = x.mean(axis=1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    return (x - mean) * rstd, rstd


def forward64(x, gamma, beta, leaky=False, eps=EPS, exact=False):
    """(y, xhat, rstd): fp64 arithmetic on the fp32 inputs, rounded to fp32 at the end (exact: left in fp64)"""
    xhat, rstd = _stats64(x, eps)
    z = xhat * np.asarray(gamma, dtype=np.float64) + np.asarray(beta, dtype=np.float64)
    y = np.where(z > SLOPE * z, z, SLOPE * z) if leaky else z
    out = (y, xhat, rstd.reshape(-1))
    return out if exact else tuple(o.astype(np.float32) for o in out)


def backward64(G, act, x, gamma, leaky=False, eps=EPS, exact=False):
    """(G_in, G_gamma, G_beta) from the incoming gradient, the sign source ``act`` (read with the flag only) and the
    forward's INPUT x: xhat and rstd are recomputed in fp64"""
    xhat, rstd = _stats64(x, eps)
    G = np.asarray(G, dtype=np.float64)
    dz = np.where(np.asarray(act) > 0, G, SLOPE * G) if leaky else G
    g = dz * np.asarray(gamma, dtype=np.float64)
    G_in = rstd * (g - g.mean(axis=1, keepdims=True) - xhat * (g * xhat).mean(axis=1, keepdims=True))
    out = (G_in, (dz * xhat).sum(axis=0, keepdims=True), dz.sum(axis=0, keepdims=True))
    return out if exact else tuple(o.astype(np.float32) for o in out)


# ---- fp32 twin: the kernel's formulas ----------------------------------------------------------------------------------------
def _lrelu32(z):
    y = np.float32(SLOPE) * z
    return np.where(z > y, z, y)


def forward32(x, gamma, beta, leaky=False, eps=EPS):
    x = np.asarray(x, dtype=np.float32)
    m = np.float32(x.shape[1])
    mean = x.sum(axis=1, keepdims=True, dtype=np.float32) / m
    d = x - mean
    var = (d * d).sum(axis=1, keepdims=True, dtype=np.float32) / m
    rstd = np.float32(1) / np.sqrt(var + np.float32(eps))
    xhat = d * rstd
    z = xhat * np.asarray(gamma, dtype=np.float32) + np.asarray(beta, dtype=np.float32)
    return (_lrelu32(z) if leaky else z).astype(np.float32), xhat.astype(np.float32), rstd.reshape(-1).astype(np.float32)


def backward32(G, act, xhat, rstd, gamma, leaky=False):
    """from the fp32 xhat and rstd the forward stored, as the kernel does"""
    G, xhat = np.asarray(G, dtype=np.float32), np.asarray(xhat, dtype=np.float32)
    m = np.float32(G.shape[1])
    dz = np.where(np.asarray(act) > 0, G, np.float32(SLOPE) * G).astype(np.float32) if leaky else G
    g = dz * np.asarray(gamma, dtype=np.float32)
    c1 = g.sum(axis=1, keepdims=True, dtype=np.float32) / m
    c2 = (g * xhat).sum(axis=1, keepdims=True, dtype=np.float32) / m
    G_in = np.asarray(rstd, dtype=np.float32).reshape(-1, 1) * ((g - c1) - xhat * c2)
    return (G_in.astype(np.float32), (dz * xhat).sum(axis=0, keepdims=True, dtype=np.float32),
            dz.sum(axis=0, keepdims=True, dtype=np.float32))


# ---- distances ---------------------------------------------------------------------------------------------------------------
def relerr(got, want):
    """the matrix-normalised distance of test_gpu_gcn.py"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-30))


def rowdist(got, want):
    """max over rows of max|delta| / max|want| of that row; relerr for vectors"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.ndim < 2 or got.shape[0] == 1:
        return relerr(got, want)
    return float((np.abs(got - want).max(axis=1) / (np.abs(want).max(axis=1) + 1e-30)).max())


# ---- the norm inside the CPU oracle ------------------------------------------------------------------------------------------
class oracle_layer_norm:
    """Layer normalisation for an oracle.Gcn, by replacing forward / backward of every layer but the last with the same
    sequence plus the norm between aggregation / linear and activation -- the oracle's own lin, spmm_* and leaky_relu_*,
    nothing under oracle/ changes.  The fp32 oracle normalises with the fp32 twin, its f64acc twin with the fp64
    restatement.  Every wrapped layer gets ``norm``: gamma, beta, G_gamma, G_beta and the Adam state; adam_update of the
    model also steps them (no weight decay).  Wrap BEFORE dropout_ref.oracle_dropout, which patches on top."""

    def __init__(self, oracle, O, seed=5):
        self.oracle, self.O = oracle, O
        for li, L in enumerate(O.layers[:-1]):
            assert L.activation
            m = L.lin.W.shape[1]
            gamma, beta = params(m, seed + li)
            L.norm = types.SimpleNamespace(gamma=gamma, beta=beta, G_gamma=np.zeros_like(gamma), G_beta=np.zeros_like(beta),
                                           mg=None, vg=None, mb=None, vb=None, step=0)
            self._patch(L, O.f64acc)
        inner = O.adam_update

        def adam_update(lr=ADAM[0], beta1=ADAM[1], beta2=ADAM[2], weight_decay=ADAM[3], eps=ADAM[4]):
            inner(lr, beta1, beta2, weight_decay, eps)
            for L in O.layers[:-1]:
                self._adam(L.norm, lr, beta1, beta2, eps)
        O.adam_update = adam_update

    def norms(self):
        return [L.norm for L in self.O.layers[:-1]]

    @staticmethod
    def _adam(N, lr, beta1, beta2, eps):
        """the chain linear.adam_update runs for b (gcn.hpp:164-168), in fp32"""
        f = np.float32
        if N.mg is None:
            N.mg, N.vg, N.mb, N.vb = (np.zeros_like(N.gamma) for _ in range(4))
            N.step = 0
        N.step += 1
        bc1, bc2 = f(1 - beta1 ** N.step), f(1 - beta2 ** N.step)
        for p, g, m, v in (("gamma", N.G_gamma, "mg", "vg"), ("beta", N.G_beta, "mb", "vb")):
            mm = f(1 - beta1) * g + f(beta1) * getattr(N, m)
            vv = f(1 - beta2) * g * g + f(beta2) * getattr(N, v)
            setattr(N, m, mm.astype(f)); setattr(N, v, vv.astype(f))
            setattr(N, p, (getattr(N, p) - (f(lr) / bc1) * mm / (np.sqrt(vv / bc2) + f(eps))).astype(f))

    def _patch(self, L, exact):
        orc, N = self.oracle, L.norm

        def forward(H):                                         # GcnLayer.forward with the norm before the activation
            L.H = H
            if L.gemm_first:
                Z = L.spmm_fwd(L.lin.forward(H))
            else:
                Z = L.lin.forward(L.spmm_fwd(H))
            N.x = Z
            if exact:
                Z, _, _ = forward64(Z, N.gamma, N.beta)
            else:
                Z, N.xhat, N.rstd = forward32(Z, N.gamma, N.beta)
            Z = orc.leaky_relu_forward(np.ascontiguousarray(Z))
            if L.res_lin is not None:
                R = L.res_lin
                Z = (Z + R.b).astype(np.float32)
                orc.gemm(H, R.W, Z, 1.0, 1.0, f64acc=R.f64acc)
                R.X = H
            elif L.residual_layer:
                Z = (Z + H).astype(np.float32)
            L.AHW = Z
            return Z

        def backward(G):                                        # GcnLayer.backward with the norm after leaky_relu_backward
            T = orc.leaky_relu_backward(L.AHW, G)
            if exact:
                T, N.G_gamma, N.G_beta = backward64(T, None, N.x, N.gamma)
            else:
                T, N.G_gamma, N.G_beta = backward32(T, None, N.xhat, N.rstd, N.gamma)
            T = np.ascontiguousarray(T)
            if L.gemm_first:
                G_out = L.lin.backward(L.spmm_bwd(T) if L.backward_spmm else T)
            else:
                L.lin.X = L.H
                G_HW = L.lin.backward(T)
                G_out = None if G_HW is None else (L.spmm_bwd(G_HW) if L.backward_spmm else G_HW)
            if L.res_lin is not None:
                R = L.res_lin
                R.G_b = orc.gemm(np.ones((1, G.shape[0]), dtype=np.float32), G, f64acc=R.f64acc)
                R.G_W = orc.gemm(R.X, G, A_T=True, f64acc=R.f64acc)
                if R.backward_out and G_out is not None:
                    orc.gemm(G, R.W, G_out, 1.0, 1.0, B_T=True, f64acc=R.f64acc)
            elif L.residual_layer and G_out is not None:
                G_out = (G_out + G).astype(np.float32)
            return G_out
        L.forward, L.backward = forward, backward
