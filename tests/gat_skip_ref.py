"""The skip connection of the attention layers on the host, for the gat-skip tests: the contract of
mggcn_gated_skip_forward_f32 / mggcn_gated_skip_backward_f32 (include/mggcn.h) restated in fp64, an fp32 numpy twin that
follows the same formulas (only the order of the sums is numpy's), the row scales of gat_ref.rowdist for every output, the
case table, the dispatch of the two kernels restated (which instantiation a width reaches, how many rows one pass of its
grid takes), the bars, and reference models that put the skip, the gate and the layer norm into gat_ref.oracle_gat,
gatv2_ref.oracle_gatv2 and gatdot_ref.oracle_gatdot.

Per row, o the attention output, r the skip linear's output, w [3 x m]:
    add    t = o + r
    gate   s = sum_c (w[0,c] o[c] + w[1,c] r[c] + w[2,c] (o[c] - r[c]));  g = 1 / (1 + exp(-s));  t = g r + (1 - g) o
    y = leaky_relu(t, 0.01) or t
    dy = G . leaky_relu'(act) or G
    add    G_o = G_r = dy
    gate   dg = sum_c dy[c] (r[c] - o[c]);  ds = dg g (1 - g);  G_o = (1 - g) dy + ds (w[0] + w[2]);  G_r = g dy + ds (w[1] - w[2])
           G_w[0] = sum_i ds_i o_i;  G_w[1] = sum_i ds_i r_i;  G_w[2] = sum_i ds_i (o_i - r_i)
"""
import types

import numpy as np

import dropout_ref
import gat_dropout_ref
import gat_ref as ref
import gatdot_ref
import gatv2_ref
import layernorm_ref
from gat_ref import ROW_TOL

SLOPE = 0.01
GATE, LEAKY = 1, 2                                  # MGGCN_GS_GATE, MGGCN_GS_LEAKY_RELU
FWD_NAMES = ("y", "gate")
BWD_NAMES = ("G_o", "G_r", "G_w")
MUTATIONS = {"w2 sign": "y", "g for 1 - g": "G_o", "G_w without the last row": "G_w"}      # mutation -> an output it spoils


def sigmoid(s):
    """1 / (1 + e^-s) from e^-|s|, the kernel's expression: finite for every finite s, exactly 0 / 1 where the format saturates"""
    s = np.asarray(s)
    e = np.exp(-np.abs(s))
    return np.where(s >= 0, 1 / (1 + e), e / (1 + e)).astype(s.dtype)


def skip(o, r, w=None, leaky=False, G=None, act=None, gate=None, dtype=np.float64, scales=False, mutate=None):
    """every quantity of FWD_NAMES (and of BWD_NAMES when G is given) in ``dtype`` arithmetic, unrounded, plus s; w None is
    the add mode (gate and G_w are then None).  ``act`` is the sign source of the backward's activation (read with ``leaky``
    only) and ``gate`` replaces the forward's g in the backward pass, which reads it as an operand.  With ``scales`` the
    result has "scale": per output the magnitude its terms add up to (gat_ref.rowdist) -- for y that includes what an error
    of the size of s's terms moves through g: |r - o| g (1 - g) sum_c |terms of s|.  ``mutate``: one of MUTATIONS, for the
    CPU tests; none of them is the contract."""
    T = dtype
    assert mutate is None or mutate in MUTATIONS
    o, r = np.asarray(o, dtype=T), np.asarray(r, dtype=T)
    n, m = o.shape
    gated = w is not None
    res = {}
    if gated:
        w = np.asarray(w, dtype=T).reshape(3, m)
        w2 = -w[2] if mutate == "w2 sign" else w[2]
        terms = (w[0] * o, w[1] * r, w2 * (o - r))
        s = (terms[0] + terms[1] + terms[2]).sum(axis=1, dtype=T)
        g = sigmoid(s)
        t = g[:, None] * r + (1 - g)[:, None] * o
        res.update(s=s, gate=g)
    else:
        g = None
        t = o + r
        res.update(s=None, gate=None)
    res["y"] = np.where(t > T(SLOPE) * t, t, T(SLOPE) * t) if leaky else t
    if scales:
        act_scale = np.where(t > 0, 1.0, SLOPE) if leaky else 1.0
        if gated:
            s_abs = (np.abs(terms[0]) + np.abs(terms[1]) + np.abs(terms[2])).sum(axis=1)
            g_scale = g * (1 - g) * s_abs + g + 1e-30
            y_scale = g[:, None] * np.abs(r) + (1 - g)[:, None] * np.abs(o) + np.abs(r - o) * (g * (1 - g) * s_abs)[:, None]
            res["scale"] = dict(y=y_scale * act_scale, gate=g_scale)
        else:
            res["scale"] = dict(y=(np.abs(o) + np.abs(r)) * act_scale)
    if G is None:
        return res
    G = np.asarray(G, dtype=T)
    dy = np.where(np.asarray(act) > 0, G, T(SLOPE) * G) if leaky else G
    if not gated:
        res.update(G_o=dy, G_r=dy, G_w=None)
        if scales:
            res["scale"].update(G_o=np.abs(dy), G_r=np.abs(dy))
        return res
    g = g if gate is None else np.asarray(gate, dtype=T).reshape(n)
    dg = (dy * (r - o)).sum(axis=1, dtype=T)
    ds = dg * (g * (1 - g))
    keep = (g if mutate == "g for 1 - g" else 1 - g)[:, None]
    G_o = keep * dy + ds[:, None] * (w[0] + w[2])
    G_r = g[:, None] * dy + ds[:, None] * (w[1] - w[2])
    rows = slice(0, n - 1) if mutate == "G_w without the last row" else slice(0, n)
    dsr = ds[rows, None]
    G_w = np.stack([(dsr * o[rows]).sum(axis=0, dtype=T), (dsr * r[rows]).sum(axis=0, dtype=T),
                    (dsr * (o - r)[rows]).sum(axis=0, dtype=T)])
    res.update(dg=dg, ds=ds, G_o=G_o, G_r=G_r, G_w=G_w)
    if scales:
        ds_abs = np.abs(dy * (r - o)).sum(axis=1) * (g * (1 - g))
        a = np.abs(ds)[:, None]
        res["scale"].update(G_o=(1 - g)[:, None] * np.abs(dy) + ds_abs[:, None] * np.abs(w[0] + w[2]),
                            G_r=g[:, None] * np.abs(dy) + ds_abs[:, None] * np.abs(w[1] - w[2]),
                            G_w=np.stack([(a * np.abs(o)).sum(axis=0), (a * np.abs(r)).sum(axis=0),
                                          (a * np.abs(o - r)).sum(axis=0)]))
    return res


def restate64(*a, exact=False, **kw):
    """the fp64 restatement: fp64 arithmetic on the fp32 inputs, rounded to fp32 at the end (exact: left in fp64)"""
    res = skip(*a, dtype=np.float64, **kw)
    return res if exact else {k: (None if v is None else v.astype(np.float32)) for k, v in res.items() if k != "scale"}


def twin32(*a, **kw):
    """the fp32 twin: the same formulas with every operation in fp32"""
    with np.errstate(over="ignore", under="ignore"):
        return {k: (None if v is None else v.astype(np.float32)) for k, v in skip(*a, dtype=np.float32, **kw).items()}


# ---- the dispatch of csrc/row_group.h, restated --------------------------------------------------------------------------------------------
GRID_CAP = 1024                                     # kLayerNormBlocks = 4 x 256 CUs, workgroups of 256 threads


def instantiation(m, vec):
    """(V, L, K, R) of MGGCN_LN_DISPATCH for a width and the path the alignment selects"""
    if vec:
        assert m % 4 == 0
        q = m // 4
        return (4, 16, 1, 1) if q <= 16 else (4, 16, 2, 1) if q <= 32 else (4, 16, 4, 1) if q <= 64 else \
            (4, 64, 2, 2) if q <= 128 else (4, 64, 4, 1)
    return (1, 16, 1, 1) if m <= 16 else (1, 16, 2, 1) if m <= 32 else (1, 16, 3, 1) if m <= 48 else (1, 16, 4, 1) if m <= 64 else \
        (1, 64, 2, 2) if m <= 128 else (1, 64, 4, 2) if m <= 256 else (1, 64, 8, 1) if m <= 512 else (1, 64, 16, 1)


def rows_per_pass(inst):
    """the rows one trip of the grid-stride loop takes at the full grid: GRID_CAP workgroups x (256 / L) groups x R rows"""
    _, L, _, R = inst
    return GRID_CAP * (256 // L) * R


# one width per instantiation, (m, vec): the float4 path on aligned operands, the element path on every other width
INSTANTIATION_WIDTHS = [(64, True), (128, True), (256, True), (512, True), (1024, True),
                        (7, False), (23, False), (41, False), (57, False), (101, False), (201, False), (257, False), (1023, False)]
assert len({instantiation(m, v) for m, v in INSTANTIATION_WIDTHS}) == 13

# ---- the case table ---------------------------------------------------------------------------------------------------------------------
WIDTHS = (1, 7, 23, 41, 57, 64, 101, 128, 132, 201, 256, 257, 512, 1023, 1024)
ROWS = (1, 37)
FLAGS = (0, LEAKY, GATE, GATE | LEAKY)


def inputs(n, m, seed=29):
    """o, r, G standard normal, w = 0.5 x normal / sqrt(m) (the scores keep a spread of about one at every width, so the
    gates are spread over (0, 1)), and the sign source: the fp32 y of the exact restatement is computed by the caller"""
    rng = np.random.default_rng(seed + 1000 * n + m)
    o = rng.standard_normal((n, m), dtype=np.float32)
    r = rng.standard_normal((n, m), dtype=np.float32)
    G = rng.standard_normal((n, m), dtype=np.float32)
    w = (0.5 / np.sqrt(m) * rng.standard_normal((3, m))).astype(np.float32)
    return o, r, G, w


def cases():
    """(n, m, flags) of every case the bars are measured over and the device runs"""
    return [(n, m, f) for m in WIDTHS for n in ROWS for f in FLAGS]


_cases = {}


TAIL = 4                                            # the rows tail_gain multiplies: the last four


def case(n, m, flags, seed=29, tail_gain=None):
    """inputs, the sign source and the gate the backward pass is handed (the exact restatement's y and g, rounded to
    fp32), the exact restatement with its row scales, and the twin of one case; computed once per process and left
    unchanged by everyone who reads it.  ``tail_gain`` (the multi-pass cases): G of the last TAIL rows is multiplied by it,
    so that those rows carry a visible share of every column sum; such a case is large and is not kept."""
    key = (n, m, flags, seed)
    if tail_gain is not None or key not in _cases:
        o, r, G, w = inputs(n, m, seed)
        if tail_gain is not None:
            G[-TAIL:] *= np.float32(tail_gain)
        gated, leaky = bool(flags & GATE), bool(flags & LEAKY)
        wa = w if gated else None
        fwd = restate64(o, r, wa, leaky)
        act, gate = fwd["y"], fwd["gate"]
        want = restate64(o, r, wa, leaky, G=G, act=act, gate=gate, exact=True, scales=True)
        twin = twin32(o, r, wa, leaky, G=G, act=act, gate=gate)
        c = dict(n=n, m=m, flags=flags, o=o, r=r, G=G, w=wa, act=act, gate=gate, want=want, scale=want["scale"], twin=twin)
        if tail_gain is not None:
            return c
        _cases[key] = c
    return _cases[key]


def names(flags):
    return (FWD_NAMES + BWD_NAMES) if flags & GATE else ("y", "G_o", "G_r")


def distances(got, c):
    """{output: worst rowdist of ``got`` from the exact restatement of case ``c``}; G_w is one row per parameter row, scaled
    per column by sum_i |ds_i| |operand|"""
    out = {}
    for name in names(c["flags"]):
        want, scale = c["want"][name], c["scale"][name]
        if name == "gate":
            want, scale = want.reshape(-1, 1), scale.reshape(-1, 1)
        out[name] = ref.rowerr(np.asarray(got[name]).reshape(want.shape), want, scale)[1]
    return out


# The bar of every output on the row-scaled measure, fixed on the CPU before any device run (the project's rule):
# gat_ref.ROW_TOL where the fp32 twin's worst rowdist from the exact restatement over cases() stays within ROW_TOL / 8,
# eight times the twin's worst, rounded up, otherwise.  TWIN_MEASURED is what test_gat_skip_cpu.py measures (it prints and
# asserts it): y 1.40e-7 at (37, 128, gate + activation), gate 7.34e-8 at (37, 7, gate without activation), G_o 2.21e-7 and G_r 2.28e-7 at (37, 23, gate + activation), G_w 2.66e-5 at (1, 256, gate + activation).
# y, gate, G_o and G_r stay within ROW_TOL / 8 = 1e-5 and get ROW_TOL.  G_w does not, and the reason is the measure the
# issue sets for it, sum_i |ds_i| |operand|: with a single row G_w is ds o, the scale is |ds| |o|, and what is left is the
# relative error of ds = dg g (1 - g) itself, where dg = sum_c dy (r - o) is a sum of 256 terms of both signs that nearly
# cancels in that row (|dg| is a few thousandths of sum |dy (r - o)|).  Its bar is 8 x 2.66e-5, rounded up.
TWIN_MEASURED = dict(y=1.40e-7, gate=7.34e-8, G_o=2.21e-7, G_r=2.28e-7, G_w=2.66e-5)
BAR = dict(y=ROW_TOL, gate=ROW_TOL, G_o=ROW_TOL, G_r=ROW_TOL, G_w=2.2e-4)


def bar_rule(twin_worst):
    return ROW_TOL if twin_worst <= ROW_TOL / 8 else 8 * twin_worst


# ---- the reference models -----------------------------------------------------------------------------------------------------------------
class _skip_model:
    """What the three reference models below share: after the attention of every layer the skip (``skip``: None, "add" or
    "gate": an oracle.Linear ``res`` over the layer's own input -- after feature dropout --, the gate's ``w`` [3 x out],
    seed-99 uniform over an [out x 3] buffer like the engine's) and, in every layer that has an activation, the layer norm
    (``norm``: None or "layer"; layernorm_ref's twin, gamma = 1 and beta = 0 like the engine's), then the oracle's leaky
    ReLU.  The backward pass runs them in reverse, the skip linear's input gradient is added to the layer linear's, and
    Adam steps res like any linear, w by the chain of W (weight decay) and gamma / beta by the chain of b (none).  fp32:
    the twins; dtype=np.float64: the fp64 restatements, rounded to fp32 between the stages."""

    def _init_skip(self, sizes, skip, norm):
        assert skip in (None, "add", "gate") and norm in (None, "layer")
        orc = self.orc
        self.skip_mode, self.norm_mode = skip, norm
        for i, L in enumerate(self.layers):
            out = sizes[i + 1]
            L.res = orc.Linear(sizes[i], out, i != 0) if skip is not None else None
            L.w = orc.init_uniform(out, 3).reshape(3, out).copy() if skip == "gate" else None
            L.G_w = None if L.w is None else np.zeros_like(L.w)
            L.wm = L.wv = None
            L.wstep = 0
            L.norm = None
            if norm == "layer" and L.activation:
                L.norm = types.SimpleNamespace(gamma=np.ones((1, out), dtype=np.float32), beta=np.zeros((1, out), dtype=np.float32),
                                               G_gamma=None, G_beta=None, mg=None, vg=None, mb=None, vb=None, step=0)

    # the attention of the variant: out, and from T the gradient of the linear's output (setting L.G_att where there is one)
    def _attn_out(self, li, L):
        raise NotImplementedError

    def _attn_back(self, li, L, T):
        raise NotImplementedError

    def _drops(self, li, on):
        return on and getattr(self, "p", 0.0) > 0.0 and li > 0

    def forward(self, H):
        orc = self.orc
        H = np.ascontiguousarray(H, dtype=np.float32)
        for li, L in enumerate(self.layers):
            if self._drops(li, getattr(self, "training", False)):
                H = np.ascontiguousarray(dropout_ref.apply(H, 0, self.p, self.seed, self._stream(li)))
            L.Z = L.lin.forward(H)
            L.out = np.ascontiguousarray(self._attn_out(li, L))
            y = L.out
            if L.res is not None:
                L.r = L.res.forward(H)
                f = (restate64 if self.exact else twin32)(L.out, L.r, L.w)
                y, L.g = np.ascontiguousarray(f["y"]), f["gate"]
            if L.norm is not None:
                L.nx = y
                if self.exact:
                    y = layernorm_ref.forward64(y, L.norm.gamma, L.norm.beta)[0]
                else:
                    y, L.norm.xhat, L.norm.rstd = layernorm_ref.forward32(y, L.norm.gamma, L.norm.beta)
            L.y = orc.leaky_relu_forward(np.ascontiguousarray(y)) if L.activation else np.ascontiguousarray(y)
            H = L.y
        return H

    def backward(self):
        orc, G = self.orc, self.G
        for li in reversed(range(len(self.layers))):
            L = self.layers[li]
            T = orc.leaky_relu_backward(L.y, G) if L.activation else G
            if L.norm is not None:
                N = L.norm
                if self.exact:
                    T, N.G_gamma, N.G_beta = layernorm_ref.backward64(T, None, L.nx, N.gamma)
                else:
                    T, N.G_gamma, N.G_beta = layernorm_ref.backward32(T, None, N.xhat, N.rstd, N.gamma)
            G_r = None
            if L.res is not None:
                b = (restate64 if self.exact else twin32)(L.out, L.r, L.w, G=T, gate=L.g)
                T, G_r, L.G_w = b["G_o"], np.ascontiguousarray(b["G_r"]), b["G_w"]
            G = L.lin.backward(self._attn_back(li, L, np.ascontiguousarray(T)))
            if G_r is not None:
                G_skip = L.res.backward(G_r)
                if G is not None:
                    G = (G + G_skip).astype(np.float32)
            if G is not None and self._drops(li, getattr(self, "dropped", False)):
                G = np.ascontiguousarray(dropout_ref.apply(G, 0, self.p, self.seed, self._stream(li)))

    def _adam_w(self, L, lr, beta1, beta2, weight_decay, eps):
        """gat_ref.oracle_gat.adam_update's chain for att, on w"""
        orc = self.orc
        lib, p, f = orc.lib(), orc._ptr, orc.f32p
        if L.wm is None:
            L.wm, L.wv, L.wstep = np.zeros_like(L.w), np.zeros_like(L.w), 0
        L.wstep += 1
        bc1, bc2 = np.float32(1 - beta1 ** L.wstep), np.float32(1 - beta2 ** L.wstep)
        L.w, L.G_w = np.ascontiguousarray(L.w), np.ascontiguousarray(L.G_w)
        lib.orc_axpy(p(L.w, f), p(L.G_w, f), weight_decay, L.w.size)
        lib.orc_axpby(p(L.G_w, f), p(L.wm, f), 1 - beta1, beta1, L.w.size)
        lib.orc_aaxpby(p(L.G_w, f), p(L.wv, f), 1 - beta2, beta2, L.w.size)
        lib.orc_adam_final(p(L.w, f), p(L.wm, f), p(L.wv, f), lr, bc1, bc2, eps, L.w.size)

    def adam_update(self, lr=ref.ADAM[0], beta1=ref.ADAM[1], beta2=ref.ADAM[2], weight_decay=ref.ADAM[3], eps=ref.ADAM[4]):
        super().adam_update(lr, beta1, beta2, weight_decay, eps)
        for L in self.layers:
            if L.res is not None:
                L.res.adam_update(lr, beta1, beta2, weight_decay, eps)
            if L.w is not None:
                self._adam_w(L, lr, beta1, beta2, weight_decay, eps)
            if L.norm is not None:
                layernorm_ref.oracle_layer_norm._adam(L.norm, lr, beta1, beta2, eps)


class oracle_gat_skip(_skip_model, gat_dropout_ref.oracle_gat_dropout):
    """gat(variant="v1", skip=, norm=) on the host, both dropouts included (gat_dropout_ref.oracle_gat_dropout)"""

    def __init__(self, oracle, A, sizes, heads, skip=None, norm=None, **kw):
        gat_dropout_ref.oracle_gat_dropout.__init__(self, oracle, A, sizes, heads, **kw)
        self._init_skip(sizes, skip, norm)

    def _attn_out(self, li, L):
        return self._attention(li, L, self.training)["out"]

    def _attn_back(self, li, L, T):
        res = self._attention(li, L, self.dropped, G=T)
        L.G_att = res["G_att"]
        return np.ascontiguousarray(res["G_Z"])


class oracle_gatv2_skip(_skip_model, gatv2_ref.oracle_gatv2):
    """gat(variant="v2", skip=, norm=) on the host"""

    def __init__(self, oracle, A, sizes, heads, skip=None, norm=None, **kw):
        gatv2_ref.oracle_gatv2.__init__(self, oracle, A, sizes, heads, **kw)
        self._init_skip(sizes, skip, norm)

    def _attn_out(self, li, L):
        return self._twin(L)["out"]

    def _attn_back(self, li, L, T):
        res = self._twin(L, G=T)
        L.G_att = res["G_att"]
        return np.ascontiguousarray(np.concatenate([res["G_Zs"], res["G_Zd"]], axis=1))


class oracle_gatdot_skip(_skip_model, gatdot_ref.oracle_gatdot):
    """gat(variant="dot", skip=, norm=) on the host: with skip="gate" and norm="layer" the UniMP block"""

    def __init__(self, oracle, A, sizes, heads, skip=None, norm=None, **kw):
        gatdot_ref.oracle_gatdot.__init__(self, oracle, A, sizes, heads, **kw)
        self._init_skip(sizes, skip, norm)

    def _attn_out(self, li, L):
        return self._twin(L)["out"]

    def _attn_back(self, li, L, T):
        res = self._twin(L, G=T)
        return np.ascontiguousarray(np.concatenate([res["G_Zq"], res["G_Zk"], res["G_Zv"]], axis=1))


ORACLES = {"v1": oracle_gat_skip, "v2": oracle_gatv2_skip, "dot": oracle_gatdot_skip}
