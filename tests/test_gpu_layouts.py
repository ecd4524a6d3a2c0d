"""The layouts the C ABI accepts beyond contiguous, aligned operands: padded leading dimensions, element offsets of B, C,
A, Z and the vectors, for the SpMM (fp32 and bf16, every plan form), the GEMM entries and the small row / flat kernels.

Every operand lives in a guarded view (guarded.py): pads and guard rows hold NaN patterns, different for inputs and
outputs.  After every call: (a) nothing outside an output's logical matrix changed (bit for bit), (b) every input,
pads included, is unchanged (a re-pitch must never write the caller's B), (c) the logical result meets the fp64
reference at the suite's bar (1e-4 of the row's sum |a||b| budget) or is bit-equal to the contiguous aligned call.
Which kernel a call reaches depends on d, the leading dimensions and the alignment of the pointers (spmm.hip
launch_main / spmm_csr, spmm_sweep.hip sweep_launch_t, gemm.hip gemm_dispatch); the layouts below are chosen to reach
each form."""
import numpy as np
import pytest
import scipy.sparse as sp

from bf16_ref import bf16_bits, widen
from guarded import Guarded

pytestmark = pytest.mark.gpu

TOL = 1e-4
LRELU = 1           # MGGCN_SPMM_LEAKY_RELU
SLOPE = 0.01


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


def _torch():
    import torch
    return torch


def _budget_check(got, want, budget, what):
    """max over rows of |got - want| / (row's largest budget entry) <= TOL, every element finite"""
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} non-finite element(s)"
    scale = np.maximum(budget.max(axis=1, keepdims=True), 1e-30)
    err = float((np.abs(got - want) / scale).max()) if got.size else 0.0
    assert err <= TOL, f"{what}: error {err:.3e} of the row budget"


# ---- SpMM -----------------------------------------------------------------------------------------------------------
N_ROWS = 1500
MAX_D = 256
# the force_sweep fixture of test_gpu_kernels.py, restated; SLICE_ROWS = 400 cuts the 1500 columns into four slices
# (beta chained from slice to slice)
SWEEP_KNOBS = {
    "MGGCN_SPMM_SWEEP_MIN_NNZ": "1", "MGGCN_SPMM_PANEL_ROWS": "64", "MGGCN_SPMM_PANEL_ROWS_NARROW": "96",
    "MGGCN_SPMM_SLICE_ROWS": "400", "MGGCN_SPMM_SWEEP_MIN_RUN_X10": "0",
}
PLANS = {                             # the plan kinds of test_gpu_agg_bf16.py and two more: (environment, d_hint, expected form)
    "null": (None, 0, None),
    "rowsplit": ({"MGGCN_SPMM_ALGO": "rowsplit"}, 0, "form=rowsplit"),
    "sweep-as-given": (dict(SWEEP_KNOBS, MGGCN_SPMM_PERMUTE_COLUMNS="0"), 0, "form=sweep "),
    "sweep-permuted": (dict(SWEEP_KNOBS, MGGCN_SPMM_PERMUTE_COLUMNS="1"), 0, "permuted=1"),
    "sweep-general-pairs": (dict(SWEEP_KNOBS, MGGCN_SPMM_PERMUTE_COLUMNS="0", MGGCN_SPMM_FAST_PAIRS="0"), 0, "form=sweep "),
    "narrow-41": (dict(SWEEP_KNOBS, MGGCN_SPMM_PERMUTE_COLUMNS="0"), 41, "form=sweep-narrow"),
    "narrow-16": (dict(SWEEP_KNOBS, MGGCN_SPMM_PERMUTE_COLUMNS="0"), 16, "form=sweep-narrow"),
    "narrow-41-permuted": (dict(SWEEP_KNOBS, MGGCN_SPMM_PERMUTE_COLUMNS="1"), 41, "permuted=1"),
    # on this small matrix the builder's cost model picks 16 lanes per entry for both hints; the Reddit shape's d = 41
    # form (12 lanes, five rows per gather) and the d = 16 one (4 lanes, sixteen rows) are forced
    "narrow-41-lpe12": (dict(SWEEP_KNOBS, MGGCN_SPMM_PERMUTE_COLUMNS="0", MGGCN_SPMM_NARROW_LPE="12"), 41, "lpe=12 "),
    "narrow-16-lpe4": (dict(SWEEP_KNOBS, MGGCN_SPMM_PERMUTE_COLUMNS="0", MGGCN_SPMM_NARROW_LPE="4"), 16, "lpe=4 "),
}

# (d, ldb, B offset, ldc, C offset), in elements
LAYOUTS = [
    # d = 128: FAST pair at the power-of-two pitches 128 / 256, the general pair at 132; C padded by 1 (the one-column
    # kernels: odd ldc) or by 8 (the pair kernels, C rows no longer at d)
    (128, 128, 0, 128, 0), (128, 128, 0, 129, 0), (128, 128, 0, 136, 0),
    (128, 132, 0, 128, 0), (128, 132, 0, 129, 0), (128, 132, 0, 136, 0),
    (128, 256, 0, 128, 0), (128, 256, 0, 129, 0), (128, 256, 0, 136, 0),
    # FAST pair with d below the pitch: a partial 128-column tile (idle lanes in the upper tile)
    (96, 128, 0, 96, 0), (124, 128, 0, 132, 0), (200, 256, 0, 200, 0), (200, 256, 0, 204, 0),
    # B / C off by one or two elements: 4-byte (generic<1>) and 8-byte (generic<2>) alignment
    (128, 128, 1, 128, 0), (128, 128, 2, 128, 0), (128, 128, 0, 128, 1), (128, 128, 0, 128, 2),
    # d = 41: the quad kernel straight on B at 64-byte pitches (48, 64), re-pitched otherwise (41, 44, a B that is
    # 16-byte but not 64-byte aligned, a B that is not 16-byte aligned)
    (41, 41, 0, 41, 0), (41, 44, 0, 44, 0), (41, 48, 0, 41, 0), (41, 64, 0, 45, 0), (41, 48, 4, 48, 0), (41, 48, 1, 41, 3),
    # d = 16 (the hint-16 plan's quad kernel, LPE 4)
    (16, 16, 0, 16, 0), (16, 20, 0, 17, 0), (16, 16, 2, 16, 1),
    # row-split vec4<16,4> / <8,2> with C padded
    (48, 48, 0, 52, 0), (24, 28, 0, 32, 0),
    # odd and tiny widths
    (66, 67, 0, 66, 0), (66, 68, 0, 70, 0), (1, 3, 0, 1, 0), (3, 4, 0, 5, 0),
]
CASES = [(1.0, 0.0, 0), (0.5, 2.0, LRELU)]        # (alpha, beta, flags); beta = 0 runs over a NaN-filled C


class _Spmm:
    """the power-law test matrix (split rows: max degree 4000 of 1500 columns), its fp64 host copies and its plans"""

    def __init__(self, pkg, ctx):
        n = N_ROWS
        ip, ix, _ = pkg.datasets.synth_powerlaw_csr(n, 60_000, 4000, seed=7)
        rng = np.random.default_rng(3)
        dv = (rng.uniform(0.25, 1.25, ix.shape[0]) * rng.choice([-1.0, 1.0], ix.shape[0])).astype(np.float32)
        self.n, self.ip, self.ix, self.dv = n, ip, ix, dv
        self.A = pkg.csr_matrix(ip, ix, dv, n)
        shape = (n, n)
        self.S = sp.csr_matrix((dv.astype(np.float64), ix.astype(np.int64), ip.astype(np.int64)), shape=shape)
        self.S_abs = sp.csr_matrix((np.abs(dv).astype(np.float64), ix.astype(np.int64), ip.astype(np.int64)), shape=shape)
        self.pkg, self.ctx = pkg, ctx
        self.plans = {}
        self._data = {}

    def plan(self, name):
        if name not in self.plans:
            env, hint, form = PLANS[name]
            if env is None:
                self.plans[name] = None
            else:
                with pytest.MonkeyPatch.context() as mp:
                    for k in ("MGGCN_SPMM_ALGO", "MGGCN_SPMM_FAST_PAIRS", "MGGCN_SPMM_PERMUTE_COLUMNS", "MGGCN_SPMM_NARROW_LPE"):
                        mp.delenv(k, raising=False)
                    for k, v in env.items():
                        mp.setenv(k, v)
                    plan = self.pkg.ops.spmm_plan_for(self.ctx, self.A, MAX_D, hint)
                line = plan.describe()
                assert form in line, line
                if name == "rowsplit":            # heavy rows cut into slices: spmm_combine_kernel runs
                    assert plan.num_split_rows() > 0, line
                else:                             # several column slices (beta chained) and sliced rows: sweep_combine_kernel
                    assert self.ctx.lib.mggcn_spmm_plan_num_slices(plan.handle) > 1, line
                    assert any(int(t[len("split_rows="):]) > 0 for t in line.split() if t.startswith("split_rows=")), line
                self.plans[name] = plan
        return self.plans[name]

    def data(self, d):
        """B (bf16-exact values: the bf16 entry multiplies the same numbers) and a finite C0, per width"""
        if d not in self._data:
            rng = np.random.default_rng(1000 + d)
            bits = bf16_bits(rng.standard_normal((self.n, d), dtype=np.float32))
            self._data[d] = (bits, widen(bits), rng.standard_normal((self.n, d), dtype=np.float32))
        return self._data[d]

    def reference(self, B, C0, alpha, beta, flags):
        B64 = B.astype(np.float64)
        want = alpha * (self.S @ B64)
        budget = abs(alpha) * (self.S_abs @ np.abs(B64))
        if beta != 0.0:
            want = want + beta * C0.astype(np.float64)
            budget = budget + abs(beta) * np.abs(C0.astype(np.float64))
        if flags & LRELU:
            want = np.where(want > 0, want, SLOPE * want)
        return want, budget

    def call(self, plan, Bg, Cg, d, alpha, beta, flags):
        """one SpMM through the C ABI; B in fp32 or bf16 by Bg.bf16"""
        _torch().cuda.synchronize()                      # uploads (torch's stream) before the library's stream
        ip, ix, dv = self.A.device(self.ctx.device)
        fn = self.ctx.lib.mggcn_spmm_csr_bf16 if Bg.bf16 else self.ctx.lib.mggcn_spmm_csr_f32
        fn(self.ctx.stream(0), plan.handle if plan else None, self.n, self.n, ip.data_ptr(), ix.data_ptr(), dv.data_ptr(),
           Bg.ptr, Bg.ld, Cg.ptr, Cg.ld, d, alpha, beta, flags, SLOPE)
        self.ctx.sync()


@pytest.fixture(scope="module")
def spmm(pkg, ctx):
    return _Spmm(pkg, ctx)


def _layout_id(lay):
    d, ldb, bo, ldc, co = lay
    return f"d{d}-ldb{ldb}+{bo}-ldc{ldc}+{co}"


@pytest.mark.parametrize("layout", LAYOUTS, ids=_layout_id)
@pytest.mark.parametrize("plan_kind", list(PLANS))
def test_spmm_layouts(spmm, plan_kind, layout):
    """fp32 and bf16 entries over padded / offset B and C: guards intact, B untouched, reproducible, bf16 == fp32 on
    the widened operand at the same element layout, and the fp64 reference at the row budget"""
    d, ldb, boff, ldc, coff = layout
    plan = spmm.plan(plan_kind)
    bits, Bw, C0 = spmm.data(d)
    B32 = Guarded(spmm.n, d, ldb, boff, logical=Bw)
    B16 = Guarded(spmm.n, d, ldb, boff, logical=bits, bf16=True)
    for alpha, beta, flags in CASES:
        what = f"{plan_kind} {_layout_id(layout)} alpha={alpha} beta={beta} flags={flags}"
        outs = []
        for Bg, entry in ((B32, "fp32"), (B32, "fp32 again"), (B16, "bf16")):
            C = Guarded(spmm.n, d, ldc, coff, logical=C0 if beta != 0.0 else None, output=True)
            spmm.call(plan, Bg, C, d, alpha, beta, flags)
            cb = C.bits()
            C.check_guards(f"{what} [{entry}] C", cb)
            outs.append(C.logical_bits(cb))
        assert np.array_equal(outs[0], outs[1]), f"{what}: two fp32 calls differ"
        assert np.array_equal(outs[0], outs[2]), \
            f"{what}: bf16 entry differs from the fp32 entry ({int((outs[0] != outs[2]).sum())} element(s))"
        want, budget = spmm.reference(Bw, C0, alpha, beta, flags)
        _budget_check(outs[0].view(np.float32), want, budget, what)
    B32.check_unchanged(f"{plan_kind} {_layout_id(layout)} fp32 B")
    B16.check_unchanged(f"{plan_kind} {_layout_id(layout)} bf16 B")


@pytest.mark.parametrize("plan_kind", list(PLANS))
def test_spmm_nonfinite_rows_stay_contained(spmm, plan_kind):
    """one row of B +Inf, another NaN: exactly the output rows with an entry in those columns turn non-finite (in every
    column -- Inf or NaN: a zero-valued pad entry of the sweep plan times Inf is NaN); every other row is bit-identical
    to the run with those rows finite.  Column 0 is one of them: a pad entry that pointed at column 0 instead of a
    column of its own row would poison rows that never reference it."""
    plan = spmm.plan(plan_kind)
    c_inf, c_nan = 0, 777
    rows = np.repeat(np.arange(spmm.n), np.diff(spmm.ip.astype(np.int64)))
    hit = np.zeros(spmm.n, dtype=bool)
    hit[rows[(spmm.ix == c_inf) | (spmm.ix == c_nan)]] = True
    assert 0 < hit.sum() < spmm.n // 4
    for d, ldb in ((128, 128), (96, 128), (41, 41), (16, 16), (3, 3)):
        bits, Bw, _ = spmm.data(d)
        bad_w, bad_bits = Bw.copy(), bits.copy()
        bad_w[c_inf], bad_bits[c_inf] = np.float32(np.inf), 0x7F80
        bad_w[c_nan], bad_bits[c_nan] = np.float32(np.nan), 0x7FC0
        for bf16, good, bad in ((False, Bw, bad_w), (True, bits, bad_bits)):
            res = []
            for B in (good, bad):
                Bg = Guarded(spmm.n, d, ldb, 0, logical=B, bf16=bf16)
                C = Guarded(spmm.n, d, d, 0, output=True)
                spmm.call(plan, Bg, C, d, 1.0, 0.0, 0)
                cb = C.bits()
                C.check_guards(f"{plan_kind} d={d} bf16={bf16} C", cb)
                res.append(C.logical_bits(cb))
            what = f"{plan_kind} d={d} bf16={bf16}"
            assert np.array_equal(res[0][~hit], res[1][~hit]), \
                f"{what}: rows that never reference the non-finite columns changed"
            poisoned = res[1][hit].view(np.float32)
            assert not np.isfinite(poisoned).any(), \
                f"{what}: {int(np.isfinite(poisoned).sum())} finite element(s) in rows that reference them"
            assert np.isfinite(res[0].view(np.float32)).all(), what


# ---- GEMM -----------------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(300, 128, 608), (300, 41, 128), (128, 41, 3001), (2, 3, 2)]    # tile, narrow N, split-K, tiny
THIN_SHAPE = (3, 130, 5000)                                                   # M <= 4, K >= 4096, no transposes
GEMM_CONFIGS = [(s, ta, tb) for s in GEMM_SHAPES for ta in (0, 1) for tb in (0, 1)] + [(THIN_SHAPE, 0, 0)]
COLSUM_SHAPES = [(300, 128, 608), (128, 41, 3001), (2, 3, 2)]
ALPHA = 0.75


def _gemm_variants(ea, eb, ec):
    """(name, (lda, off), (ldb, off), (ldc, off), (ldz / vector, off)); the first is the contiguous aligned baseline"""
    up4 = lambda e: (e + 3) // 4 * 4
    v = [("contiguous", (ea, 0), (eb, 0), (ec, 0), (ec, 0)),
         ("ld+1, offsets 1/2/3", (ea + 1, 1), (eb + 1, 2), (ec + 1, 3), (ec + 3, 1)),
         ("ld+4", (ea + 4, 0), (eb + 4, 0), (ec + 4, 0), (ec + 8, 0)),
         ("offsets 3/1/2", (ea, 3), (eb, 1), (ec, 2), (ec, 3))]
    if any(up4(e) != e for e in (ea, eb, ec)):          # ld % 4 == 0 over an odd extent (the gemm.hip sub-view case)
        v.append(("ld rounded up to 4", (up4(ea), 0), (up4(eb), 0), (up4(ec), 0), (up4(ec) + 4, 2)))
    return v


def _gemm_call(ctx, entry, ta, tb, M, N, K, var, data, beta):
    """one call on guarded operands; returns (C bits, colsum bits or None) after the guard / input checks"""
    lib = ctx.lib
    torch = _torch()
    name, (lda, oa), (ldb, ob), (ldc, oc), (ldz, oz) = var
    A = Guarded(*data["A"].shape, lda, oa, logical=data["A"])
    B = Guarded(*data["B"].shape, ldb, ob, logical=data["B"])
    C = Guarded(M, N, ldc, oc, logical=data["C0"] if beta != 0.0 else None, output=True)
    inputs, outputs = [A, B], [C]
    if entry == "colsum":
        wsb = lib.mggcn_gemm_tn_colsum_workspace_bytes(M, N, K)
    else:
        wsb = lib.mggcn_gemm_workspace_bytes(ta, tb, M, N, K)
    ws = torch.empty(max(int(wsb), 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = ctx.stream(0)
    if entry == "gemm":
        lib.mggcn_gemm_f32(st, ta, tb, M, N, K, ALPHA, A.ptr, lda, B.ptr, ldb, beta, C.ptr, ldc, ws.data_ptr(), wsb)
    elif entry == "bias":
        bias = Guarded(1, N, N, oz, logical=data["bias"])
        inputs.append(bias)
        lib.mggcn_gemm_bias_f32(st, ta, tb, M, N, K, ALPHA, A.ptr, lda, B.ptr, ldb, bias.ptr, C.ptr, ldc, ws.data_ptr(), wsb)
    elif entry == "lrelu":
        Z = Guarded(M, N, ldz, oz, logical=data["Z"])
        inputs.append(Z)
        lib.mggcn_gemm_lrelu_bwd_f32(st, ta, tb, M, N, K, ALPHA, A.ptr, lda, B.ptr, ldb, Z.ptr, ldz, SLOPE, C.ptr, ldc,
                                     ws.data_ptr(), wsb)
    else:
        S = Guarded(1, N, N, oz, output=True)
        outputs.append(S)
        lib.mggcn_gemm_tn_colsum_f32(st, M, N, K, ALPHA, A.ptr, lda, B.ptr, ldb, C.ptr, ldc, S.ptr, ws.data_ptr(), wsb)
    ctx.sync()
    res = []
    for g, label in zip(outputs, ("C", "colsum")):
        b = g.bits()
        g.check_guards(f"{entry} [{name}] {label}", b)
        res.append(g.logical_bits(b))
    for g in inputs:
        g.check_unchanged(f"{entry} [{name}] input")
    return res[0], (res[1] if len(res) > 1 else None)


def _gemm_reference(entry, ta, tb, data, beta):
    A, B = data["A"].astype(np.float64), data["B"].astype(np.float64)
    opA, opB = (A.T if ta else A), (B.T if tb else B)
    want = ALPHA * (opA @ opB)
    budget = abs(ALPHA) * (np.abs(opA) @ np.abs(opB))
    if entry == "gemm" and beta != 0.0:
        want = want + beta * data["C0"]
        budget = budget + abs(beta) * np.abs(data["C0"].astype(np.float64))
    if entry == "bias":
        want = want + data["bias"][0]
        budget = budget + np.abs(data["bias"][0].astype(np.float64))
    if entry == "lrelu":
        f = np.where(data["Z"] > 0, 1.0, SLOPE)
        want, budget = want * f, budget * f
    return want, budget


def _gemm_data(M, N, K, ta, tb, seed):
    rng = np.random.default_rng(seed)
    sa = (K, M) if ta else (M, K)
    sb = (N, K) if tb else (K, N)
    return {"A": rng.standard_normal(sa, dtype=np.float32), "B": rng.standard_normal(sb, dtype=np.float32),
            "C0": rng.standard_normal((M, N), dtype=np.float32), "bias": rng.standard_normal((1, N), dtype=np.float32),
            "Z": rng.standard_normal((M, N), dtype=np.float32)}


def _gemm_layouts(ctx, entry, ta, tb, M, N, K, betas):
    data = _gemm_data(M, N, K, ta, tb, seed=M * 7 + N * 3 + K + 11 * ta + 13 * tb)
    variants = _gemm_variants(M if ta else K, K if tb else N, N)
    for beta in betas:
        base, base_s = _gemm_call(ctx, entry, ta, tb, M, N, K, variants[0], data, beta)
        what = f"{entry} M={M} N={N} K={K} ta={ta} tb={tb} beta={beta}"
        want, budget = _gemm_reference(entry, ta, tb, data, beta)
        _budget_check(base.view(np.float32), want, budget, what)
        if base_s is not None:
            B64 = data["B"].astype(np.float64)
            _budget_check(base_s.view(np.float32), ALPHA * B64.sum(axis=0, keepdims=True),
                          np.abs(ALPHA) * np.abs(B64).sum(axis=0, keepdims=True), what + " colsum")
        for var in variants[1:]:
            got, got_s = _gemm_call(ctx, entry, ta, tb, M, N, K, var, data, beta)
            # the split, the tile width and the summation order depend on (M, N, K) only; the float4 and the scalar
            # loads stage the same values into LDS
            assert np.array_equal(got, base), \
                f"{what} [{var[0]}]: differs from the contiguous call ({int((got != base).sum())} element(s))"
            if base_s is not None:
                assert np.array_equal(got_s, base_s), f"{what} [{var[0]}]: column sums differ from the contiguous call"


def _cfg_id(cfg):
    (M, N, K), ta, tb = cfg
    return f"{M}x{N}x{K}-{'T' if ta else 'N'}{'T' if tb else 'N'}"


@pytest.mark.parametrize("cfg", GEMM_CONFIGS, ids=_cfg_id)
@pytest.mark.parametrize("entry", ["gemm", "bias", "lrelu"])
def test_gemm_layouts(ctx, entry, cfg):
    (M, N, K), ta, tb = cfg
    _gemm_layouts(ctx, entry, ta, tb, M, N, K, (0.0, 0.5) if entry == "gemm" else (0.0,))


@pytest.mark.parametrize("shape", COLSUM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm_tn_colsum_layouts(ctx, shape):
    M, N, K = shape
    _gemm_layouts(ctx, "colsum", 1, 0, M, N, K, (0.0,))


# ---- the small row kernels ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,ld_src,off_src,ld_dst,off_dst", [
    (64, 64, 0, 64, 0), (64, 68, 0, 72, 0), (64, 68, 1, 72, 0), (64, 64, 0, 68, 3), (41, 44, 2, 48, 1), (41, 41, 0, 41, 0),
])
def test_gather_rows_layouts(ctx, d, ld_src, off_src, ld_dst, off_dst):
    torch = _torch()
    rng = np.random.default_rng(d + ld_src + off_src)
    n_src, n_idx = 500, 700
    X = rng.standard_normal((n_src, d), dtype=np.float32)
    idx = rng.integers(0, n_src, n_idx).astype(np.uint32)
    idx[:3] = [n_src - 1, 0, n_src - 1]
    src = Guarded(n_src, d, ld_src, off_src, logical=X)
    dst = Guarded(n_idx, d, ld_dst, off_dst, output=True)
    idx_d = torch.from_numpy(idx.view(np.int32)).cuda()
    torch.cuda.synchronize()
    ctx.lib.mggcn_gather_rows_f32(ctx.stream(0), src.ptr, ld_src, idx_d.data_ptr(), n_idx, d, dst.ptr, ld_dst)
    ctx.sync()
    b = dst.bits()
    dst.check_guards("gather_rows dst", b)
    src.check_unchanged("gather_rows src")
    assert np.array_equal(dst.logical_bits(b), X.view(np.uint32)[idx])


def _convert_input(n, m, seed):
    """finite values over the whole exponent range, rounding ties, bf16 overflow and infinities (no NaN: compared bit for
    bit against torch's cast)"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, m)) * np.exp(rng.uniform(-40, 40, (n, m)))).astype(np.float32)
    special = np.array([0x3F808000, 0x3F818000, 0x00008000, 0x00018000, 0x80028000, 0x7F7F8000, 0x7F7FFFFF, 0xFF7FFFFF,
                        0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x3F807FFF, 0x3F808001, 0x00000000, 0x80000000],
                       dtype=np.uint32).view(np.float32)
    flat = x.reshape(-1)
    flat[:special.size] = special
    flat[-special.size:] = special[::-1]
    return x


@pytest.mark.parametrize("m,ld_src,off_src,ld_dst,off_dst", [
    (128, 128, 0, 128, 0), (128, 132, 1, 136, 0), (128, 128, 3, 128, 0), (128, 128, 0, 132, 1), (128, 132, 2, 128, 2),
    (40, 44, 3, 41, 0),
])
def test_convert_f32_bf16_layouts(ctx, m, ld_src, off_src, ld_dst, off_dst):
    torch = _torch()
    n = 333
    x = _convert_input(n, m, seed=m + off_src)
    src = Guarded(n, m, ld_src, off_src, logical=x)
    dst = Guarded(n, m, ld_dst, off_dst, output=True, bf16=True)
    torch.cuda.synchronize()
    ctx.lib.mggcn_convert_f32_bf16(ctx.stream(0), src.ptr, ld_src, dst.ptr, ld_dst, n, m)
    ctx.sync()
    b = dst.bits()
    dst.check_guards("convert dst", b)
    src.check_unchanged("convert src")
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(dst.logical_bits(b), want)


FLAT_SIZE = 4100                                       # % 4 == 0: only the pointers decide between float4 and scalar
FLAT_OPS = {                                           # name: (inputs, in-place outputs, new outputs, call)
    "leaky_relu_forward": (1, 0, 1, lambda L, s, p, n: L.mggcn_leaky_relu_forward_f32(s, p[0], p[1], n, 0.03)),
    "leaky_relu_backward": (2, 0, 1, lambda L, s, p, n: L.mggcn_leaky_relu_backward_f32(s, p[0], p[1], p[2], n, 0.03)),
    "axpby": (1, 1, 0, lambda L, s, p, n: L.mggcn_axpby_f32(s, p[0], p[1], 0.7, -1.3, n)),
    "aaxpby": (1, 1, 0, lambda L, s, p, n: L.mggcn_aaxpby_f32(s, p[0], p[1], 0.7, -1.3, n)),
    "axpy": (1, 1, 0, lambda L, s, p, n: L.mggcn_axpy_f32(s, p[0], p[1], -0.3, n)),
    "scale_mat": (0, 1, 0, lambda L, s, p, n: L.mggcn_scale_mat_f32(s, p[0], 1.7, n)),
}


@pytest.mark.parametrize("op", list(FLAT_OPS))
def test_flat_maps_on_offset_pointers(ctx, op):
    """every operand 1-3 floats off 16-byte alignment (the scalar kernel) against the aligned call (the float4 kernel):
    bit-equal, and nothing past either end written"""
    torch = _torch()
    n_in, n_inplace, n_out, fn = FLAT_OPS[op]
    rng = np.random.default_rng(len(op))
    vals = [rng.standard_normal((1, FLAT_SIZE), dtype=np.float32) for _ in range(n_in + n_inplace)]
    results = []
    for offs in ((0, 0, 0), (1, 2, 3), (3, 1, 2), (2, 3, 1)):
        ins = [Guarded(1, FLAT_SIZE, FLAT_SIZE, offs[k], logical=vals[k]) for k in range(n_in)]
        inplace = [Guarded(1, FLAT_SIZE, FLAT_SIZE, offs[n_in], logical=vals[n_in], output=True)] if n_inplace else []
        outs = [Guarded(1, FLAT_SIZE, FLAT_SIZE, offs[n_in], output=True)] if n_out else []
        torch.cuda.synchronize()
        fn(ctx.lib, ctx.stream(0), [g.ptr for g in ins + inplace + outs], FLAT_SIZE)
        ctx.sync()
        for g in ins:
            g.check_unchanged(f"{op} offsets {offs} input")
        (res,) = inplace + outs
        b = res.bits()
        res.check_guards(f"{op} offsets {offs} output", b)
        results.append(res.logical_bits(b))
    for k in range(1, len(results)):
        assert np.array_equal(results[k], results[0]), f"{op}: misaligned call {k} differs from the aligned call"
    got = results[0].view(np.float32).astype(np.float64)
    x = vals[0].astype(np.float64)
    want = {"leaky_relu_forward": lambda: np.where(x > 0, x, 0.03 * x),
            "leaky_relu_backward": lambda: np.where(x > 0, vals[1], 0.03 * vals[1].astype(np.float64)),
            "axpby": lambda: 0.7 * x - 1.3 * vals[1],
            "aaxpby": lambda: 0.7 * x * x - 1.3 * vals[1],
            "axpy": lambda: -0.3 * x + vals[1],
            "scale_mat": lambda: 1.7 * x}[op]()
    scale = np.abs(x).max() ** (2 if op == "aaxpby" else 1) + (np.abs(vals[1]).max() if len(vals) > 1 else 0.0)
    assert np.abs(got - want).max() <= 1e-6 * scale, op
