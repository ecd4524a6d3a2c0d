"""The three entries of csrc/propagate.hip (include/mggcn.h: mggcn_cs_residual_f32, mggcn_cs_step_f32, mggcn_cs_correct_f32),
each alone through the C ABI with raw pointers, against the fp32 twin and the fp64 restatement of cs_ref.py.  Every
operand sits in a guarded.Guarded buffer (NaN patterns around the logical matrix, checked bit for bit).

residual and correct: the row-scaled measure of gat_ref (rowdist) against fp64, at eight times the twin's worst distance
over the same cases -- computed here, once -- and never above gat_ref.ROW_TOL; sums_device[0] by the same rule, relative.
step: bit for bit with the twin on operands of at most 12 significant bits (the exact value rounds once), within one ulp
on unrestricted ones.  Every output is written twice and compared as bits."""
import functools

import numpy as np
import pytest

import cs_ref as ref
from gat_ref import ROW_TOL, rowdist
from guarded import Guarded

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 16, 41, 64, 65, 130, 1024)          # both row layouts and every K of each; element and float4 step paths
ROWS = (1, 5, 257, 1031)                            # less than one group, one workgroup, several
# more than one grid pass of the row kernels (their grid is capped at 1024 workgroups of 16 or 4 rows)
SHAPES = [(m, n) for m in WIDTHS for n in ROWS] + [(3, 16500), (130, 4200)]
FIX, AUTOSCALE, SET_LABELS = 1, 2, 4


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


def _ints(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def _in(a, off=0):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return Guarded(a.shape[0], a.shape[1], a.shape[1], off, logical=a)


def _out(n, m, off=0):
    return Guarded(n, m, m, off, output=True)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def case(m, n):
    """logits, labels and sets (0 / 1 / 2 / 7; exactly one training row where n == 5), the residual's reference and twin,
    and the inputs of the correct kernel: the twin's P, an E that is the twin's E0 plus noise on every other row (the rest
    of the rows that do not train stay zero: their quotient is not finite), the twin's sum"""
    rng = np.random.default_rng(1000 * m + n)
    logits = (3.0 * rng.standard_normal((n, m))).astype(np.float32)
    Y = rng.integers(0, m, size=n).astype(np.int32)
    S = rng.choice([0, 1, 2, 7], size=n, p=[0.4, 0.2, 0.3, 0.1]).astype(np.int32)
    if n == 5:
        S = np.array([2, 7, 0, 1, 2], dtype=np.int32)
    S[0 if n != 5 else 2] = 0
    want = dict(zip(("P", "E0", "total"), ref.residual(logits, Y, S, 0, np.float64)))
    twin = dict(zip(("P", "E0", "total"), ref.residual(logits, Y, S, 0, np.float32)))
    E = twin["E0"].copy()
    E[::2] += (0.01 * rng.standard_normal((n, m))).astype(np.float32)[::2]
    inv_T = ref.inv_count(S, 0, np.float32)
    c = dict(m=m, n=n, logits=logits, Y=Y, S=S, want=want, twin=twin, E=E, inv_T=inv_T, total=np.float32(twin["total"]))
    for name, (auto, labels) in (("auto", (True, True)), ("fixed", (False, False))):
        for kind, dt in (("want", np.float64), ("twin", np.float32)):
            Z, s = ref.correct(twin["P"], E, Y, S, 0, c["total"], inv_T, 0.75, auto, labels, dt)
            c[name + "_" + kind] = dict(Z=Z, s=s, P=twin["P"].astype(dt), E=E.astype(dt))
    c["quotient"] = ref.row_scale(E, c["total"], inv_T, np.float64)[1]
    return c


def _z_dist(got, c, name):
    w = c[name + "_want"]
    return rowdist(got, w["Z"], ref.z_scale(w)).max()


def _rel(got, want):
    return abs(float(got) - float(want)) / float(want) if want != 0 else (0.0 if got == 0 else np.inf)


@functools.lru_cache(maxsize=None)
def bars():
    """eight times the twin's worst distance over all the cases, per output, never above ROW_TOL"""
    worst = dict(P=0.0, E0=0.0, total=0.0, Z=0.0)
    for m, n in SHAPES:
        c = case(m, n)
        ones = np.ones((n, m))
        worst["P"] = max(worst["P"], rowdist(c["twin"]["P"], c["want"]["P"], ones).max())
        worst["E0"] = max(worst["E0"], rowdist(c["twin"]["E0"], c["want"]["E0"], ones).max())
        worst["total"] = max(worst["total"], _rel(c["twin"]["total"], c["want"]["total"]))
        for name in ("auto", "fixed"):
            worst["Z"] = max(worst["Z"], _z_dist(c[name + "_twin"]["Z"], c, name))
    out = {k: min(8.0 * v, ROW_TOL) for k, v in worst.items()}
    print("[cs] bars (8 x the twin's worst):", {k: f"{v:.3e}" for k, v in out.items()})
    assert all(v > 0 for v in out.values())
    return out


def _residual(ctx, c, out_P, out_E0, sums):
    ctx.lib.mggcn_cs_residual_f32(ctx.stream(0), c["_logits"].ptr, c["_Y"].data_ptr(), c["_S"].data_ptr(), c["n"], c["m"], 0,
                                  out_P.ptr, out_E0.ptr, sums.data_ptr())


@pytest.mark.parametrize("m,n", SHAPES)
def test_residual(ctx, m, n):
    import torch
    c, bar = dict(case(m, n)), bars()
    c["_logits"], c["_Y"], c["_S"] = _in(c["logits"]), _ints(c["Y"]), _ints(c["S"])
    outs = [(_out(n, m), _out(n, m), torch.full((3,), 123.0, device="cuda")) for _ in range(2)]
    ctx.sync()
    for P, E0, sums in outs:
        _residual(ctx, c, P, E0, sums)
    ctx.sync()
    c["_logits"].check_unchanged("logits")
    for P, E0, sums in outs:
        P.check_guards("P")
        E0.check_guards("E0")
        assert sums.cpu().numpy()[1:].tolist() == [123.0, 123.0]             # one float is written
    (P, E0, sums), (P2, E02, sums2) = outs
    np.testing.assert_array_equal(P.logical_bits(), P2.logical_bits())       # the same bits on every call
    np.testing.assert_array_equal(E0.logical_bits(), E02.logical_bits())
    np.testing.assert_array_equal(_bits(sums.cpu().numpy()), _bits(sums2.cpu().numpy()))
    gP, gE, gt = P.values(), E0.values(), float(sums.cpu().numpy()[0])
    ones = np.ones((n, m))
    dP, dE, dt = rowdist(gP, c["want"]["P"], ones).max(), rowdist(gE, c["want"]["E0"], ones).max(), _rel(gt, c["want"]["total"])
    print(f"[cs] residual m={m} n={n}: P {dP:.3e} E0 {dE:.3e} sum {dt:.3e} (bars {bar['P']:.3e} {bar['E0']:.3e} {bar['total']:.3e})")
    assert not E0.logical_bits()[c["S"] != 0].any()                          # +0.0, as bits, outside the training set
    assert dP <= bar["P"] and dE <= bar["E0"] and dt <= bar["total"]
    if m == 1:                                      # P = 1, E0 = 0, sigma = 0 -- exactly
        assert (gP == 1.0).all() and not E0.logical_bits().any() and _bits(np.array([gt]))[0] == 0


def _correct(ctx, P, E, Y, S, n, m, sums, inv_T, scale, flags, out):
    ctx.lib.mggcn_cs_correct_f32(ctx.stream(0), P.ptr, E.ptr, Y.data_ptr() if Y is not None else None,
                                 S.data_ptr() if S is not None else None, n, m, 0,
                                 sums.data_ptr() if sums is not None else None, inv_T, scale, flags, out.ptr)


@pytest.mark.parametrize("m,n", SHAPES)
def test_correct(ctx, m, n):
    import torch
    c, bar = case(m, n), bars()
    assert ref.threshold_clear(c["quotient"]), "a row's quotient sits on the switch at 1000: choose another seed"
    Y, S = _ints(c["Y"]), _ints(c["S"])
    sums = torch.from_numpy(np.array([c["total"]], dtype=np.float32)).cuda()
    P, E = _in(c["twin"]["P"]), _in(c["E"])
    fixed = [_out(n, m), _out(n, m)]
    alias = [_in(c["twin"]["P"]), _in(c["twin"]["P"])]                       # out = P, with the labels written in
    ctx.sync()
    for out in fixed:
        _correct(ctx, P, E, None, None, n, m, None, 0.0, 0.75, 0, out)
    for buf in alias:
        _correct(ctx, buf, E, Y, S, n, m, sums, c["inv_T"], 1.0, AUTOSCALE | SET_LABELS, buf)
    ctx.sync()
    P.check_unchanged("P")
    E.check_unchanged("E")
    for g in fixed + alias:
        g.check_guards("out")
    np.testing.assert_array_equal(fixed[0].logical_bits(), fixed[1].logical_bits())
    np.testing.assert_array_equal(alias[0].logical_bits(), alias[1].logical_bits())
    d_fixed, d_auto = _z_dist(fixed[0].values(), c, "fixed"), _z_dist(alias[0].values(), c, "auto")
    print(f"[cs] correct m={m} n={n}: scale {d_fixed:.3e} autoscale + labels {d_auto:.3e} (bar {bar['Z']:.3e})")
    assert d_fixed <= bar["Z"] and d_auto <= bar["Z"]
    train = c["S"] == 0
    np.testing.assert_array_equal(alias[0].values()[train], ref.onehot(c["Y"], m, np.float32)[train])
    if m == 1:                                      # sigma = 0 and E = 0 on the rows without noise: 0 / 0 -> s = 1 -> Z = P
        quiet = np.ones(n, dtype=bool)
        quiet[::2] = False
        np.testing.assert_array_equal(alias[0].logical_bits()[quiet & ~train], _bits(c["twin"]["P"])[quiet & ~train])


@pytest.mark.parametrize("m", [4, 65])
def test_scale_rule(ctx, m):
    """sigma = 1: a row with E = 0 (the quotient is infinite) and a row whose quotient is just above 1000 take s = 1, a row
    just below takes the quotient; sigma = 0 with E = 0 (0 / 0) takes s = 1 as well"""
    import torch
    P = np.full((4, m), 1.0 / m, dtype=np.float32)
    E = np.zeros((4, m), dtype=np.float32)
    E[1, m - 1] = np.float32(1.0 / 1000.5)
    E[2, 0] = -np.float32(1.0 / 999.5)
    E[3, :2] = 0.25
    for total, inv_T in ((3.0, 1.0 / 3.0), (0.0, 1.0)):
        inv32 = float(np.float32(inv_T))
        want, s64 = ref.correct(P, E, None, None, 0, np.float32(total), inv32, 1.0, True, False, np.float64)
        q = ref.row_scale(E, np.float32(total), inv32, np.float64)[1]
        if total:
            assert not np.isfinite(q[0]) and 1000.0 < q[1] < 1001.0 and 999.0 < q[2] < 1000.0 and s64.tolist()[:2] == [1.0, 1.0]
        else:
            assert np.isnan(q[0]) and s64[0] == 1.0
        dP, dE, out = _in(P), _in(E), _out(4, m)
        sums = torch.from_numpy(np.array([total], dtype=np.float32)).cuda()
        ctx.sync()
        _correct(ctx, dP, dE, None, None, 4, m, sums, inv32, 1.0, AUTOSCALE, out)
        ctx.sync()
        out.check_guards("out")
        got = out.values()
        np.testing.assert_array_equal(_bits(got[0]), _bits(P[0]))            # E = 0: P's row
        if total:
            np.testing.assert_array_equal(_bits(got[1]), _bits(P[1] + E[1]))     # s = 1 exactly: one fp32 add
        else:
            np.testing.assert_array_equal(_bits(got[1:]), _bits(P[1:]))          # sigma = 0: s = 0 where E is not
        sc = np.broadcast_to((np.abs(P) + np.abs(s64[:, None] * E)).max(axis=1, keepdims=True), P.shape)
        assert rowdist(got, want, sc).max() <= bars()["Z"]
        if total:
            assert abs(got[2, 0] - (1.0 / m - 999.5 / 999.5)) < 1e-3           # s ~ 999.5, not 1


# ---- the step ----------------------------------------------------------------------------------------------------------------------
def _q12(x):
    """x rounded to 12 significant bits (zeros, infinities and signs kept)"""
    fr, ex = np.frexp(np.asarray(x, dtype=np.float64))
    return np.ldexp(np.round(np.ldexp(fr, 12)), ex - 12).astype(np.float32)


def _ordered(a):
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def _step_inputs(m, n, seed, coarse):
    rng = np.random.default_rng(seed)
    T, R = 2.0 * rng.standard_normal((n, m)), 1.5 * rng.standard_normal((n, m))     # well beyond both edges of [-1, 1] and [0, 1]
    flat_T, flat_R = T.reshape(-1), R.reshape(-1)
    k = rng.integers(0, n * m, size=max(4, n * m // 16))
    flat_T[k[0::4]], flat_R[k[0::4]] = 0.0, -0.0
    flat_T[k[1::4]], flat_R[k[1::4]] = -0.0, -0.0
    flat_T[k[2::4]] = 0.0
    flat_R[k[3::4]] = 0.0
    T, R = T.astype(np.float32), R.astype(np.float32)
    return (_q12(T), _q12(R)) if coarse else (T, R)


@pytest.mark.parametrize("m,n", SHAPES)
def test_step(ctx, m, n):
    rng = np.random.default_rng(7 * m + n)
    S = rng.choice([0, 1, 2, 7], size=n).astype(np.int32)
    S[0] = 0
    dS = _ints(S)
    al12, be12 = float(_q12(0.8)), float(_q12(0.2))
    al, be = ref.factors(0.8)
    #        coarse  fix    out is T  base offset  (lo, hi)            factors
    runs = [(True, False, False, 0, (-1.0, 1.0), (al12, be12)),
            (True, True, True, 0, (-ref.INF, ref.INF), (al12, be12)),
            (True, False, True, 1, (0.0, 1.0), (al12, be12)),      # a base one float off alignment: the element path
            (True, True, False, 1, (0.0, 1.0), (al12, be12)),
            (False, True, False, 0, (-1.0, 1.0), (al, be)),
            (False, False, True, 0, (0.0, 1.0), (al, be))]
    for i, (coarse, fix, inplace, off, (lo, hi), (a, b)) in enumerate(runs):
        T, R = _step_inputs(m, n, 100 * m + n + i, coarse)
        twin = ref.step(T, R, S, a, b, lo, hi, 0, fix, np.float32)
        got = []
        for _ in range(2):
            dT, dR = _in(T, off), _in(R, off)
            out = dT if inplace else _out(n, m, off)
            ctx.sync()
            ctx.lib.mggcn_cs_step_f32(ctx.stream(0), dT.ptr, dR.ptr, dS.data_ptr() if fix else None, n, m, a, b, lo, hi, 0,
                                      FIX if fix else 0, out.ptr)
            ctx.sync()
            dR.check_unchanged("R")
            if not inplace:
                dT.check_unchanged("T")
            out.check_guards("out")
            got.append(out.values())
        what = (m, n, "coarse" if coarse else "free", "fix" if fix else "", "in place" if inplace else "", off)
        np.testing.assert_array_equal(_bits(got[0]), _bits(got[1]), err_msg=str(what))
        if fix:
            np.testing.assert_array_equal(_bits(got[0])[S == 0], _bits(R)[S == 0], err_msg=str(what))      # unclamped, as bits
        if coarse:
            np.testing.assert_array_equal(_bits(got[0]), _bits(twin), err_msg=str(what))
        else:
            ulps = np.abs(_ordered(got[0]) - _ordered(twin)).max()
            assert ulps <= 1, (what, int(ulps))
        want = ref.step(T, R, S, a, b, lo, hi, 0, fix, np.float64)
        # fp64: two roundings, of beta R and of the sum, each half an ulp of a magnitude below 16 here
        assert max(np.abs(T).max(), np.abs(R).max()) < 16 and np.abs(got[0] - want).max() <= 2.0 ** -19, what


def test_zero_rows_return_before_any_pointer_is_looked_at(ctx):
    lib, st = ctx.lib, ctx.stream(0)
    lib.mggcn_cs_residual_f32(st, None, None, None, 0, 41, 0, None, None, None)
    lib.mggcn_cs_step_f32(st, None, None, None, 0, 41, 0.8, 0.2, 0.0, 1.0, 0, FIX, None)
    lib.mggcn_cs_correct_f32(st, None, None, None, None, 0, 41, 0, None, 1.0, 1.0, AUTOSCALE | SET_LABELS, None)
    ctx.sync()
