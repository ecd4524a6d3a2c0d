"""The row-value entry stream of the sweep SpMM (MGGCN_SPMM_ROW_VALUES, csrc/plan_host.h): when every stored value of a
row is the same, the plan drops the per-entry value and the kernels take the run's row value -- the same fmaf on the
same operands in the same order.  So C with the knob on is array_equal to C of the same call with the knob at 0 (only
the sign of an exactly-zero sum may differ, which array_equal ignores), on the FAST pair kernel (d = 128), the general
pair kernel (132), the narrow kernel (41, 16) and, through the stream expanded back on the device, the one-row-per-load
kernels (130, 67); both are within the row budget of tests/test_gpu_kernels.py of an fp64 reference.

The matrix: 40 rows x 9 000 columns = three tasks of sixteen rows and three column panels of 4 096; an empty row, a
one-entry row, odd and even run lengths, one row long enough to be sliced; one random value per row."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-4
N_ROWS, N_COLS = 40, 9_000
WIDTHS = (128, 132, 41, 16, 130, 67)
KNOBS = {"MGGCN_SPMM_SWEEP_MIN_NNZ": "1", "MGGCN_SPMM_SWEEP_MIN_RUN_X10": "0", "MGGCN_SPMM_PANEL_ROWS": "4096",
         "MGGCN_SPMM_PANEL_ROWS_NARROW": "4096", "MGGCN_SPMM_SWEEP_SPLIT": "256"}
LAYOUTS = {"plain": {"MGGCN_SPMM_PERMUTE_COLUMNS": "0"},
           "permuted": {"MGGCN_SPMM_PERMUTE_COLUMNS": "1"},
           "two-slices": {"MGGCN_SPMM_PERMUTE_COLUMNS": "0", "MGGCN_SPMM_SLICE_ROWS": "4608"}}


def rowwise_relerr(got, want):
    """as in tests/test_gpu_kernels.py: per row, the row scale floored at 1 % of the global scale"""
    want = np.asarray(want, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64)
    den = np.maximum(np.abs(want).max(axis=1), 1e-2 * np.abs(want).max()) + 1e-30
    return float((np.abs(got - want).max(axis=1) / den).max())


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


@pytest.fixture(scope="module")
def case(oracle):
    """the matrix, and per width B, C0 and the fp64 products, computed once"""
    rng = np.random.default_rng(2024)
    lens = rng.integers(2, 61, size=N_ROWS)
    lens[0], lens[1], lens[2], lens[3], lens[7] = 0, 1, 7, 8, 1200       # empty, one entry, odd, even, sliced (> 1.5 x 256)
    ip = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    ix = np.concatenate([np.sort(rng.choice(N_COLS, size=int(n), replace=False)) for n in lens]).astype(np.uint32)
    row_val = rng.standard_normal(N_ROWS).astype(np.float32)
    dv = np.repeat(row_val, lens).astype(np.float32)
    dense = np.zeros((N_ROWS, N_COLS), dtype=np.float64)
    for r in range(N_ROWS):
        dense[r, ix[ip[r]:ip[r + 1]]] = dv[ip[r]:ip[r + 1]]
    per_d = {}
    for d in WIDTHS:
        B = rng.standard_normal((N_COLS, d), dtype=np.float32)
        C0 = rng.standard_normal((N_ROWS, d), dtype=np.float32)
        AB = dense @ B.astype(np.float64)
        per_d[d] = (B, C0, {0.0: 0.5 * AB, 1.0: 0.5 * AB + C0.astype(np.float64)})
    return dict(ip=ip, ix=ix, dv=dv, per_d=per_d, oracle=oracle)


def _run(pkg, ctx, case, dv, d, monkeypatch, knob):
    """every (beta, activation) variant of alpha = 0.5 on a plan built with MGGCN_SPMM_ROW_VALUES = knob"""
    monkeypatch.setenv("MGGCN_SPMM_ROW_VALUES", knob)                 # read once, when the plan is built
    B, C0, _ = case["per_d"][d]
    A = pkg.csr_matrix(case["ip"], case["ix"], dv, N_COLS)
    Bd = pkg.dn_matrix.from_numpy(B)
    buf = pkg.get_matmul_buffer(ctx, A, Bd, pkg.dn_matrix.from_numpy(C0))
    text = buf.describe()
    assert buf.num_sweep_tasks() > 0 and ("form=sweep-narrow" in text) == (d <= 64), text
    got = {}
    for beta in (0.0, 1.0):
        for flags in (0, 1):
            Cd = pkg.dn_matrix.from_numpy(C0 if beta else np.full_like(C0, np.nan))     # beta = 0 never reads C
            pkg.matmul(ctx, A, Bd, Cd, buf, 0.5, beta, flags)
            ctx.sync()
            got[beta, flags] = Cd.numpy()
    return text, got


def _check(case, d, got):
    _, _, want = case["per_d"][d]
    for (beta, flags), c in got.items():
        ref = case["oracle"].leaky_relu_forward(want[beta]) if flags else want[beta]
        err = rowwise_relerr(c, ref)
        print(f"  d={d} beta={beta} flags={flags} rowwise_relerr={err:.3e}")
        assert err <= TOL, (d, beta, flags, err)


def _setup(monkeypatch, layout):
    for k, v in {**KNOBS, **LAYOUTS[layout]}.items():
        monkeypatch.setenv(k, v)
    for k in ("MGGCN_SPMM_ALGO", "MGGCN_SPMM_XCD_COLUMNS") + (("MGGCN_SPMM_SLICE_ROWS",) if layout != "two-slices" else ()):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("d", WIDTHS)
def test_row_value_stream_computes_what_the_entry_stream_computes(pkg, ctx, case, monkeypatch, d, layout):
    _setup(monkeypatch, layout)
    text_row, got_row = _run(pkg, ctx, case, case["dv"], d, monkeypatch, "1")
    text_ent, got_ent = _run(pkg, ctx, case, case["dv"], d, monkeypatch, "0")
    n_slices = 2 if layout == "two-slices" else 1
    assert re.findall(r"values=(\w+)", text_row) == ["row"] * n_slices, text_row
    assert re.findall(r"values=(\w+)", text_ent) == ["entry"] * n_slices, text_ent
    assert all(int(n) > 0 for n in re.findall(r" split_rows=(\d+)", text_row)), text_row          # the long row is sliced
    assert ("permuted=1" in text_row) == (layout == "permuted"), text_row
    # the plan around the stream is the same one: tasks, rounds, padded entries, slots, round_excess
    assert re.sub(r"values=\w+", "", text_row.split("|", 1)[1]) == re.sub(r"values=\w+", "", text_ent.split("|", 1)[1])
    for key in got_row:
        assert not np.isnan(got_row[key]).any(), key
        np.testing.assert_array_equal(got_row[key], got_ent[key], err_msg=str((d, layout, key)))
    _check(case, d, got_row)
    _check(case, d, got_ent)


@pytest.mark.parametrize("d", [128, 41])
def test_one_changed_value_keeps_the_entry_stream(pkg, ctx, case, monkeypatch, d):
    _setup(monkeypatch, "plain")
    dv = case["dv"].copy()
    e = int(case["ip"][3]) + 2                                     # one value of the eight-entry row
    delta = np.float32(0.25)
    dv[e] += delta
    monkeypatch.delenv("MGGCN_SPMM_ROW_VALUES", raising=False)     # the default: row values where the matrix allows
    A = pkg.csr_matrix(case["ip"], case["ix"], case["dv"], N_COLS)
    B, C0, want = case["per_d"][d]
    Bd = pkg.dn_matrix.from_numpy(B)
    assert "values=row" in pkg.get_matmul_buffer(ctx, A, Bd, pkg.dn_matrix.from_numpy(C0)).describe()
    text, got = _run(pkg, ctx, case, dv, d, monkeypatch, "1")
    assert re.findall(r"values=(\w+)", text) == ["entry"], text
    fix = np.zeros_like(want[0.0])
    fix[3] = 0.5 * float(delta) * B[case["ix"][e]].astype(np.float64)
    for (beta, flags), c in got.items():
        ref = want[beta] + fix
        ref = case["oracle"].leaky_relu_forward(ref) if flags else ref
        assert rowwise_relerr(c, ref) <= TOL, (d, beta, flags)


@pytest.mark.parametrize("d", [128, 41])
def test_bf16_operand_on_a_row_value_plan(pkg, ctx, case, monkeypatch, d):
    """mggcn_spmm_csr_bf16 runs the row-value instances too (the plan grows by nothing but its bf16 scratch): bit for bit
    the entry stream's result"""
    torch = pytest.importorskip("torch")
    from bf16_ref import bf16_bits
    _setup(monkeypatch, "plain")
    B, C0, _ = case["per_d"][d]
    B16 = torch.from_numpy(bf16_bits(B).view(np.int16)).cuda()
    got = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("MGGCN_SPMM_ROW_VALUES", knob)
        A = pkg.csr_matrix(case["ip"], case["ix"], case["dv"], N_COLS)
        plan = pkg.ops.spmm_plan_for(ctx, A, 128, d if d <= 64 else 0)
        assert ("values=row" if knob == "1" else "values=entry") in plan.describe(), plan.describe()
        for beta in (0.0, 1.0):
            Cd = pkg.dn_matrix.from_numpy(C0 if beta else np.full_like(C0, np.nan))
            pkg.ops.spmm_bf16(ctx, A, B16, Cd, plan, 0.5, beta, 1, 0.01)
            ctx.sync()
            got[knob, beta] = Cd.numpy()
    for beta in (0.0, 1.0):
        assert not np.isnan(got["1", beta]).any()
        np.testing.assert_array_equal(got["1", beta], got["0", beta])
