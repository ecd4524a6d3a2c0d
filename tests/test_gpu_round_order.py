"""The order of a sweep plan's task table (MGGCN_SPMM_SORT_ROUNDS, csrc/plan_host.h) decides which tasks share a
launch, never what a task computes: C with the table in order of length is BITWISE the C of the table in LPT order, on
every kernel the sweep form launches, and both match the fp64-accumulated oracle at the bar of tests/test_gpu_kernels.py.

The matrices are sized for several full launch rounds on a whole MI355X with few rows: two rows per task
(MGGCN_SPMM_SWEEP_ROWS_PER_TASK=2) and 22 000 rows are 11 000 tasks, filled up to three rounds of 4096 -- tasks of one
row and tasks of two, the two classes the ordering is about -- in each of two column slices."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-4
N_ROWS, N_COLS = 22_000, 32_768


def rowwise_relerr(got, want):
    """as in tests/test_gpu_kernels.py: per row, the row scale floored at 1 % of the global scale"""
    want = np.asarray(want, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64)
    den = np.maximum(np.abs(want).max(axis=1), 1e-2 * np.abs(want).max()) + 1e-30
    return float((np.abs(got - want).max(axis=1) / den).max())


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


def _matrix(heavy):
    rng = np.random.default_rng(31 + heavy)
    lens = rng.integers(40, 121, size=N_ROWS)
    if heavy:
        lens[rng.choice(N_ROWS, size=6, replace=False)] = [3000, 1500, 900, 5000, 2100, 700]     # longer than 1.5 slices of 256: sliced
    ip = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    ix = rng.integers(0, N_COLS, size=int(ip[-1]), dtype=np.uint32)
    dv = rng.standard_normal(int(ip[-1])).astype(np.float32)
    return ip, ix, dv


@pytest.fixture(scope="module", params=[0, 1], ids=["short-rows", "with-sliced-rows"])
def case(request, pkg, oracle):
    """the matrix, and per width B, C0 and the oracle's A B (fp64 accumulation), computed once"""
    ip, ix, dv = _matrix(request.param)
    Ao = oracle.Csr(ip, ix, dv, N_COLS)
    rng = np.random.default_rng(77 + request.param)
    per_d = {}
    for d in (128, 96, 41):
        B = rng.standard_normal((N_COLS, d), dtype=np.float32)
        C0 = rng.standard_normal((N_ROWS, d), dtype=np.float32)
        per_d[d] = (B, C0, {beta: oracle.spmm(Ao, B, C0.copy(), alpha, beta, f64acc=True) for alpha, beta in ((1.0, 0.0), (0.5, 2.0))})
    return dict(heavy=bool(request.param), ip=ip, ix=ix, dv=dv, per_d=per_d)


# d = 128: the FAST pair kernel (power-of-two pitch); 96: the pair kernel's general instance; 41: the narrow kernel
@pytest.mark.parametrize("d", [128, 96, 41])
def test_round_order_moves_tasks_not_bits(pkg, oracle, ctx, case, monkeypatch, d):
    monkeypatch.setenv("MGGCN_SPMM_SWEEP_MIN_NNZ", "1")
    monkeypatch.setenv("MGGCN_SPMM_SWEEP_MIN_RUN_X10", "0")
    monkeypatch.setenv("MGGCN_SPMM_SWEEP_ROWS_PER_TASK", "2")
    monkeypatch.setenv("MGGCN_SPMM_SLICE_ROWS", "16384")          # two column slices: the second launches with beta = 1
    monkeypatch.setenv("MGGCN_SPMM_PERMUTE_COLUMNS", "0")
    monkeypatch.delenv("MGGCN_SPMM_ALGO", raising=False)
    monkeypatch.delenv("MGGCN_SPMM_XCD_COLUMNS", raising=False)
    B, C0, want = case["per_d"][d]
    Bd = pkg.dn_matrix.from_numpy(B)
    got, excess = {}, {}
    for knob in ("1", "0"):
        monkeypatch.setenv("MGGCN_SPMM_SORT_ROUNDS", knob)         # read once, when the plan is built
        A = pkg.csr_matrix(case["ip"], case["ix"], case["dv"], N_COLS)
        Cd = pkg.dn_matrix.from_numpy(C0)
        buf = pkg.get_matmul_buffer(ctx, A, Bd, Cd)
        text = buf.describe()
        assert buf.num_sweep_tasks() > 0 and "slices=2" in text, text
        assert ("form=sweep-narrow" in text) == (d == 41), text
        assert all(int(r) >= 3 for r in re.findall(r"rounds=(\d+)", text)), text       # several launches per slice to order
        assert (buf.num_split_rows() > 0) == case["heavy"]
        excess[knob] = [float(x) for x in re.findall(r"round_excess=([0-9.]+)", text)]
        assert len(excess[knob]) == 2 and text.rstrip().endswith(f"round_excess={excess[knob][-1]:.4f}"), text
        for alpha, beta in ((1.0, 0.0), (0.5, 2.0)):
            for flags in (0, 1):
                Cd = pkg.dn_matrix.from_numpy(C0)
                pkg.matmul(ctx, A, Bd, Cd, buf, alpha, beta, flags)
                ctx.sync()
                got[knob, beta, flags] = Cd.numpy()
    print(f"d={d} heavy={case['heavy']} round_excess sorted={excess['1']} unsorted={excess['0']}")
    assert all(s <= u for s, u in zip(excess["1"], excess["0"])), excess
    assert min(excess["0"]) > 0.0, excess                       # tasks of several lengths: there is something to order
    for beta in (0.0, 2.0):
        for flags in (0, 1):
            np.testing.assert_array_equal(got["1", beta, flags], got["0", beta, flags])
            ref = oracle.leaky_relu_forward(want[beta]) if flags else want[beta]
            err = rowwise_relerr(got["1", beta, flags], ref)
            print(f"  beta={beta} flags={flags} rowwise_relerr={err:.3e}")
            assert err <= TOL, (d, beta, flags, err)
