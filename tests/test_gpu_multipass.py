"""The kernels of elementwise.hip beyond one pass of their grid, judged element by element and row by row.

Every kernel there is a grid-stride loop under a capped grid.  The other kernel tests stay at sizes where a thread
handles one item; here every size is two full passes and a ragged third, derived from the caps below.  A changed cap
makes `_three_passes` fail (a stale constant) instead of silently losing the coverage.

Caps assumed (a pass = what the capped grid covers in one trip of the loop):
  stream_grid (common.h: kNumCU * 8 = 2048 workgroups of 256 threads)            524 288 threads
    map1 / map2 (scalar), broadcast_rows, scale_rows, subtract_rows_exp, is_equal,
    adam_final, adam_fused                                                       524 288 elements
    map1_vec4 / map2_vec4                                                        524 288 float4 = 2 097 152 floats
    index_log_rows, add_indexed_rows (a thread per row)                          524 288 rows
    max_rows, max_row_indices (a wave per row)                                   8 192 rows
  abssum (kAsumBlocks = 1024 workgroups)                                         262 144 elements
  gather_rows (kNumCU * 16 = 4096 workgroups of 4 waves, a wave per index)       16 384 indices
  convert_f32_bf16 (kNumCU * 16 = 4096 workgroups)                               1 048 576 float4 groups / elements
  fused loss, m <= 64 (softmax_xent_rows16_kernel<KE, 4>: a 16-lane group per row, 4 row slots per group,
    slot q of a pass = first row + q * 32 768)                                   131 072 rows
  fused loss, m > 64 (softmax_xent_fused_kernel<K, R>: a wave per row, slot stride 8 192,
    R = 4 / 2 / 1 / 1 for m <= 128 / 256 / 512 / 1024)                           32 768 / 16 384 / 8 192 / 8 192 rows

References are numpy in fp64 (fp32 where a kernel rounds once and must be bit-exact), written here.

Worst errors of the first run on an MI355X, every test prints its own (pytest -s); the bar in brackets:
  leaky ReLU fwd / bwd, scale_mat, broadcast_rows, is_equal, max_rows, max_row_indices,
  gather_rows, convert_f32_bf16, add_indexed_rows                  bit-exact
  axpy / axpby / aaxpby, float4 and scalar                         6.0e-8 / 1.1e-7 / 1.2e-7 of |a||x| + |b||y|  [1e-6]
  scale_rows                                                       6.0e-8 relative                              [1e-6]
  subtract_rows_exp (arguments in [-80, 0])                        0.83 ulp                                     [8 ulp]
  index_log_rows (arguments in (e^-20, 1])                         2.15 ulp                                     [8 ulp]
  abssum, 536 633 / 100 elements                                   3.4e-9 / 3.1e-8 of sum|x|                    [1e-5]
  adam_final                                                       2.9e-7 of max(|p|, lr)                       [1e-5]
  adam_fused, three steps (param, grad, m, v)                      4.4e-6 of max(|.|, lr)                       [1e-5]
  fused loss, worst row in units of grad_scale * the row's largest probability                                  [1e-4]
    rows16 KE = 1 (m = 1, 16) / 2 (17) / 3 (41, 48) / 4 (64)       4.1e-7 / 3.6e-7 / 1.7e-6 / 8.3e-7
    wave per row K = 2 (65, 128) / 4 (129, 256) / 8 (257, 512)     3.2e-6 / 3.6e-6 / 7.9e-6
    wave per row K = 16 (513, 1000, 1024)                          1.8e-5, 2.5e-5, 2.9e-5
    cold rows and -inf entries (m = 41 ... 1024)                   5.6e-7
    loss sum                                                       1.1e-7 relative                              [1e-4]
  Above 1e-5 at K = 16 because of the unit, not the kernel: the label's entry is p_y - 1, rounded to fp32 next to 1, an
  absolute error of up to 2^-25 = 3.0e-8 whatever p_y is, and a row of m classes can have a largest probability as
  small as 1 / m.  2^-25 * 1024 = 3.1e-5 is the worst any correctly rounding fp32 kernel can show at m = 1024 (an fp32
  numpy restatement of the same rows shows the same 2.9e-5), a third of the bar.
"""
import numpy as np
import pytest

from guarded import Guarded
from test_gpu_layouts import _convert_input

pytestmark = pytest.mark.gpu

# ---- the caps (see the module docstring) ------------------------------------------------------------------------------
STREAM_THREADS = 256 * 8 * 256          # common.h stream_grid: cap = kNumCU * 8 workgroups, 256 threads each
VEC4_FLOATS = 4 * STREAM_THREADS        # elementwise.hip launch_map1 / launch_map2: stream_grid(size / 4)
WAVE_ROWS = STREAM_THREADS // 64        # mggcn_max_rows_f32 / mggcn_max_row_indices_f32: stream_grid(n_rows * 64)
ABSSUM_ELEMS = 1024 * 256               # elementwise.hip kAsumBlocks
GATHER_ROWS = 256 * 16 * 4              # mggcn_gather_rows_f32: min((n + 3) / 4, kNumCU * 16) workgroups of 4 waves
CONVERT_ITEMS = 256 * 16 * 256          # mggcn_convert_f32_bf16: min(ceil(work / 256), kNumCU * 16) workgroups
XENT16_SLOT = STREAM_THREADS // 16      # mggcn_softmax_xent_fused_from_f32, m <= 64: stream_grid(n_rows * 16), R = 4
XENT_SLOT = STREAM_THREADS // 64        # the same, m > 64: stream_grid(n_rows * 64)


def _xent_geometry(m):
    """(slot stride in rows, rows in flight R) of the fused-loss instance that serves m classes when the grid is capped"""
    if m <= 64:
        return XENT16_SLOT, 4
    return XENT_SLOT, 4 if m <= 128 else 2 if m <= 256 else 1


def _three_passes(items, cap, what):
    """two full passes of the capped grid and a ragged third"""
    rest = items - 2 * cap
    assert 0 < rest < cap, f"{what}: {items} items are not 2 passes of {cap} and a partial third"
    assert rest % 4 != 0, f"{what}: the last pass ({rest} items) is not ragged"
    return items


RAGGED = 12_345                         # odd: not a multiple of 4, 16, 64 or 256
FLAT_SCALAR = _three_passes(2 * STREAM_THREADS + RAGGED, STREAM_THREADS, "scalar maps")          # odd size: map1 / map2
FLAT_VEC4 = 4 * _three_passes(2 * STREAM_THREADS + RAGGED, STREAM_THREADS, "float4 maps")         # % 4 == 0, aligned
CHUNK = 400_000                         # below one pass of either form, a multiple of 4


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


def _torch():
    import torch
    return torch


def _dev(a):
    torch = _torch()
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _f32(x):
    return float(np.float32(x))


def _first_bad(mask):
    bad = np.flatnonzero(np.asarray(mask).reshape(-1))
    return f"{bad.size} bad, first at flat index {int(bad[0])}" if bad.size else "none"


def _assert_bits_equal(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gb = got.view(np.uint32 if got.dtype.itemsize == 4 else np.uint16)
    wb = want.view(np.uint32 if want.dtype.itemsize == 4 else np.uint16)
    neq = gb != wb
    if neq.any():
        i = int(np.flatnonzero(neq.reshape(-1))[0])
        raise AssertionError(f"{what}: {int(neq.sum())} element(s) differ; first at flat index {i} "
                             f"(got {got.reshape(-1)[i]!r}, want {want.reshape(-1)[i]!r})")


def _chunks(total, step):
    return [(a, min(step, total - a)) for a in range(0, total, step)]


# ---- the flat maps -----------------------------------------------------------------------------------------------------
SLOPE, ALPHA, BETA = np.float32(0.03), np.float32(0.7), np.float32(-1.3)
FLAT_OPS = {    # name: (call(lib, stream, x_ptr, y_ptr, out_ptr, n), fp32 reference or None, fp64 reference, its error budget)
    "leaky_relu_forward": (lambda L, s, x, y, o, n: L.mggcn_leaky_relu_forward_f32(s, x, o, n, float(SLOPE)),
                           lambda x, y: np.where(x > SLOPE * x, x, SLOPE * x), None, None),
    "leaky_relu_backward": (lambda L, s, x, y, o, n: L.mggcn_leaky_relu_backward_f32(s, x, y, o, n, float(SLOPE)),
                            lambda x, y: np.where(x > 0, y, SLOPE * y), None, None),
    "scale_mat": (lambda L, s, x, y, o, n: (L.mggcn_memcpy_d2d(o, x, 4 * n, s), L.mggcn_scale_mat_f32(s, o, float(ALPHA), n)),
                  lambda x, y: x * ALPHA, None, None),
    # B = f(A, B) in place: out starts as a copy of y
    "axpy": (lambda L, s, x, y, o, n: (L.mggcn_memcpy_d2d(o, y, 4 * n, s), L.mggcn_axpy_f32(s, x, o, float(ALPHA), n)),
             None, lambda x, y: float(ALPHA) * x + y, lambda x, y: abs(float(ALPHA)) * np.abs(x) + np.abs(y)),
    "axpby": (lambda L, s, x, y, o, n: (L.mggcn_memcpy_d2d(o, y, 4 * n, s), L.mggcn_axpby_f32(s, x, o, float(ALPHA), float(BETA), n)),
              None, lambda x, y: float(ALPHA) * x + float(BETA) * y, lambda x, y: abs(float(ALPHA)) * np.abs(x) + abs(float(BETA)) * np.abs(y)),
    "aaxpby": (lambda L, s, x, y, o, n: (L.mggcn_memcpy_d2d(o, y, 4 * n, s), L.mggcn_aaxpby_f32(s, x, o, float(ALPHA), float(BETA), n)),
               None, lambda x, y: float(ALPHA) * x * x + float(BETA) * y, lambda x, y: abs(float(ALPHA)) * x * x + abs(float(BETA)) * np.abs(y)),
}


@pytest.mark.parametrize("form", ["float4", "scalar"])
@pytest.mark.parametrize("op", list(FLAT_OPS))
def test_flat_maps_three_passes(ctx, op, form):
    """leaky ReLU forward / backward and scale_mat bit-exact against numpy fp32; axpy / axpby / aaxpby per element against
    fp64 at 1e-6 of |a||x| + |b||y| (the budget of test_flat_maps_on_offset_pointers, per element instead of per buffer)
    and bit for bit equal to the same entry point run chunk by chunk, every chunk below one pass"""
    torch = _torch()
    call, ref32, ref64, budget = FLAT_OPS[op]
    n = FLAT_VEC4 if form == "float4" else FLAT_SCALAR
    rng = np.random.default_rng(len(op) + n % 1000)
    x = rng.standard_normal((1, n), dtype=np.float32)
    x[0, ::1001] = 0.0                                          # x > 0 is strict
    y = rng.standard_normal((1, n), dtype=np.float32)
    X, Y = Guarded(1, n, n, 0, logical=x), Guarded(1, n, n, 0, logical=y)
    O = Guarded(1, n, n, 0, output=True)
    torch.cuda.synchronize()
    call(ctx.lib, ctx.stream(0), X.ptr, Y.ptr, O.ptr, n)
    ctx.sync()
    b = O.bits()
    O.check_guards(f"{op} {form}", b)
    X.check_unchanged(f"{op} {form} x"); Y.check_unchanged(f"{op} {form} y")
    got = O.values(b)
    if ref32 is not None:
        _assert_bits_equal(got, ref32(x, y).astype(np.float32), f"{op} {form} vs numpy fp32")
        return
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    err = np.abs(got.astype(np.float64) - ref64(x64, y64)) / budget(x64, y64)
    print(f"\n[multipass] {op} {form}: worst error {err.max():.3e} of |a||x| + |b||y| (bar 1e-6)")
    assert err.max() <= 1e-6, f"{op} {form}: {_first_bad(err > 1e-6)}"
    P = Guarded(1, n, n, 0, output=True)                        # the same call, chunk by chunk
    torch.cuda.synchronize()
    for a, k in _chunks(n, CHUNK):
        call(ctx.lib, ctx.stream(0), X.ptr + 4 * a, Y.ptr + 4 * a, P.ptr + 4 * a, k)
    ctx.sync()
    _assert_bits_equal(got, P.values(), f"{op} {form}: one call vs chunks of {CHUNK}")


# ---- the row-indexed streaming kernels ---------------------------------------------------------------------------------
ROW_M = 41
ROW_N = 25_901                                                  # 25 901 x 41 = 2 x 524 288 + 13 365
_three_passes(ROW_N * ROW_M, STREAM_THREADS, "row-indexed streaming kernels")
ROW_CHUNK = 12_000                                              # rows: 492 000 elements, below one pass, a multiple of 4


def test_broadcast_rows_three_passes(pkg, ctx):
    rng = np.random.default_rng(11)
    x = rng.standard_normal((ROW_N, ROW_M), dtype=np.float32)
    row = rng.standard_normal((1, ROW_M), dtype=np.float32)
    R, M = pkg.dn_matrix.from_numpy(row), pkg.dn_matrix.from_numpy(x)
    pkg.ops.broadcast_rows(ctx, R, M, False); ctx.sync()
    _assert_bits_equal(M.numpy(), x + row, "broadcast_rows, accumulate")
    pkg.ops.broadcast_rows(ctx, R, M, True); ctx.sync()
    _assert_bits_equal(M.numpy(), np.broadcast_to(row, x.shape), "broadcast_rows, discard")


def test_scale_rows_three_passes(ctx):
    """mat[i] /= scalar[i / m]: per element against fp64 at 1e-6 (one division), and equal to the chunked calls"""
    torch = _torch()
    rng = np.random.default_rng(12)
    x = rng.standard_normal((ROW_N, ROW_M), dtype=np.float32)
    s = (rng.uniform(0.5, 40.0, (ROW_N, 1)) * rng.choice([-1.0, 1.0], (ROW_N, 1))).astype(np.float32)
    S = _dev(s)
    A, B = Guarded(ROW_N, ROW_M, ROW_M, 0, logical=x, output=True), Guarded(ROW_N, ROW_M, ROW_M, 0, logical=x, output=True)
    torch.cuda.synchronize()
    ctx.lib.mggcn_scale_rows_f32(ctx.stream(0), A.ptr, S.data_ptr(), ROW_N * ROW_M, ROW_M)
    for r, k in _chunks(ROW_N, ROW_CHUNK):
        ctx.lib.mggcn_scale_rows_f32(ctx.stream(0), B.ptr + 4 * r * ROW_M, S.data_ptr() + 4 * r, k * ROW_M, ROW_M)
    ctx.sync()
    b = A.bits()
    A.check_guards("scale_rows", b)
    got = A.values(b)
    want = x.astype(np.float64) / s.astype(np.float64)
    err = np.abs(got - want) / np.abs(want).clip(1e-30)
    print(f"\n[multipass] scale_rows: worst relative error {err.max():.3e} (bar 1e-6)")
    assert err.max() <= 1e-6, _first_bad(err > 1e-6)
    _assert_bits_equal(got, B.values(), "scale_rows: one call vs chunks")
    np.testing.assert_array_equal(S.cpu().numpy(), s)


def _ulps(got, want64):
    """|got - want| in units of the spacing of fp32 at the fp64 value"""
    w32 = want64.astype(np.float32)
    return np.abs(got.astype(np.float64) - want64) / np.spacing(np.abs(w32)).astype(np.float64)


# numpy's own fp32 exp / log are off by up to 2.4 / 3.4 ulp on these ranges; the bar leaves a factor 2-3 above that for a
# different but sound device function.  First run on the device: expf 0.83 ulp, logf 2.15 ulp.
ULP_BAR = 8.0


def test_subtract_rows_exp_three_passes(ctx):
    """out = exp(mat - scalar[row]), arguments in [-80, 0]: the argument formed in fp32 like the kernel's, exp of it in
    fp64, error counted in ulps of the fp32 result; and equal to the chunked calls"""
    torch = _torch()
    rng = np.random.default_rng(13)
    s = (rng.standard_normal((ROW_N, 1)) * 4).astype(np.float32)
    x = (s + rng.uniform(-80.0, 0.0, (ROW_N, ROW_M))).astype(np.float32)
    x[np.arange(ROW_N), rng.integers(0, ROW_M, ROW_N)] = s[:, 0]            # the row maximum itself: argument 0
    arg = x - s                                                               # fp32, one subtraction
    assert arg.min() >= -80.01 and arg.max() <= 0.01 and (arg == 0).sum() >= ROW_N
    X, S = Guarded(ROW_N, ROW_M, ROW_M, 0, logical=x), _dev(s)
    A, B = Guarded(ROW_N, ROW_M, ROW_M, 0, output=True), Guarded(ROW_N, ROW_M, ROW_M, 0, output=True)
    torch.cuda.synchronize()
    ctx.lib.mggcn_subtract_rows_exp_f32(ctx.stream(0), X.ptr, S.data_ptr(), A.ptr, ROW_N * ROW_M, ROW_M)
    for r, k in _chunks(ROW_N, ROW_CHUNK):
        off = 4 * r * ROW_M
        ctx.lib.mggcn_subtract_rows_exp_f32(ctx.stream(0), X.ptr + off, S.data_ptr() + 4 * r, B.ptr + off, k * ROW_M, ROW_M)
    ctx.sync()
    b = A.bits()
    A.check_guards("subtract_rows_exp", b)
    X.check_unchanged("subtract_rows_exp input")
    got = A.values(b)
    u = _ulps(got, np.exp(arg.astype(np.float64)))
    print(f"\n[multipass] subtract_rows_exp: worst error {u.max():.2f} ulp (bar {ULP_BAR})")
    assert u.max() <= ULP_BAR, _first_bad(u > ULP_BAR)
    _assert_bits_equal(got, B.values(), "subtract_rows_exp: one call vs chunks")


IDX_M = 5
IDX_N = _three_passes(2 * STREAM_THREADS + RAGGED, STREAM_THREADS, "index_log_rows / add_indexed_rows")
IDX_CHUNK = 400_000                                             # rows, below one pass; 400 000 x 5 is a multiple of 4


def test_index_log_rows_three_passes(ctx):
    """values[r] = log(mat[r, idx[r]]), arguments in (e^-20, 1]: ulps of the fp32 result against fp64 log of the stored
    value; and equal to the chunked calls"""
    torch = _torch()
    rng = np.random.default_rng(14)
    x = np.exp(rng.uniform(-20.0, 0.0, (IDX_N, IDX_M))).astype(np.float32)
    idx = rng.integers(0, IDX_M, (IDX_N, 1)).astype(np.int32)
    idx[[0, -1]] = [[IDX_M - 1], [IDX_M - 1]]                   # the very last element of the matrix is read
    x[::997, :] = 1.0                                           # log 1 = 0 exactly
    X, I = _dev(x), _dev(idx)
    A, B = Guarded(IDX_N, 1, 1, 0, output=True), Guarded(IDX_N, 1, 1, 0, output=True)
    torch.cuda.synchronize()
    ctx.lib.mggcn_index_log_rows_f32(ctx.stream(0), X.data_ptr(), I.data_ptr(), A.ptr, IDX_N * IDX_M, IDX_M)
    for r, k in _chunks(IDX_N, IDX_CHUNK):
        ctx.lib.mggcn_index_log_rows_f32(ctx.stream(0), X.data_ptr() + 4 * r * IDX_M, I.data_ptr() + 4 * r, B.ptr + 4 * r,
                                         k * IDX_M, IDX_M)
    ctx.sync()
    b = A.bits()
    A.check_guards("index_log_rows", b)
    got = A.values(b).reshape(-1)
    picked = x[np.arange(IDX_N), idx[:, 0]]
    want = np.log(picked.astype(np.float64))
    assert (got[picked == 1.0] == 0.0).all()
    nz = want != 0
    u = _ulps(got[nz], want[nz])
    print(f"\n[multipass] index_log_rows: worst error {u.max():.2f} ulp (bar {ULP_BAR})")
    assert u.max() <= ULP_BAR, _first_bad(u > ULP_BAR)
    _assert_bits_equal(got, B.values().reshape(-1), "index_log_rows: one call vs chunks")


def test_add_indexed_rows_three_passes(ctx):
    torch = _torch()
    rng = np.random.default_rng(15)
    x = rng.standard_normal((IDX_N, IDX_M), dtype=np.float32)
    idx = rng.integers(0, IDX_M, (IDX_N, 1)).astype(np.int32)
    idx[[0, -1]] = [[0], [IDX_M - 1]]
    A, I = Guarded(IDX_N, IDX_M, IDX_M, 0, logical=x, output=True), _dev(idx)
    torch.cuda.synchronize()
    ctx.lib.mggcn_add_indexed_rows_f32(ctx.stream(0), A.ptr, I.data_ptr(), -1.0, IDX_N * IDX_M, IDX_M)
    ctx.sync()
    b = A.bits()
    A.check_guards("add_indexed_rows", b)
    want = x.copy()
    want[np.arange(IDX_N), idx[:, 0]] += np.float32(-1.0)
    _assert_bits_equal(A.values(b), want, "add_indexed_rows")


def test_is_equal_three_passes(ctx):
    torch = _torch()
    n = FLAT_SCALAR
    rng = np.random.default_rng(16)
    a = rng.integers(0, 3, n).astype(np.int32)
    b_ = rng.integers(0, 3, n).astype(np.int32)
    A, B = _dev(a), _dev(b_)
    O = Guarded(1, n, n, 0, output=True)
    torch.cuda.synchronize()
    ctx.lib.mggcn_is_equal_i32(ctx.stream(0), A.data_ptr(), B.data_ptr(), O.ptr, n)
    ctx.sync()
    bits = O.bits()
    O.check_guards("is_equal", bits)
    _assert_bits_equal(O.values(bits).reshape(-1), (a == b_).astype(np.float32), "is_equal")


# ---- a wave per row ----------------------------------------------------------------------------------------------------
MAX_N = _three_passes(2 * WAVE_ROWS + 1_237, WAVE_ROWS, "max_rows / max_row_indices")


@pytest.mark.parametrize("m", [41, 130])
def test_max_rows_and_indices_three_passes(pkg, ctx, m):
    """row maximum and its FIRST column, bit-exact; exact ties planted in rows of the first pass, the middle pass and the
    ragged last pass (full ties, and a two-way tie whose later column a "last maximum wins" kernel would report)"""
    n = MAX_N
    rng = np.random.default_rng(m)
    x = (rng.standard_normal((n, m)) * 3).astype(np.float32)
    for p in range(3):
        for r in (p * WAVE_ROWS, p * WAVE_ROWS + 617, min((p + 1) * WAVE_ROWS, n) - 1):
            x[r, :] = np.float32(0.375 + p)                                     # full tie -> column 0
            x[r - 1 if r % WAVE_ROWS else r + 1, [3, m - 2]] = 40.0             # two-way tie -> column 3
    x[n - 2, [m - 1, 65 % m]] = 50.0                                            # a tie across the lanes' second trip
    X = pkg.dn_matrix.from_numpy(x)
    mx, ix = pkg.dn_matrix(n, 1), pkg.dn_matrix(n, 1, dtype=np.int32)
    pkg.ops.max_rows(ctx, X, mx)
    pkg.ops.max_row_indices(ctx, X, ix)
    ctx.sync()
    _assert_bits_equal(mx.numpy().reshape(-1), x.max(axis=1), f"max_rows m={m}")
    got, want = ix.numpy().reshape(-1), x.argmax(axis=1).astype(np.int32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"max_row_indices m={m}: {bad.size} row(s) wrong; first row {bad[0]} (pass {bad[0] // WAVE_ROWS}): "
                           f"got {got[bad[0]]}, want {want[bad[0]]}")


def test_all_minus_inf_row_reports_index_zero(pkg, ctx):
    """the documented degenerate row (elementwise.hip, max_row_indices_kernel: the reference's strict `<` never fires)"""
    x = np.random.default_rng(3).standard_normal((300, 41)).astype(np.float32)
    x[[0, 77, 299], :] = -np.inf
    X, ix = pkg.dn_matrix.from_numpy(x), pkg.dn_matrix(300, 1, dtype=np.int32)
    pkg.ops.max_row_indices(ctx, X, ix); ctx.sync()
    want = x.argmax(axis=1)
    want[[0, 77, 299]] = 0
    np.testing.assert_array_equal(ix.numpy().reshape(-1), want)


@pytest.mark.parametrize("d", [128, 41])
def test_gather_rows_three_passes(ctx, d):
    torch = _torch()
    n_idx = _three_passes(2 * GATHER_ROWS + 1_237, GATHER_ROWS, "gather_rows")
    n_src = 5_000
    rng = np.random.default_rng(d)
    X = rng.standard_normal((n_src, d), dtype=np.float32)
    idx = rng.integers(0, n_src, n_idx).astype(np.uint32)
    idx[[0, 1, -1]] = [n_src - 1, 0, n_src - 1]
    src, dst = Guarded(n_src, d, d, 0, logical=X), Guarded(n_idx, d, d, 0, output=True)
    I = _dev(idx.view(np.int32))
    torch.cuda.synchronize()
    ctx.lib.mggcn_gather_rows_f32(ctx.stream(0), src.ptr, d, I.data_ptr(), n_idx, d, dst.ptr, d)
    ctx.sync()
    b = dst.bits()
    dst.check_guards("gather_rows dst", b)
    src.check_unchanged("gather_rows src")
    _assert_bits_equal(dst.logical_bits(b), X.view(np.uint32)[idx], f"gather_rows d={d}")


@pytest.mark.parametrize("m", [44, 41])             # float4 form (11 groups per row) and scalar form
def test_convert_f32_bf16_three_passes(ctx, m):
    torch = _torch()
    per_row = m // 4 if m % 4 == 0 else m
    n = 2 * CONVERT_ITEMS // per_row + 1_001
    _three_passes(n * per_row, CONVERT_ITEMS, f"convert_f32_bf16 m={m}")
    x = _convert_input(n, m, seed=m)                # the specials sit at both ends of the buffer
    src, dst = Guarded(n, m, m, 0, logical=x), Guarded(n, m, m, 0, output=True, bf16=True)
    torch.cuda.synchronize()
    ctx.lib.mggcn_convert_f32_bf16(ctx.stream(0), src.ptr, m, dst.ptr, m, n, m)
    ctx.sync()
    b = dst.bits()
    dst.check_guards("convert dst", b)
    src.check_unchanged("convert src")
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    _assert_bits_equal(dst.logical_bits(b), want, f"convert_f32_bf16 m={m}")


@pytest.mark.parametrize("n", [_three_passes(2 * ABSSUM_ELEMS + RAGGED, ABSSUM_ELEMS, "abssum"), 100])
def test_abssum_three_passes(ctx, n):
    torch = _torch()
    x = np.random.default_rng(n % 1000).standard_normal(n).astype(np.float32)
    X = _dev(x)
    out = []
    for _ in range(3):
        s = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.lib.mggcn_abssum_f32(ctx.stream(0), X.data_ptr(), n, s.data_ptr()); ctx.sync()
        out.append(s.cpu().numpy().copy())
    want = np.abs(x.astype(np.float64)).sum()
    print(f"\n[multipass] abssum n={n}: error {abs(float(out[0][0]) - want) / want:.3e} of sum|x| (bar 1e-5)")
    assert abs(float(out[0][0]) - want) <= 1e-5 * want
    for o in out[1:]:
        _assert_bits_equal(o, out[0], f"abssum n={n}: run to run")


# ---- Adam --------------------------------------------------------------------------------------------------------------
ADAM_N = _three_passes(2 * STREAM_THREADS + 777, STREAM_THREADS, "adam_final / adam_fused")
LR, B1, B2, WD, EPS = 1e-2, 0.9, 0.999, 5e-4, 1e-8


def _adam64(p, g, m, v, step, wd):
    """one Adam step of adam_fused_kernel in fp64, over the fp32 constants the kernel gets"""
    lr, b1, b2, eps, wd = (float(np.float32(t)) for t in (LR, B1, B2, EPS, wd))
    c1, c2 = _f32(1 - B1 ** step), _f32(1 - B2 ** step)
    g = wd * p + g
    m = (1.0 - b1) * g + b1 * m
    v = (1.0 - b2) * g * g + b2 * v
    return p - (lr / c1) * m / (np.sqrt(v / c2) + eps), g, m, v


def test_adam_final_three_passes(ctx):
    """param -= lr / c1 * m / (sqrt(v / c2) + eps): per element against fp64 at 1e-5 of max(|param|, lr), and equal to
    the chunked calls.  The moments are those of an Adam run (m / c1 ~ g, v / c2 ~ g^2 for a gradient g), so the update
    is of the order of lr: with unrelated m and v it can be as large as the parameter, the difference cancels, and no
    fp32 evaluation meets a bar relative to the result (1.7e-5 with such inputs on the first run: the test's fault)."""
    torch = _torch()
    n = ADAM_N
    rng = np.random.default_rng(21)
    p = rng.standard_normal((1, n), dtype=np.float32)
    c1, c2 = _f32(1 - B1 ** 2), _f32(1 - B2 ** 2)
    g = rng.standard_normal((1, n))
    g[0, ::1013] = 0.0                                           # m = v = 0: the update is 0 / eps = 0
    m = (c1 * g * rng.uniform(0.5, 1.5, (1, n))).astype(np.float32)
    v = (c2 * g * g * rng.uniform(0.5, 2.0, (1, n))).astype(np.float32)
    assert (np.abs(m / c1) <= 3.0 * (np.sqrt(v / c2) + EPS)).all()          # |update| <= 3 lr
    M, V = _dev(m), _dev(v)
    A, B = Guarded(1, n, n, 0, logical=p, output=True), Guarded(1, n, n, 0, logical=p, output=True)
    torch.cuda.synchronize()
    ctx.lib.mggcn_adam_final_f32(ctx.stream(0), A.ptr, M.data_ptr(), V.data_ptr(), LR, c1, c2, EPS, n)
    for a, k in _chunks(n, CHUNK):
        ctx.lib.mggcn_adam_final_f32(ctx.stream(0), B.ptr + 4 * a, M.data_ptr() + 4 * a, V.data_ptr() + 4 * a, LR, c1, c2, EPS, k)
    ctx.sync()
    b = A.bits()
    A.check_guards("adam_final", b)
    got = A.values(b)
    p64, m64, v64 = (t.astype(np.float64) for t in (p, m, v))
    want = p64 - (_f32(LR) / c1) * m64 / (np.sqrt(v64 / c2) + _f32(EPS))
    err = np.abs(got - want) / np.maximum(np.abs(want), LR)
    print(f"\n[multipass] adam_final: worst error {err.max():.3e} of max(|p|, lr) (bar 1e-5)")
    assert err.max() <= 1e-5, _first_bad(err > 1e-5)
    _assert_bits_equal(got, B.values(), "adam_final: one call vs chunks")


def test_adam_fused_three_passes_and_adam_multi(pkg, ctx):
    """adam_fused on one tensor of three grid passes over three steps: every element of param, grad, m, v against an fp64
    restatement (1e-5 of max(|.|, lr), the bar of test_adam_fused_equals_chain_equals_oracle, per element) and bit for bit
    equal to chunked calls; adam_multi with that tensor between small ones in the table (its ~1 000 blocks in the middle
    of the first_block search) bitwise equal to adam_fused per tensor."""
    rng = np.random.default_rng(22)
    shapes = [(3, 1), (1025, 1), (ADAM_N, 1), (128, 41), (1, 41)]
    wds = [WD, WD, WD, WD, 0.0]
    big = 2
    mk = lambda a: pkg.dn_matrix.from_numpy(a.copy())
    P0 = [rng.standard_normal(s, dtype=np.float32) for s in shapes]
    sets = []                                                    # 0: adam_multi, 1: adam_fused, 2: adam_fused in chunks (big only)
    for _ in range(3):
        sets.append([(mk(p), pkg.dn_matrix(*s), pkg.dn_matrix(*s), pkg.dn_matrix(*s)) for p, s in zip(P0, shapes)])
        for p, g, m, v in sets[-1]:
            m.zero(ctx); v.zero(ctx)
    table = pkg.ops.adam_table(ctx, [(p, g, m, v, wd) for (p, g, m, v), wd in zip(sets[0], wds)])
    assert table.blocks == sum((s[0] * s[1] + 1023) // 1024 for s in shapes)
    p64 = P0[big].astype(np.float64)
    m64, v64 = np.zeros_like(p64), np.zeros_like(p64)
    worst = 0.0
    for step in range(1, 4):
        c1, c2 = _f32(1 - B1 ** step), _f32(1 - B2 ** step)
        grads = [rng.standard_normal(s, dtype=np.float32) for s in shapes]
        for k, gr in enumerate(grads):
            for st in sets:
                st[k][1].init(gr)
        table.step(ctx, LR, B1, B2, c1, c2, EPS)
        for (p, g, m, v), wd in zip(sets[1], wds):
            pkg.ops.adam_fused(ctx, p, g, m, v, LR, B1, B2, wd, c1, c2, EPS)
        p, g, m, v = sets[2][big]
        for a, k in _chunks(ADAM_N, CHUNK):
            ctx.lib.mggcn_adam_fused_f32(ctx.stream(0), p.buffer() + 4 * a, g.buffer() + 4 * a, m.buffer() + 4 * a,
                                         v.buffer() + 4 * a, LR, B1, B2, WD, c1, c2, EPS, k)
        ctx.sync()
        for k, (a, b) in enumerate(zip(sets[0], sets[1])):
            for name, x, y in zip("pgmv", a, b):
                _assert_bits_equal(x.numpy(), y.numpy(), f"step {step}, tensor {k} {shapes[k]}, {name}: adam_multi vs adam_fused")
        for name, x, y in zip("pgmv", sets[1][big], sets[2][big]):
            _assert_bits_equal(x.numpy(), y.numpy(), f"step {step}, {name}: adam_fused in one call vs chunks of {CHUNK}")
        p64, g64, m64, v64 = _adam64(p64, grads[big].astype(np.float64), m64, v64, step, WD)
        for name, got, want in zip("pgmv", sets[1][big], (p64, g64, m64, v64)):
            err = np.abs(got.numpy() - want) / np.maximum(np.abs(want), LR)
            worst = max(worst, float(err.max()))
            assert err.max() <= 1e-5, f"step {step}, {name}: {_first_bad(err > 1e-5)}"
    print(f"\n[multipass] adam_fused, 3 steps: worst error {worst:.3e} of max(|.|, lr) (bar 1e-5)")


# ---- the fused loss ----------------------------------------------------------------------------------------------------
def _xent64(H, Y, gs):
    """fp64 softmax cross-entropy of fp32 logits: (gradient, per-row largest probability, per-row -log p_y, first-maximum argmax)"""
    x = H.astype(np.float64)
    rows = np.arange(H.shape[0])
    mx = x.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        e = np.exp(x - mx)
    s = e.sum(axis=1, keepdims=True)
    p = e / s
    with np.errstate(divide="ignore"):
        nll = -((x - mx)[rows, Y] - np.log(s[:, 0]))
    pmax = p.max(axis=1)
    p[rows, Y] -= 1.0
    p *= gs
    return p, pmax, nll, H.argmax(axis=1)


def _xent_where(r, m):
    S, R = _xent_geometry(m)
    return f"row {r}: pass {r // (S * R)}, slot {(r // S) % R}, offset {r % S} of the slot"


def _slot_rows(n, m):
    """first, an inner and the last row of every (pass, slot) that holds rows, and the last rows of the matrix"""
    S, _ = _xent_geometry(m)
    rows = []
    for a in range(0, n, S):
        rows += [a, a + 5, a + S // 2 + 3, a + S - 1]
    rows += [n - 1, n - 2, n - 7]
    return sorted({r for r in rows if 0 <= r < n})


def _plant_ties(H, Y, m):
    """full ties and two-way ties in every pass and slot; the label is the FIRST tied column, so a kernel that lets the
    last maximum win counts every one of these rows differently (all in the same direction: they cannot cancel)"""
    n = H.shape[0]
    if m < 2:
        return 0
    planted = 0
    for k, r in enumerate(_slot_rows(n, m)):
        if k % 2 == 0 or m < 3:
            H[r, :] = np.float32(-2.25 + (k % 5))
            Y[r] = 0
        else:
            a, b = 1 + k % (m - 2), m - 1                      # a < b; b sits in the last lane group / register
            H[r, [a, b]] = H[r].max() + np.float32(1.5)
            Y[r] = a
        planted += 1
    return planted


def _run_xent(ctx, Hg, Gg, Yd, n, m, gs):
    torch = _torch()
    sums = torch.zeros(2, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.lib.mggcn_softmax_xent_fused_from_f32(ctx.stream(0), Hg.ptr, Gg.ptr, Yd.data_ptr(), n, m, gs, sums.data_ptr())
    ctx.sync()
    return sums.cpu().numpy().copy()


def _check_xent(ctx, H, Y, what):
    """the five checks of the fused loss on one (logits, labels) pair; returns (the worst per-row gradient error in units
    of grad_scale * the row's largest probability, the gradient)"""
    n, m = H.shape
    gs = _f32(1.0 / n)
    G64, pmax, nll, amax = _xent64(H, Y, gs)
    Yd = _dev(Y.astype(np.int32).reshape(-1, 1))
    # out of place, twice; then in place
    Hg, Gg = Guarded(n, m, m, 0, logical=H), Guarded(n, m, m, 0, output=True)
    s1 = _run_xent(ctx, Hg, Gg, Yd, n, m, gs)
    b = Gg.bits()
    Gg.check_guards(f"{what}: G", b)
    Hg.check_unchanged(f"{what}: logits, out of place")                                   # (5)
    G = Gg.values(b)
    del Gg, b
    G2 = Guarded(n, m, m, 0, output=True)
    s2 = _run_xent(ctx, Hg, G2, Yd, n, m, gs)
    _assert_bits_equal(G2.values(), G, f"{what}: second out-of-place run")
    del G2, Hg
    Hi = Guarded(n, m, m, 0, logical=H, output=True)
    s3 = _run_xent(ctx, Hi, Hi, Yd, n, m, gs)
    b = Hi.bits()
    Hi.check_guards(f"{what}: in place", b)
    _assert_bits_equal(Hi.values(b), G, f"{what}: in place vs out of place")
    del Hi, b
    _assert_bits_equal(s2, s1, f"{what}: sums, second run"); _assert_bits_equal(s3, s1, f"{what}: sums, in place")     # (3)
    # (1) gradient, row by row
    assert np.isfinite(G).all(), f"{what}: {_first_bad(~np.isfinite(G))}"
    err = np.abs(G - G64).max(axis=1) / (gs * pmax)
    bad = np.flatnonzero(err > 1e-4)
    S, R = _xent_geometry(m)
    assert bad.size == 0, (f"{what}: {bad.size} gradient row(s) above 1e-4 of grad_scale * max p; worst {err.max():.3e}; first: "
                           f"{_xent_where(int(bad[0]), m)}; (pass, slot) of the bad rows: "
                           f"{sorted({(int(r) // (S * R), int(r) // S % R) for r in bad})[:16]}")
    # (2) the correct count, exactly
    want_correct = int((amax == Y).sum())
    assert float(s1[1]) == float(want_correct), f"{what}: correct count {s1[1]} != {want_correct}"
    # (3) the loss sum
    want_loss = float(nll.sum())
    assert abs(float(s1[0]) - want_loss) <= 1e-4 * abs(want_loss), f"{what}: loss sum {s1[0]} vs {want_loss}"
    # (4) rows are independent: the same rows through calls of <= 4096 rows
    sample = np.unique(np.concatenate([np.linspace(0, n - 1, min(n, 6000)).astype(np.int64), _slot_rows(n, m)]))
    assert sample.size >= min(n, 4096) and sample[-1] == n - 1
    for a, k in _chunks(sample.size, 4096):
        idx = sample[a:a + k]
        Hs, Gs = Guarded(k, m, m, 0, logical=H[idx]), Guarded(k, m, m, 0, output=True)
        _run_xent(ctx, Hs, Gs, _dev(Y[idx].astype(np.int32).reshape(-1, 1)), k, m, gs)
        small = Gs.values()
        neq = np.flatnonzero((small.view(np.uint32) != G[idx].view(np.uint32)).any(axis=1))
        assert neq.size == 0, (f"{what}: {neq.size} sampled row(s) differ from the same rows in a {k}-row call; first: "
                               f"{_xent_where(int(idx[neq[0]]), m)}")
    print(f"\n[multipass] {what}: worst row {err.max():.3e} of grad_scale * max p (bar 1e-4), "
          f"loss sum off by {abs(float(s1[0]) - want_loss) / max(abs(want_loss), 1e-300):.2e}")
    return float(err.max()), G


def _xent_case(m, n, seed):
    rng = np.random.default_rng(seed)
    H = (rng.standard_normal((n, m), dtype=np.float32) * np.float32(4.0))
    Y = rng.integers(0, m, n).astype(np.int64)
    planted = _plant_ties(H, Y, m)
    assert m < 2 or planted >= 2 * -(-n // _xent_geometry(m)[0]) + 2           # every (pass, slot) holds ties
    return H, Y


XENT_CASES = ([(m, n) for m in (1, 16, 17, 41, 48, 64) for n in (70_001, 300_001)]          # KE = 1, 1, 2, 3, 3, 4; R = 4
              + [(m, n) for m in (65, 128) for n in (20_011, 70_001)]                         # K = 2, R = 4
              + [(m, n) for m in (129, 256) for n in (12_007, 40_009)]                        # K = 4, R = 2
              + [(m, 20_011) for m in (257, 512)]                                             # K = 8, R = 1
              + [(m, 20_011) for m in (513, 1000, 1024)])                                     # K = 16, R = 1


@pytest.mark.parametrize("m,n", XENT_CASES)
def test_fused_loss_every_slot_and_pass(ctx, m, n):
    """Every instance of the fused loss with its grid capped: 70 001 rows at m <= 64 fill slots 0 and 1, part of slot 2 and
    leave slot 3 dead; 300 001 rows are three passes, the last ragged; likewise 20 011 / 70 001 (m <= 128), 12 007 / 40 009
    (m <= 256) and 20 011 (m <= 1024: three passes of 8 192 rows).  Per row: gradient against fp64 at 1e-4 of grad_scale *
    the row's largest probability; the correct count exactly (first maximum wins; ties planted in every pass and slot);
    the loss sum at 1e-4; the three runs bitwise equal; sampled rows bitwise equal to the same rows in small calls; the
    logits untouched out of place; nothing written outside G."""
    assert n > _xent_geometry(m)[0], "the grid is not capped: slots 1.. would be dead"
    H, Y = _xent_case(m, n, seed=1000 * m + n % 1000)
    _check_xent(ctx, H, Y, f"fused loss m={m} n={n}")


@pytest.mark.parametrize("m,n", [(41, 40_001), (64, 40_001), (128, 9_001), (256, 9_001), (1024, 9_001)])
def test_fused_loss_cold_rows_and_minus_inf_entries(ctx, m, n):
    """rows whose other logits sit 30 to 100 below the maximum (exp underflows towards zero), and rows with -inf entries
    next to a finite maximum (gradient exactly 0 there); labels only on columns of probability >= 1e-30"""
    rng = np.random.default_rng(m + n)
    H = (rng.standard_normal((n, m), dtype=np.float32) * np.float32(4.0))
    Y = rng.integers(0, m, n).astype(np.int64)
    rows = np.arange(n)
    cold = rows[rows % 3 == 0]
    top = rng.integers(0, m, cold.size)
    H[cold] = (rng.uniform(-100.0, -30.0, (cold.size, m)) + 7.0).astype(np.float32)
    H[cold, top] = np.float32(7.0)
    H[cold[::2], (top[::2] + 1) % m] = np.float32(7.0 - 35.0)           # one column that keeps a label-worthy probability
    inf_rows = rows[rows % 3 == 1]
    mask = rng.random((inf_rows.size, m)) < 0.3
    mask[np.arange(inf_rows.size), H[inf_rows].argmax(axis=1)] = False   # the maximum stays finite
    H[inf_rows] = np.where(mask, -np.inf, H[inf_rows]).astype(np.float32)
    x = H.astype(np.float64)
    with np.errstate(invalid="ignore"):
        p = np.exp(x - x.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    ok = p >= 1e-30
    # move every label onto a column the reference can take the log of: the nearest allowed column at or after it
    for r in np.flatnonzero(~ok[rows, Y]):
        allowed = np.flatnonzero(ok[r])
        Y[r] = allowed[np.searchsorted(allowed, Y[r]) % allowed.size]
    if m > 1:
        Y[cold[::2]] = (top[::2] + 1) % m                                # a label 35 below the maximum: p_y ~ 6e-16
    # the inputs are what this test is about
    assert cold.size >= n // 3 and inf_rows.size >= n // 3 - 1
    if m > 1:
        gap = np.sort(H[cold], axis=1)
        assert (gap[:, -1] - gap[:, -2] >= 30.0).all() and (gap[:, -1] - gap[:, 0] <= 100.0).all()
        assert np.isneginf(H[inf_rows]).any(axis=1).mean() > 0.9 and np.isfinite(H[inf_rows].max(axis=1)).all()
    assert (p[rows, Y] >= 1e-30).all()
    assert n > _xent_geometry(m)[0]                                      # the grid is capped: slot 1 is live
    _, G = _check_xent(ctx, H, Y, f"fused loss, cold and -inf rows, m={m} n={n}")
    assert (G[np.isneginf(H)] == 0.0).all()                              # exactly


@pytest.mark.parametrize("m", [41, 130])
def test_fused_loss_all_minus_inf_row_stays_contained(ctx, m):
    """an all -inf row (NaN gradient, NaN sums: documented) leaves every other row of the call bitwise what it is without
    that row"""
    n = 300
    rng = np.random.default_rng(m)
    H = (rng.standard_normal((n, m), dtype=np.float32) * np.float32(4.0))
    Y = rng.integers(0, m, (n, 1)).astype(np.int32)
    Hbad = H.copy()
    Hbad[[1, 150, n - 1], :] = -np.inf
    Yd = _dev(Y)
    out = []
    for h in (H, Hbad):
        Hg, Gg = Guarded(n, m, m, 0, logical=h), Guarded(n, m, m, 0, output=True)
        _run_xent(ctx, Hg, Gg, Yd, n, m, _f32(1.0 / n))
        b = Gg.bits()
        Gg.check_guards("fused loss with an all -inf row", b)
        out.append(Gg.values(b))
    keep = np.ones(n, dtype=bool)
    keep[[1, 150, n - 1]] = False
    _assert_bits_equal(out[1][keep], out[0][keep], f"m={m}: rows next to an all -inf row")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "chain"])
@pytest.mark.parametrize("m", [16, 41, 64, 128, 256, 512, 1024])
def test_loss_is_shift_invariant(pkg, ctx, m, fused):
    """logits that are multiples of 1/64 in [-16, 16], and the same plus 32 768: both exact in fp32 with identical x - max,
    so the gradient and both sums are bitwise equal.  A kernel that skipped or botched the max subtraction overflows."""
    n = 9_001 if fused else 2_001
    rng = np.random.default_rng(m)
    H = (rng.integers(-1024, 1025, (n, m)) / 64.0).astype(np.float32)
    Hs = H + np.float32(32768.0)
    assert ((Hs.astype(np.float64) - 32768.0) == H).all()
    Y = rng.integers(0, m, (n, 1)).astype(np.int32)
    res = []
    for h in (H, Hs):
        L = pkg.softmax_cross_entropy_loss("s_", copy=True, fused=fused)
        L(ctx, pkg.dn_matrix.from_numpy(h), pkg.dn_matrix.from_numpy(Y))
        res.append((L.backward().numpy().copy(), L.sums.numpy().copy()))
    assert np.isfinite(res[1][0]).all() and np.isfinite(res[1][1]).all()
    _assert_bits_equal(res[1][0], res[0][0], f"m={m} fused={fused}: gradient of the shifted logits")
    _assert_bits_equal(res[1][1], res[0][1], f"m={m} fused={fused}: sums of the shifted logits")
    G64, pmax, nll, amax = _xent64(H, Y[:, 0].astype(np.int64), _f32(1.0 / n))
    if fused:
        assert (np.abs(res[0][0] - G64).max(axis=1) <= 1e-4 * _f32(1.0 / n) * pmax).all()
    assert float(res[0][1][1]) == float((amax == Y[:, 0]).sum())


# ---- more than 1024 classes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1025, 0])
def test_fused_loss_entry_point_rejects_unsupported_widths(pkg, ctx, m):
    """ops.softmax_xent_fused raises before any library call (the library would print and exit the process)"""
    torch = _torch()
    H, Y = pkg.dn_matrix(3, m), pkg.dn_matrix(3, 1, dtype=np.int32)
    sums = torch.zeros(2, dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        pkg.ops.softmax_xent_fused(ctx, H, Y, 1.0, sums)
    with pytest.raises(ValueError):
        pkg.ops.softmax_xent_fused(ctx, H, Y, 1.0, sums, out=pkg.dn_matrix(3, m))


def test_loss_layer_runs_the_chain_above_1024_classes(pkg, ctx):
    n, m = 300, 1025
    rng = np.random.default_rng(5)
    H = (rng.standard_normal((n, m)) * 3).astype(np.float32)
    Y = rng.integers(0, m, (n, 1)).astype(np.int32)
    res = []
    for fused in (True, False):
        L = pkg.softmax_cross_entropy_loss("w_", copy=True, fused=fused)
        Hd = pkg.dn_matrix.from_numpy(H)
        loss, acc = L(ctx, Hd, pkg.dn_matrix.from_numpy(Y))
        res.append((L.backward().numpy().copy(), L.sums.numpy().copy(), loss, acc))
        np.testing.assert_array_equal(Hd.numpy(), H)
    _assert_bits_equal(res[0][0], res[1][0], "gradient, fused=True vs fused=False at m = 1025")
    _assert_bits_equal(res[0][1], res[1][1], "sums, fused=True vs fused=False at m = 1025")
    assert res[0][2:] == res[1][2:]
    assert float(res[0][1][1]) == float((H.argmax(axis=1) == Y[:, 0]).sum())
