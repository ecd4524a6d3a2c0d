"""Multi-label training on one GPU: mggcn_sigmoid_bce_from_f32 (sigmoid + binary cross-entropy + gradient + the counts
behind micro-F1 in one pass), gcn(loss="bce") against the wrapped oracle, and MGGCN_LOSS=bce of the command line.

The bars are the project's (test_gpu_splits.py): a gradient row's worst error <= 1e-4 x grad_scale x max(1, max |p - t| of
the fp64 row) -- |p - t| <= 1, so 1e-4 x grad_scale --, a loss sum at 1e-4 of the fp64 sum, counts exactly equal (every
count here stays far below 2^24); the model at loss 1e-4, gradients 1e-4 (relerr), TP / FP / FN within 3 of the oracle's.
Everything that is claimed bitwise is compared as bits.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import bce_ref as ref
import dropout_ref
import layernorm_ref
from guarded import Guarded
from test_gpu_layer_norm import _sync_oracle_state
from test_gpu_multipass import STREAM_THREADS, _assert_bits_equal, _dev, _f32, _three_passes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mg-gcn_amd", "bin")
TOL = 1e-4
WIDTHS = (1, 3, 4, 100, 121, 1100)
SET_VALUES = np.array([0, 1, 2, 3, -1, 7], dtype=np.int32)          # 3, -1 and 7 all go to slot 3
SET_P = (0.45, 0.2, 0.2, 0.05, 0.05, 0.05)
# two full passes of the capped grid and a ragged third.  The kernel walks units grid-stride with stream_grid(units)
# workgroups of 256 threads, capped at kNumCU * 8: a unit is a float4 when m % 4 == 0 and the operands are 16-byte
# aligned (m / 4 units per row), an element otherwise (m units per row).
MULTIPASS_ROWS = {1: 2 * STREAM_THREADS + 12_345, 3: 400_003, 4: 2 * STREAM_THREADS + 12_345, 100: 55_001, 121: 11_003,
                  1100: 4_801}


def _units_per_row(m, aligned=True):
    return m // 4 if m % 4 == 0 and aligned else m


def _multipass_rows(m):
    n = MULTIPASS_ROWS[m]
    _three_passes(n * _units_per_row(m), STREAM_THREADS, f"sigmoid_bce m={m}")     # asserts that the grid is capped
    return n


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


def _torch():
    import torch
    return torch


def _case(m, n, seed):
    rng = np.random.default_rng(seed)
    H = rng.standard_normal((n, m), dtype=np.float32) * np.float32(4.0)
    T = (rng.random((n, m)) < 0.1).astype(np.int32)
    T[T != 0] = rng.integers(1, 5, int((T != 0).sum())) * rng.choice([-1, 1], int((T != 0).sum()))   # non-zero = positive
    S = SET_VALUES[rng.choice(len(SET_VALUES), size=n, p=SET_P)].astype(np.int32)
    return H, T, S


def _run(ctx, h_ptr, g_ptr, t_ptr, Sd, n, m, t, gs):
    torch = _torch()
    sums = torch.zeros(16, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.lib.mggcn_sigmoid_bce_from_f32(ctx.stream(0), h_ptr, g_ptr, t_ptr, None if Sd is None else Sd.data_ptr(), n, m, t, gs,
                                       sums.data_ptr())
    ctx.sync()
    return sums.cpu().numpy().copy()


class _Ref:
    """the fp64 side of one (H, T), computed once and shared by the calls on it"""

    def __init__(self, H, T):
        self.d64 = ref.prob64(H) - (T != 0)                          # p - t
        self.loss = ref.loss64(H, T)
        self.pred, self.pos = ref.pred(H), T != 0


def _check(ctx, H, T, S, t, what, R=None, off=0):
    """the whole list of (1) for one call; returns (G, sums).  ``off``: base offset of all three matrices in floats"""
    n, m = H.shape
    R = R or _Ref(H, T)
    slot = np.zeros(n, dtype=np.int64) if S is None else ref.slot(S)
    train = np.ones(n, dtype=bool) if S is None else S == t
    gs = _f32(1.0 / (max(int(train.sum()), 1) * m))
    Sd = None if S is None else _dev(S.reshape(-1, 1))
    Tg = Guarded(n, m, m, off, logical=T.view(np.uint32))
    # out of place, twice; then in place (G == logits)
    Hg, Gg = Guarded(n, m, m, off, logical=H), Guarded(n, m, m, off, output=True)
    s1 = _run(ctx, Hg.ptr, Gg.ptr, Tg.ptr, Sd, n, m, t, gs)
    b = Gg.bits()
    Gg.check_guards(f"{what}: G", b)
    Hg.check_unchanged(f"{what}: logits, out of place")
    Tg.check_unchanged(f"{what}: targets")
    G = Gg.values(b)
    del Gg, b
    G2 = Guarded(n, m, m, off, output=True)
    s2 = _run(ctx, Hg.ptr, G2.ptr, Tg.ptr, Sd, n, m, t, gs)
    _assert_bits_equal(G2.values(), G, f"{what}: second run")
    _assert_bits_equal(s2, s1, f"{what}: sums, second run")
    del G2, Hg
    Hi = Guarded(n, m, m, off, logical=H, output=True)
    s3 = _run(ctx, Hi.ptr, Hi.ptr, Tg.ptr, Sd, n, m, t, gs)
    b = Hi.bits()
    Hi.check_guards(f"{what}: in place", b)
    _assert_bits_equal(Hi.values(b), G, f"{what}: in place vs out of place")
    _assert_bits_equal(s3, s1, f"{what}: sums, in place")
    del Hi, b
    # rows outside train_set: +0.0 in every column, bit for bit
    offrows = G[~train].view(np.uint32)
    assert not offrows.any(), f"{what}: {int((offrows != 0).any(axis=1).sum())} row(s) outside the training set are not +0.0"
    if train.any():
        assert np.isfinite(G[train]).all(), what
        err = np.abs(G[train] - R.d64[train] * gs).max(axis=1) / (gs * np.maximum(1.0, np.abs(R.d64[train]).max(axis=1)))
        print(f"\n[bce] {what}: worst training row {err.max():.3e} of grad_scale (bar 1e-4)")
        assert err.max() <= TOL, f"{what}: worst gradient row {err.max():.3e}, row {int(np.flatnonzero(train)[err.argmax()])}"
    for k in range(4):
        r = slot == k
        p, q = R.pred[r], R.pos[r]
        want = (float(R.loss[r].sum()), float((p & q).sum()), float((p & ~q).sum()), float((~p & q).sum()))
        got = tuple(float(v) for v in s1[4 * k:4 * k + 4])
        print(f"[bce] {what}: slot {k}: {int(r.sum())} rows, (loss sum, TP, FP, FN) {got} want {want}")
        assert got[1:] == want[1:], f"{what}: slot {k}: counts {got[1:]} != {want[1:]}"
        assert abs(got[0] - want[0]) <= TOL * abs(want[0]), f"{what}: slot {k}: loss sum {got[0]} vs {want[0]}"
    return G, s1


@pytest.mark.parametrize("m", WIDTHS)
def test_bce_against_fp64_row_by_row(ctx, m):
    """(1) both load paths x {1 row, 5 rows, two passes of the capped grid and a ragged third} x the three train_set values
    with S drawn row by row from {0, 1, 2, 3, -1, 7}, and the S == NULL form"""
    for n in (1, 5, _multipass_rows(m)):
        H, T, S = _case(m, n, seed=5000 * m + n % 1000)
        R = _Ref(H, T)
        for t in (0, 1, 2):
            if n == 1:
                S = np.array([t if m % 2 else (t + 1) % 3], dtype=np.int32)      # the only row trains / does not train
            _check(ctx, H, T, S, t, f"bce m={m} n={n} train_set={t}", R)
        _check(ctx, H, T, None, 0, f"bce m={m} n={n} S=NULL", R)


@pytest.mark.parametrize("m", WIDTHS)
def test_null_sets_are_the_sets_equal_to_train_set_everywhere(ctx, m):
    """(2) G and the four sums of the training slot are bitwise those of the S == NULL form; the other twelve stay +0.0"""
    torch = _torch()
    n = _multipass_rows(m)
    H, T, _ = _case(m, n, seed=6000 * m + 1)
    gs = _f32(1.0 / (n * m))
    Hd, Td = _dev(H), _dev(T)
    G0 = torch.empty_like(Hd)
    s0 = _run(ctx, Hd.data_ptr(), G0.data_ptr(), Td.data_ptr(), None, n, m, 0, gs)
    G0 = G0.cpu().numpy()
    assert not s0[4:].view(np.uint32).any(), s0
    for t in (0, 1, 2):
        Sd = _dev(np.full((n, 1), t, dtype=np.int32))
        Gs = torch.empty_like(Hd)
        s = _run(ctx, Hd.data_ptr(), Gs.data_ptr(), Td.data_ptr(), Sd, n, m, t, gs)
        _assert_bits_equal(Gs.cpu().numpy(), G0, f"m={m} train_set={t}: gradient vs S == NULL")
        _assert_bits_equal(s[4 * t:4 * t + 4], s0[0:4], f"m={m} train_set={t}: the training slot's sums vs S == NULL")
        rest = np.delete(s, range(4 * t, 4 * t + 4))
        assert not rest.view(np.uint32).any(), f"m={m} train_set={t}: the other slots' sums are not +0.0: {s}"


@pytest.mark.parametrize("m,n", [(100, 5), (100, 2_001), (4, 7), (1100, 3)])
def test_a_misaligned_base_runs_the_element_path_with_the_same_gradient(ctx, m, n):
    """(3) the same matrices one float off 16-byte alignment: G bitwise equal, sums within 1e-4, counts equal"""
    H, T, S = _case(m, n, seed=7000 + m + n)
    R = _Ref(H, T)
    Ga, sa = _check(ctx, H, T, S, 0, f"aligned m={m} n={n}", R, off=0)
    Gb, sb = _check(ctx, H, T, S, 0, f"offset by one float m={m} n={n}", R, off=1)
    _assert_bits_equal(Gb, Ga, f"m={m} n={n}: gradient, element path vs 16-byte path")
    for k in range(4):
        assert abs(float(sb[4 * k]) - float(sa[4 * k])) <= TOL * abs(float(sa[4 * k])), (k, sa, sb)
        _assert_bits_equal(sb[4 * k + 1:4 * k + 4], sa[4 * k + 1:4 * k + 4], f"m={m} n={n}: counts of slot {k}")
    # only ONE operand off alignment is the element path too
    torch = _torch()
    Hd, Sd = _dev(H), _dev(S.reshape(-1, 1))
    Tg = Guarded(n, m, m, 1, logical=T.view(np.uint32))
    Gd = torch.empty_like(Hd)
    gs = _f32(1.0 / (max(int((S == 0).sum()), 1) * m))
    s = _run(ctx, Hd.data_ptr(), Gd.data_ptr(), Tg.ptr, Sd, n, m, 0, gs)
    _assert_bits_equal(Gd.cpu().numpy(), Ga, f"m={m} n={n}: gradient with only the targets misaligned")
    _assert_bits_equal(s, sb, f"m={m} n={n}: sums with only the targets misaligned")


@pytest.mark.parametrize("m", [100, 121, 4, 3])
def test_a_row_range_alone_gives_the_bits_of_the_whole_call(ctx, m):
    """(4) rows [a, b), a and b no multiples of 4, with the whole call's grad_scale"""
    torch = _torch()
    n = 1_001 if m >= 100 else 30_011
    H, T, S = _case(m, n, seed=8000 + m)
    gs = _f32(1.0 / (max(int((S == 1).sum()), 1) * m))
    Hd, Td, Sd = _dev(H), _dev(T), _dev(S.reshape(-1, 1))
    G = torch.empty_like(Hd)
    _run(ctx, Hd.data_ptr(), G.data_ptr(), Td.data_ptr(), Sd, n, m, 1, gs)
    G = G.cpu().numpy()
    for a, b in ((3, n - 2), (1, 6), (n - 6, n - 2)):
        assert a % 4 and b % 4
        Hs, Ts, Ss = _dev(H[a:b]), _dev(T[a:b]), _dev(S[a:b].reshape(-1, 1))
        Gs = torch.empty_like(Hs)
        _run(ctx, Hs.data_ptr(), Gs.data_ptr(), Ts.data_ptr(), Ss, b - a, m, 1, gs)
        _assert_bits_equal(Gs.cpu().numpy(), G[a:b], f"m={m}: rows [{a}, {b}) alone")


SPECIAL = [0.0, -0.0, 88.0, -88.0, 104.0, -104.0, 1e30, -1e30, np.inf, -np.inf]


def test_special_values(ctx):
    """(5) z in {+-0, +-88, +-104, +-1e30, +-inf} against both targets, one element per call and all of them on the
    16-byte path: the loss is finite or +inf and never NaN, G is exactly 0 or +-grad_scale where p saturates in fp32
    (p = 1 exactly for z >= 88: 1 + e^-88 rounds to 1; p underflows to 0 for z <= -104: e^-104 is below half the
    smallest denormal times any grad_scale <= 1/2; at z = -88 p = e^-88 ~ 6e-39 is a denormal, so there G only has to lie
    in [0, 1e-38 x grad_scale] for t = 0 and is -grad_scale exactly for t = 1), pred follows z > 0"""
    torch = _torch()
    gs = _f32(0.01)
    Z = np.array([SPECIAL + [1.0, -1.0]] * 2, dtype=np.float32)
    T = np.array([[0] * 12, [1] * 12], dtype=np.int32)
    single = np.zeros((2, len(SPECIAL)), dtype=np.float32)
    with np.errstate(over="ignore"):
        l64 = ref.loss64(Z, T)
    for ti in (0, 1):
        for zi, z in enumerate(SPECIAL):
            Hd, Td, Gd = _dev(np.array([[z]], dtype=np.float32)), _dev(np.array([[ti]], dtype=np.int32)), torch.empty(1, 1, device="cuda")
            s = _run(ctx, Hd.data_ptr(), Gd.data_ptr(), Td.data_ptr(), None, 1, 1, 0, gs)
            g = float(Gd.cpu().numpy()[0, 0])
            single[ti, zi] = g
            loss, tp, fp, fn = (float(v) for v in s[:4])
            print(f"[bce] z={z!r} t={ti}: loss {loss!r} G {g!r} (tp, fp, fn) {(tp, fp, fn)}")
            assert not np.isnan(loss) and loss >= 0, (z, ti, loss)
            assert np.isinf(loss) == np.isinf(l64[ti, zi]), (z, ti, loss)
            if np.isfinite(l64[ti, zi]):
                assert abs(loss - l64[ti, zi]) <= 1e-6 * l64[ti, zi] + 1e-37, (z, ti, loss, l64[ti, zi])
            pred = z > 0
            assert (tp, fp, fn) == (float(pred and ti), float(pred and not ti), float(not pred and ti)), (z, ti, s[:4])
            if z == 0:
                assert g == (0.5 - ti) * gs, (z, ti, g)
            elif z == -88.0 and ti == 0:
                assert 0.0 <= g <= 1e-38 * gs, (z, ti, g)
            else:
                assert g == ((1.0 if z > 0 else 0.0) - ti) * gs, (z, ti, g)
    Hd, Td, Gd = _dev(Z), _dev(T), torch.empty(2, 12, device="cuda")
    s = _run(ctx, Hd.data_ptr(), Gd.data_ptr(), Td.data_ptr(), None, 2, 12, 0, gs)
    _assert_bits_equal(Gd.cpu().numpy()[:, :len(SPECIAL)], single, "special values on the 16-byte path vs one by one")
    assert np.isinf(s[0]) and s[0] > 0 and not np.isnan(s).any(), s


@pytest.mark.parametrize("m", [100, 121])
def test_a_nan_logit_stays_in_its_slot(ctx, m):
    """(5) a NaN planted in one validation row against the same logit set to 0: the train, test and other sums, all counts
    and every other element of G are bitwise unchanged"""
    torch = _torch()
    n = 2_001
    H, T, S = _case(m, n, seed=9000 + m)
    r = int(np.flatnonzero(S == 1)[3])
    H0, H1 = H.copy(), H.copy()
    H0[r, 7], H1[r, 7] = 0.0, np.nan
    gs = _f32(1.0 / (int((S == 0).sum()) * m))
    Td, Sd = _dev(T), _dev(S.reshape(-1, 1))
    out = []
    for Hx in (H0, H1):
        Hd = _dev(Hx)
        Gd = torch.empty_like(Hd)
        s = _run(ctx, Hd.data_ptr(), Gd.data_ptr(), Td.data_ptr(), Sd, n, m, 0, gs)
        out.append((Gd.cpu().numpy(), s))
    (G0, s0), (G1, s1) = out
    assert np.isnan(s1[4]) and np.isfinite(s0).all(), (s0, s1)
    keep = np.ones(16, dtype=bool)
    keep[4] = False                                                  # the validation loss sum is the only one that moves
    _assert_bits_equal(s1[keep], s0[keep], f"m={m}: sums outside the NaN's slot, and every count")
    mask = np.ones_like(G0, dtype=bool)
    mask[r, 7] = False
    _assert_bits_equal(G1[mask], G0[mask], f"m={m}: every other element of G")
    assert G1[r, 7].view(np.uint32) == 0                             # a validation row: +0.0, not NaN


def test_ops_wrapper_validates_before_the_library(pkg, ctx):
    """(6) ValueError for a float T, a wrong shape, a short sums tensor and train_set = 3; a good call equals the C ABI's"""
    torch = _torch()
    n, m = 9, 12
    H, T, S = _case(m, n, seed=3)
    dn = pkg.dn_matrix
    Hd, Td, Sd = dn.from_numpy(H), dn.from_numpy(T), dn.from_numpy(S.reshape(-1, 1))
    sums = torch.zeros(16, dtype=torch.float32, device="cuda")
    for bad_T in (dn.from_numpy(T.astype(np.float32)), dn.from_numpy(T[:, :-1]), dn.from_numpy(T[:-1])):
        with pytest.raises(ValueError):
            pkg.ops.sigmoid_bce(ctx, Hd, bad_T, Sd, 0, 0.1, sums)
    with pytest.raises(ValueError):
        pkg.ops.sigmoid_bce(ctx, Hd, Td, Sd, 0, 0.1, sums[:15])
    with pytest.raises(ValueError):
        pkg.ops.sigmoid_bce(ctx, Hd, Td, Sd, 3, 0.1, sums)
    with pytest.raises(ValueError):
        pkg.ops.sigmoid_bce(ctx, Hd, Td, dn.from_numpy(S[:-1].reshape(-1, 1)), 0, 0.1, sums)
    with pytest.raises(ValueError):
        pkg.ops.sigmoid_bce(ctx, Hd, Td, Sd, 0, 0.1, sums, out=dn(n, m + 1))
    ctx.sync()
    assert not sums.cpu().numpy().any()                              # nothing ran
    Gd = dn(n, m)
    gs = _f32(0.1)
    pkg.ops.sigmoid_bce(ctx, Hd, Td, Sd, 0, gs, sums, out=Gd)
    ctx.sync()
    raw = torch.empty(n, m, device="cuda")
    s = _run(ctx, Hd.buffer(), raw.data_ptr(), Td.buffer(), Sd.t, n, m, 0, gs)
    _assert_bits_equal(Gd.numpy(), raw.cpu().numpy(), "ops.sigmoid_bce vs the C ABI")
    _assert_bits_equal(sums.cpu().numpy(), s, "ops.sigmoid_bce sums vs the C ABI")


_CHILD = """
import sys
import numpy as np
sys.path.insert(0, {root!r})
import __graft_entry__ as ge
pkg = ge.load_package()
import torch
ctx = pkg.context(0)
H = torch.zeros(2, 4, device="cuda"); T = torch.zeros(2, 4, dtype=torch.int32, device="cuda")
sums = torch.zeros(16, device="cuda")
torch.cuda.synchronize()
ctx.lib.mggcn_sigmoid_bce_from_f32(ctx.stream(0), H.data_ptr(), H.data_ptr(), T.data_ptr(), None, 2, 4, 3, 0.1, sums.data_ptr())
print("returned")
"""


def test_the_library_refuses_train_set_3_itself():
    """(6) a host check before any launch: the library prints its precondition message and exits non-zero (a fresh child)"""
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "returned" not in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
    assert "MGGCN precondition failed" in r.stderr and "train_set" in r.stderr, r.stderr[-2000:]


# ---- the model ---------------------------------------------------------------------------------------------------------
N, F, C, HIDDEN = 1536, 20, 8, [16, 16]
SIZES = [F] + HIDDEN + [C]
ADAM = layernorm_ref.ADAM
relerr = layernorm_ref.relerr


def _grads(layers, is_dev):
    out = []
    for l in layers:
        row = {"G_W": l.lin.G_W, "G_b": l.lin.G_b}
        if getattr(l, "norm", None) is not None:
            row.update(G_gamma=l.norm.G_gamma, G_beta=l.norm.G_beta)
        out.append({k: (v.numpy().copy() if is_dev else np.array(v, copy=True)) for k, v in row.items()})
    return out


def _host_f1(logits, T, rows=slice(None)):
    c = ref.counts(logits[rows], T[rows])[0]
    return ref.micro_f1(*c)


@pytest.mark.parametrize("splits,dropout,norm", [(False, 0.0, None), (True, 0.0, None), (True, 0.5, "layer")])
def test_model_matches_the_wrapped_oracle(pkg, oracle, ctx, splits, dropout, norm):
    """(7) three epochs of gcn(loss="bce") against oracle.Gcn with the loss replaced (bce_ref.oracle_bce), from identical
    state every epoch (the oracle takes over the device's parameters and Adam moments, as the norm's test does); the last
    epoch through train_step, whose gradients are compared after the Adam step (both sides add the weight decay in place)"""
    csr, X, T, S = ref.model_data(pkg, N, F, C)
    ip, ix, dv = csr
    G = pkg.gcn(pkg.csr_matrix(ip.copy(), ix.copy(), dv.copy(), N), SIZES, dropout=dropout, norm=norm, loss="bce")
    assert type(G.loss_layer).__name__ == "sigmoid_bce_loss"
    O = oracle.Gcn(oracle.Csr(ip.copy(), ix.copy(), dv.copy(), N), SIZES, f64acc=True)
    if norm:
        layernorm_ref.oracle_layer_norm(oracle, O)
        for layer, ol in zip(G.layers()[:-1], O.layers[:-1]):
            layer.norm.gamma.init(ol.norm.gamma)
            layer.norm.beta.init(ol.norm.beta)
    B = ref.oracle_bce(oracle, O, T, S if splits else None, 0)
    if dropout:
        G.set_dropout(dropout, seed=2024)
        dropout_ref.oracle_dropout(O, dropout, seed=2024)               # on top of the norm and the loss wrappers
    if splits:
        G.set_splits(S)
    # the comparison can tell the two losses apart: softmax on the arg-max labels of the same targets is far away
    plain = oracle.Gcn(oracle.Csr(ip.copy(), ix.copy(), dv.copy(), N), SIZES, f64acc=True)
    soft = plain.train_forward(X, T.argmax(axis=1).reshape(-1, 1).astype(np.int32))[0]
    bce0 = ref.oracle_bce(oracle, plain, T).loss(plain.forward(X))[0]
    assert abs(soft - bce0) > 100 * TOL * abs(bce0), (soft, bce0)
    Xd, Td = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(T)
    name = "train"
    for epoch in range(3):
        _sync_oracle_state(G, O)
        ol, of1 = O.train_forward(X, T)
        O.backward()
        og = _grads(O.layers, False)
        O.adam_update()
        og_after = _grads(O.layers, False)
        if epoch < 2:
            loss, f1 = G.train_forward(ctx, Xd, Td)
            G.backward(ctx)
            ctx.sync()
            got, want = _grads(G.layers(), True), og
            G.adam_update(ctx, *ADAM)
            ctx.sync()
        else:
            loss, f1 = G.train_step(ctx, Xd, Td, *ADAM)
            got, want = _grads(G.layers(), True), og_after
        conf = G.loss_layer.confusion()
        print(f"[bce] splits={splits} dropout={dropout} norm={norm} epoch {epoch}: loss {loss!r} oracle {ol!r}, f1 {f1!r} "
              f"oracle {of1!r}, (tp, fp, fn) {conf} oracle {B.per[name][2]}")
        assert abs(loss - ol) <= TOL * abs(ol), (epoch, loss, ol)
        for k, (a, b) in enumerate(zip(conf, B.per[name][2])):
            assert abs(a - b) <= 3, (epoch, ("tp", "fp", "fn")[k], conf, B.per[name][2])
        assert f1 == ref.micro_f1(*conf)
        if splits:
            m = G.split_metrics()
            assert m["train"] == (loss, f1) and set(m) == {"train", "val", "test", "other", "counts", "confusion"}
            for nm in ("train", "val", "test"):
                wl, _, wc, rows = B.per[nm]
                assert m["counts"][nm] == rows and abs(m[nm][0] - wl) <= TOL * abs(wl), (epoch, nm, m[nm], wl)
                assert all(abs(a - b) <= 3 for a, b in zip(m["confusion"][nm], wc)), (epoch, nm, m["confusion"][nm], wc)
            assert m["counts"]["other"] == 0 and np.isnan(m["other"]).all()
        for li in range(len(got)):
            assert set(got[li]) == set(want[li])
            for what in got[li]:
                err = relerr(got[li][what], want[li][what])
                print(f"[bce]   layer {li} {what}: {err:.3e}")
                assert err <= TOL, (epoch, li, what, err)
    # evaluate(): micro-F1 from the copied logits, all and per split
    logits = G(ctx, Xd)
    ctx.sync()
    Z = logits.numpy()
    ev = G.evaluate(ctx, Xd, Td, pkg.dn_matrix.from_numpy(S.reshape(-1, 1)))
    assert ev["all"] == _host_f1(Z, T) and 0.0 <= ev["all"] <= 1.0
    for k, nm in enumerate(("train", "val", "test")):
        assert ev[nm] == _host_f1(Z, T, S == k), (nm, ev)
    assert set(G.evaluate(ctx, Xd, Td)) == {"all"}


def test_model_refuses_targets_of_the_wrong_shape_before_any_launch(pkg, ctx):
    csr, X, T, S = ref.model_data(pkg, N, F, C)
    G = pkg.gcn(pkg.csr_matrix(*(a.copy() for a in csr), N), SIZES, loss="bce")
    Xd = pkg.dn_matrix.from_numpy(X)
    for bad in (pkg.dn_matrix.from_numpy(T[:, :1]), pkg.dn_matrix.from_numpy(T.astype(np.float32)),
                pkg.dn_matrix.from_numpy(T[:-1])):
        for call in (lambda Y: G.train_forward(ctx, Xd, Y), lambda Y: G.train_step(ctx, Xd, Y, *ADAM),
                     lambda Y: G.evaluate(ctx, Xd, Y)):
            with pytest.raises(ValueError, match="int32 targets"):
                call(bad)
    assert G._plan_wants                                             # not even the SpMM plans were built


# ---- the CLI -----------------------------------------------------------------------------------------------------------
def _cli(tmp_path, d, args, env_extra, E=3):
    env = {k: v for k, v in os.environ.items() if k not in ("MGGCN_LOSS", "MGGCN_TRAIN_SET")}
    env.update(env_extra, MGGCN_OVERSUBSCRIBE="1")
    return subprocess.run([os.path.join(BIN, "mg_gcn")] + args + ["-E", str(E), "train", str(d), "2", "16", "16"],
                          cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def bce_dir(pkg, tmp_path_factory):
    csr, X, T, S = ref.model_data(pkg, N, F, C)
    d = tmp_path_factory.mktemp("bce") / "permuted" / "multi"
    pkg.datasets.write_dataset(str(d), *csr, X, T, S)
    return d


@pytest.mark.parametrize("train_set", [None, 0])
def test_cli_bce_matches_the_python_model(pkg, ctx, tmp_path, bce_dir, train_set):
    """(8) MGGCN_LOSS=bce [MGGCN_TRAIN_SET=0] mg_gcn -P 1: every epoch replayed by the Python model from the weights the
    command line started it with (MGGCN_DUMP_WEIGHTS): loss at 1e-4, micro-F1 from counts within 3"""
    E = 3
    csr, X, T, S = ref.model_data(pkg, N, F, C)
    env = dict(MGGCN_LOSS="bce", MGGCN_DUMP_WEIGHTS=str(tmp_path / "w"))
    if train_set is not None:
        env["MGGCN_TRAIN_SET"] = str(train_set)
    r = _cli(tmp_path, bce_dir, ["-P", "1"], env, E)
    assert r.returncode == 0, r.stderr[-3000:]
    head, lines = r.stderr.strip().splitlines()[:3], r.stderr.strip().splitlines()[3:]
    assert head[1] == f"num_labels = {C}" and head[2] == f"feature size = {F}", head
    epoch = [tuple(float(x) for x in ln.split()) for ln in lines if not ln.startswith("[")]
    splits = [ln.split() for ln in lines if ln.startswith("[mggcn splits]")]
    assert len(epoch) == E and all(len(e) == 4 for e in epoch), r.stderr[-3000:]
    assert len(splits) == (E if train_set is not None else 0)
    G = pkg.gcn(pkg.csr_matrix(*(a.copy() for a in csr), N), SIZES, loss="bce")
    if train_set is not None:
        G.set_splits(S, train_set)
    Xd, Td = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(T)

    def f1_within_3(got, conf):
        """the F1 of SOME (tp, fp, fn) within 3 of the model's counts"""
        tp, fp, fn = conf
        lo = ref.micro_f1(max(tp - 3, 0), fp + 3, fn + 3)
        hi = ref.micro_f1(tp + 3, max(fp - 3, 0), max(fn - 3, 0))
        return lo - 1e-6 <= got <= hi + 1e-6

    for e in range(E):
        for li, layer in enumerate(G.layers()):
            layer.W().init(pkg.datasets.read_dense(str(tmp_path / "w" / f"e{e}_W{li}.bin"), "<f4"))
            layer.b().init(pkg.datasets.read_dense(str(tmp_path / "w" / f"e{e}_b{li}.bin"), "<f4"))
        loss, f1 = G.train_forward(ctx, Xd, Td)
        print(f"[bce] cli train_set={train_set} epoch {e}: {epoch[e]} vs the Python model {(loss, f1)}")
        assert int(epoch[e][0]) == e and abs(epoch[e][1] - loss) <= TOL * abs(loss), (e, epoch[e], loss)
        assert f1_within_3(epoch[e][2], G.loss_layer.confusion()), (e, epoch[e], f1, G.loss_layer.confusion())
        if train_set is not None:
            m, w = G.split_metrics(), splits[e]
            assert w[:3] == ["[mggcn", "splits]", str(e)] and w[3::3] == ["train", "val", "test"], w
            for k, nm in enumerate(("train", "val", "test")):
                gl, gf = float(w[4 + 3 * k]), float(w[5 + 3 * k])
                assert abs(gl - m[nm][0]) <= TOL * abs(m[nm][0]), (e, nm, gl, m[nm])
                assert f1_within_3(gf, m["confusion"][nm]), (e, nm, gf, m[nm], m["confusion"][nm])
    assert epoch[-1][1] < epoch[0][1]


@pytest.mark.parametrize("args,env,message", [(["-P", "2", "-R", "1"], {"MGGCN_LOSS": "bce"}, "MGGCN_LOSS=bce is single-GPU only"),
                                              (["-P", "1", "-R", "1"], {"MGGCN_LOSS": "bce"}, "MGGCN_LOSS=bce is single-GPU only"),
                                              (["-P", "1"], {"MGGCN_LOSS": "hinge"}, "MGGCN_LOSS must be softmax or bce")])
def test_cli_rejects_before_training(tmp_path, bce_dir, args, env, message):
    r = _cli(tmp_path, bce_dir, args, env)
    assert r.returncode != 0 and message in r.stderr, r.stderr[-2000:]
    assert "num_labels" not in r.stderr                               # before anything was loaded


@pytest.mark.parametrize("env", [{}, {"MGGCN_LOSS": "softmax"}])
def test_cli_without_bce_is_the_softmax_run(pkg, tmp_path, env):
    """unset (or softmax): the five stderr lines of a 2-epoch run, num_labels = 1 + max label"""
    n, F_, C_ = 512, 8, 3
    ip, ix, dv = pkg.datasets.synth_uniform_csr(n, 6, seed=1)
    rng = np.random.default_rng(2)
    d = tmp_path / "permuted" / "tiny"
    Y = rng.integers(0, C_, size=(n, 1)).astype(np.int32)
    Y[0, 0] = C_ - 1
    pkg.datasets.write_dataset(str(d), ip, ix, dv, rng.standard_normal((n, F_), dtype=np.float32), Y)
    e = {k: v for k, v in os.environ.items() if k not in ("MGGCN_LOSS", "MGGCN_TRAIN_SET")}
    e.update(env)
    r = subprocess.run([os.path.join(BIN, "mg_gcn"), "-P", "1", "-E", "2", "train", str(d), "1", "8"], cwd=str(tmp_path),
                       env=e, capture_output=True, text=True, timeout=600)
    lines = r.stderr.strip().splitlines()
    assert r.returncode == 0 and len(lines) == 5 and lines[1] == f"num_labels = {C_}", r.stderr
    assert 0.0 <= float(lines[3].split()[2]) <= 1.0
