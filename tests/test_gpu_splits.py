"""Split-aware training on one GPU: mggcn_softmax_xent_split_from_f32, the two steps of the unfused chain
(mggcn_select_rows_by_set_f32, mggcn_abssum_by_set_f32) and gcn.set_splits.

S holds one set value per row (sets.bin: 0 train / 1 validation / 2 test); slot(s) = s for 0 <= s <= 2, 3 for every other
value.  Rows outside train_set get a gradient row of +0.0, the gradient is scaled by 1 / n_train, and a (loss sum, correct
count) pair is kept per slot.

The bars are the project's own (test_gpu_multipass.py): a gradient row at 1e-4 of grad_scale x the row's
largest probability, correct counts exact, loss sums at 1e-4 of the fp64 sum, |x| sums at 1e-5; the model at the bars of
test_dist_gpu.py (loss 1e-4, accuracy 3 / n_split, a gradient tensor at 1e-4 of its largest entry).  Everything that
is claimed bitwise is compared as bits.
"""
import os
import subprocess

import numpy as np
import pytest

from guarded import Guarded
from test_gpu_multipass import (ABSSUM_ELEMS, RAGGED, STREAM_THREADS, _assert_bits_equal, _dev, _f32, _plant_ties,
                                _slot_rows, _three_passes, _xent64, _xent_geometry)

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 5, 16, 17, 41, 48, 64, 65, 128, 200, 1024)
SET_VALUES = np.array([0, 1, 2, 3, -1, 7], dtype=np.int32)          # 3, -1 and 7 all go to slot 3
SET_P = (0.45, 0.2, 0.2, 0.05, 0.05, 0.05)


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


def _torch():
    import torch
    return torch


def _slot(S):
    S = np.asarray(S).reshape(-1)
    return np.where((S >= 0) & (S <= 2), S, 3).astype(np.int64)


def _multipass_rows(m):
    """two full passes of the capped grid and a ragged third: the sizes of test_gpu_multipass.py XENT_CASES"""
    n = 300_001 if m <= 64 else 70_001 if m <= 128 else 40_009 if m <= 256 else 20_011
    stride, R = _xent_geometry(m)
    assert 2 * stride * R < n < 3 * stride * R
    return n


def _split_case(m, n, seed):
    """logits, labels and sets: the sets are drawn row by row, so every wave step mixes them; ties for the maximum are
    planted in every (pass, row slot) of the grid and the tied rows walk through all six set values, so every split slot
    holds some"""
    rng = np.random.default_rng(seed)
    H = rng.standard_normal((n, m), dtype=np.float32) * np.float32(4.0)
    Y = rng.integers(0, m, n).astype(np.int64)
    S = SET_VALUES[rng.choice(len(SET_VALUES), size=n, p=SET_P)]
    _plant_ties(H, Y, m)
    tied = _slot_rows(n, m)
    for k, r in enumerate(tied):
        S[r] = SET_VALUES[k % len(SET_VALUES)]
    if m >= 2 and len(tied) >= 2 * len(SET_VALUES):
        assert set(_slot(S[tied]).tolist()) == {0, 1, 2, 3}
    return H, Y, S.astype(np.int32)


def _run_split(ctx, h_ptr, g_ptr, Yd, Sd, n, m, t, gs):
    torch = _torch()
    sums = torch.zeros(8, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.lib.mggcn_softmax_xent_split_from_f32(ctx.stream(0), h_ptr, g_ptr, Yd.data_ptr(), Sd.data_ptr(), n, m, t, gs,
                                              sums.data_ptr())
    ctx.sync()
    return sums.cpu().numpy().copy()


def _run_plain(ctx, h_ptr, g_ptr, Yd, n, m, gs):
    torch = _torch()
    sums = torch.zeros(2, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.lib.mggcn_softmax_xent_fused_from_f32(ctx.stream(0), h_ptr, g_ptr, Yd.data_ptr(), n, m, gs, sums.data_ptr())
    ctx.sync()
    return sums.cpu().numpy().copy()


def _check_split_kernel(ctx, H, Y, S, t, what):
    n, m = H.shape
    slot = _slot(S)
    train = S == t
    gs = _f32(1.0 / max(int(train.sum()), 1))
    G64, pmax, nll, amax = _xent64(H, Y, gs)
    Yd, Sd = _dev(Y.astype(np.int32).reshape(-1, 1)), _dev(S.reshape(-1, 1))
    # out of place, twice; then in place (G == logits)
    Hg, Gg = Guarded(n, m, m, 0, logical=H), Guarded(n, m, m, 0, output=True)
    s1 = _run_split(ctx, Hg.ptr, Gg.ptr, Yd, Sd, n, m, t, gs)
    b = Gg.bits()
    Gg.check_guards(f"{what}: G", b)
    Hg.check_unchanged(f"{what}: logits, out of place")
    G = Gg.values(b)
    del Gg, b
    G2 = Guarded(n, m, m, 0, output=True)
    s2 = _run_split(ctx, Hg.ptr, G2.ptr, Yd, Sd, n, m, t, gs)
    _assert_bits_equal(G2.values(), G, f"{what}: second run")
    _assert_bits_equal(s2, s1, f"{what}: sums, second run")
    del G2, Hg
    Hi = Guarded(n, m, m, 0, logical=H, output=True)
    s3 = _run_split(ctx, Hi.ptr, Hi.ptr, Yd, Sd, n, m, t, gs)
    b = Hi.bits()
    Hi.check_guards(f"{what}: in place", b)
    _assert_bits_equal(Hi.values(b), G, f"{what}: in place vs out of place")
    _assert_bits_equal(s3, s1, f"{what}: sums, in place")
    del Hi, b
    # rows outside train_set: +0.0 in every column, bit for bit
    off = G[~train].view(np.uint32)
    assert not off.any(), f"{what}: {int((off != 0).any(axis=1).sum())} row(s) outside the training set are not +0.0"
    # training rows against fp64
    if train.any():
        assert np.isfinite(G[train]).all(), what
        err = np.abs(G[train] - G64[train]).max(axis=1) / (gs * pmax[train])
        print(f"\n[splits] {what}: worst training row {err.max():.3e} of grad_scale * max p (bar 1e-4)")
        assert err.max() <= 1e-4, f"{what}: worst gradient row {err.max():.3e}, row {int(np.flatnonzero(train)[err.argmax()])}"
    correct = (amax == Y)
    for k in range(4):
        rows = slot == k
        want_c, want_l = float(correct[rows].sum()), float(nll[rows].sum())
        print(f"[splits] {what}: slot {k}: {int(rows.sum())} rows, correct {s1[2 * k + 1]:.0f} (want {want_c:.0f}), "
              f"loss sum {s1[2 * k]!r} (fp64 {want_l!r})")
        assert float(s1[2 * k + 1]) == want_c, f"{what}: slot {k}: correct count {s1[2 * k + 1]} != {want_c}"
        assert abs(float(s1[2 * k]) - want_l) <= 1e-4 * abs(want_l), f"{what}: slot {k}: loss sum {s1[2 * k]} vs {want_l}"
    return G, s1


@pytest.mark.parametrize("m", WIDTHS)
def test_split_loss_against_fp64_row_by_row(ctx, m):
    """(1) every width class of both kernels x {1 row, fewer rows than one wave step holds, two grid passes and a ragged
    third} x the three train_set values, in place and out of place, S in {0, 1, 2, 3, -1, 7}"""
    for n in (1, 3, _multipass_rows(m)):
        H, Y, S = _split_case(m, n, seed=7000 * m + n % 1000)
        for t in (0, 1, 2):
            if n == 1:
                S = np.array([t if m % 2 else (t + 1) % 3], dtype=np.int32)      # the only row trains / does not train
            _check_split_kernel(ctx, H, Y, S, t, f"split loss m={m} n={n} train_set={t}")


@pytest.mark.parametrize("m", WIDTHS)
def test_split_loss_is_anchored_to_the_plain_loss(ctx, m):
    """(2) with S == train_set everywhere the gradient and the training slot's two sums are the bits of
    mggcn_softmax_xent_fused_from_f32 and the other six sums stay +0.0; with mixed sets the four correct counts add up to
    the plain entry's count; (run-to-run bits: checked in every case of the test above)"""
    torch = _torch()
    n = _multipass_rows(m)
    H, Y, S = _split_case(m, n, seed=9000 * m + 1)
    gs = _f32(1.0 / n)
    Hd, Yd = _dev(H), _dev(Y.astype(np.int32).reshape(-1, 1))
    Gp = torch.empty_like(Hd)
    plain = _run_plain(ctx, Hd.data_ptr(), Gp.data_ptr(), Yd, n, m, gs)
    Gp = Gp.cpu().numpy()
    for t in (0, 1, 2):
        Sd = _dev(np.full((n, 1), t, dtype=np.int32))
        Gs = torch.empty_like(Hd)
        s = _run_split(ctx, Hd.data_ptr(), Gs.data_ptr(), Yd, Sd, n, m, t, gs)
        _assert_bits_equal(Gs.cpu().numpy(), Gp, f"m={m} train_set={t}: gradient vs the plain entry")
        _assert_bits_equal(s[2 * t:2 * t + 2], plain, f"m={m} train_set={t}: the training slot's sums vs the plain entry")
        rest = np.delete(s, [2 * t, 2 * t + 1])
        assert not rest.view(np.uint32).any(), f"m={m} train_set={t}: the other slots' sums are not +0.0: {s}"
        Hi = Hd.clone()
        s_in = _run_split(ctx, Hi.data_ptr(), Hi.data_ptr(), Yd, Sd, n, m, t, gs)
        _assert_bits_equal(Hi.cpu().numpy(), Gp, f"m={m} train_set={t}: in-place gradient vs the plain entry")
        _assert_bits_equal(s_in, s, f"m={m} train_set={t}: in-place sums")
    Sd = _dev(S.reshape(-1, 1))
    Gs = torch.empty_like(Hd)
    s = _run_split(ctx, Hd.data_ptr(), Gs.data_ptr(), Yd, Sd, n, m, 0, gs)
    assert float(s[1] + s[3] + s[5] + s[7]) == float(plain[1]), (s, plain)
    # the same grad_scale: the training rows carry the plain entry's bits, row by row
    Gs = Gs.cpu().numpy()
    _assert_bits_equal(Gs[S == 0], Gp[S == 0], f"m={m}: training rows of a mixed S vs the plain entry")


@pytest.mark.parametrize("m,n", [(41, 25_901), (5, 3), (1, 1), (1030, 1031)])
def test_select_rows_by_set(pkg, ctx, m, n):
    """(3) exact against numpy; 25 901 x 41 elements are two passes of the capped grid and a ragged third"""
    if n == 25_901:
        _three_passes(n * m, STREAM_THREADS, "select_rows_by_set")
    rng = np.random.default_rng(n + m)
    x = rng.standard_normal((n, m), dtype=np.float32)
    x[::7] *= np.float32(-1.0)
    S = SET_VALUES[rng.choice(len(SET_VALUES), size=n, p=SET_P)].astype(np.int32)
    for t in (0, 1, 2):
        X, Sd = pkg.dn_matrix.from_numpy(x), pkg.dn_matrix.from_numpy(S.reshape(-1, 1))
        Xg = Guarded(n, m, m, 0, logical=x, output=True)
        ctx.lib.mggcn_select_rows_by_set_f32(ctx.stream(0), Xg.ptr, Sd.buffer(), t, n * m, m)
        pkg.ops.select_rows_by_set(ctx, X, Sd, t)
        ctx.sync()
        want = np.where((S == t)[:, None], x, np.float32(0.0))
        b = Xg.bits()
        Xg.check_guards(f"select_rows_by_set m={m} n={n}", b)
        _assert_bits_equal(Xg.values(b), want, f"select_rows_by_set m={m} n={n} set={t}")
        _assert_bits_equal(X.numpy(), want, f"ops.select_rows_by_set m={m} n={n} set={t}")


@pytest.mark.parametrize("n", [_three_passes(2 * ABSSUM_ELEMS + RAGGED, ABSSUM_ELEMS, "abssum_by_set"), 100, 1])
def test_abssum_by_set(pkg, ctx, n):
    """(3) at the bar mggcn_abssum_f32 is tested at (1e-5 of the fp64 sum), slot by slot; three runs give the same bits"""
    torch = _torch()
    rng = np.random.default_rng(n % 1000)
    x = rng.standard_normal(n).astype(np.float32)
    S = SET_VALUES[rng.choice(len(SET_VALUES), size=n, p=SET_P)].astype(np.int32)
    X, Sd = _dev(x), _dev(S)
    out = []
    for _ in range(3):
        r = torch.full((4,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.lib.mggcn_abssum_by_set_f32(ctx.stream(0), X.data_ptr(), Sd.data_ptr(), n, r.data_ptr()); ctx.sync()
        out.append(r.cpu().numpy().copy())
    slot = _slot(S)
    for k in range(4):
        want = float(np.abs(x[slot == k].astype(np.float64)).sum())
        print(f"\n[splits] abssum_by_set n={n} slot {k}: {out[0][k]!r} vs fp64 {want!r} (bar 1e-5)")
        assert abs(float(out[0][k]) - want) <= 1e-5 * want
    for o in out[1:]:
        _assert_bits_equal(o, out[0], f"abssum_by_set n={n}: run to run")
    r = torch.full((4,), float("nan"), dtype=torch.float32, device="cuda")
    pkg.ops.abssum_by_set(ctx, pkg.dn_matrix.from_numpy(x.reshape(-1, 1)), pkg.dn_matrix.from_numpy(S.reshape(-1, 1)), r)
    ctx.sync()
    _assert_bits_equal(r.cpu().numpy(), out[0], f"ops.abssum_by_set n={n}")


# ---- the model ---------------------------------------------------------------------------------------------------------
N, F, HIDDEN = 1536, 20, [16, 16]
ADAM = (1e-2, 0.9, 0.999, 5e-4, 1e-8)


def _model_data(pkg, C):
    """the inputs of test_dist_gpu.py::_data, and S drawn after X and Y: 771 training rows at C = 5"""
    ip, ix, dv = pkg.datasets.synth_powerlaw_csr(N, N * 16, 700, seed=21)
    rng = np.random.default_rng(22)
    X = rng.standard_normal((N, F), dtype=np.float32)
    Y = rng.integers(0, C, size=(N, 1)).astype(np.int32)
    S = rng.choice(4, size=N, p=(0.5, 0.2, 0.25, 0.05)).astype(np.int32)
    if C == 5:
        assert int((S == 0).sum()) == 771
    return (ip, ix, dv), X, Y, S


def _gcn(pkg, csr, C, **kw):
    ip, ix, dv = csr
    return pkg.gcn(pkg.csr_matrix(ip.copy(), ix.copy(), dv.copy(), N), [F] + HIDDEN + [C], **kw)


def _oracle_split_epoch(orc, O, X, Y, S, t):
    """the issue's composition, the oracle as it is: forward, the loss over n_train, the gradient rows outside train_set
    zeroed, backward; per-split loss and accuracy in numpy from the oracle's probabilities (fp64 |log p_y|, first-maximum
    argmax)"""
    n_train = int((S == t).sum())
    H = O.forward(X)
    ls, ac, G, Pr = orc.softmax_cross_entropy(H, Y, n_global=n_train, f64acc=True)
    G[S != t] = 0
    O.G = G
    O.backward()
    y = Y.reshape(-1)
    nll = np.abs(np.log(Pr.astype(np.float64)[np.arange(len(y)), y]))
    hit = Pr.argmax(axis=1) == y
    per = {}
    for k, name in enumerate(("train", "val", "test", "other")):
        rows = _slot(S) == k
        per[name] = (float(nll[rows].sum() / rows.sum()), float(hit[rows].sum() / rows.sum()), int(rows.sum()))
    grads = [(lin.G_W.copy(), lin.G_b.copy()) for l in O.layers for lin in l.linears()]
    return per, grads


def _lins(G):
    return [lin for l in G.layers() for lin in l.linears()]


def _assert_split_epoch(what, got, per, grads, model_grads):
    for name in ("train", "val", "test", "other"):
        ol, oa, cnt = per[name]
        loss, acc = got[name]
        print(f"[splits] {what} {name}: loss {loss!r} (oracle {ol!r}), acc {acc!r} (oracle {oa!r}), {cnt} rows")
        assert abs(loss - ol) <= 1e-4 * abs(ol), (what, name, loss, ol)
        assert abs(acc - oa) <= 3.0 / cnt, (what, name, acc, oa)
        assert got["counts"][name] == cnt
    for k, ((gw, gb), (ow, ob)) in enumerate(zip(model_grads, grads)):
        assert np.abs(gw - ow).max() <= 1e-4 * np.abs(ow).max(), (what, "G_W", k, np.abs(gw - ow).max(), np.abs(ow).max())
        assert np.abs(gb - ob).max() <= 1e-4 * np.abs(ob).max(), (what, "G_b", k, np.abs(gb - ob).max(), np.abs(ob).max())


@pytest.mark.parametrize("fused,residual,C", [(True, False, 5), (False, False, 5), (True, True, 5), (False, True, 5),
                                              (True, False, 1030)])
def test_model_with_splits_matches_the_oracle(pkg, oracle, ctx, fused, residual, C):
    """(4) three epochs against oracle.Gcn(f64acc=True) with the gradient rows outside the training split zeroed, the
    parameters re-synchronised after every Adam step as in test_dist_gpu.py; residual_layer flips the loss layer's copy;
    1030 classes send fused=True down the unfused chain"""
    csr, X, Y, S = _model_data(pkg, C)
    O = oracle.Gcn(oracle.Csr(*(a.copy() for a in csr), N), [F] + HIDDEN + [C], f64acc=True, residual_layer=residual)
    G = _gcn(pkg, csr, C, fused=fused, residual_layer=residual)
    G.set_splits(S)
    assert G.loss_layer.copy == residual
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    losses = []
    for ep in range(3):
        per, grads = _oracle_split_epoch(oracle, O, X, Y, S, 0)
        O.adam_update()
        loss, acc = G.train_forward(ctx, Xd, Yd)
        got = G.split_metrics()
        assert (loss, acc) == got["train"]
        G.backward(ctx)
        ctx.sync()
        mine = [(lin.G_W.numpy().copy(), lin.G_b.numpy().copy()) for lin in _lins(G)]
        _assert_split_epoch(f"fused={fused} residual={residual} C={C} epoch {ep}", got, per, grads, mine)
        G.adam_update(ctx, *ADAM)
        ctx.sync()
        losses.append(loss)
        for lin, olin in zip(_lins(G), [lin for l in O.layers for lin in l.linears()]):
            assert np.abs(lin.W.numpy() - olin.W).max() <= 2.05e-2 and np.abs(lin.b.numpy() - olin.b).max() <= 2.05e-2
            lin.W.init(olin.W)
            lin.b.init(olin.b)
        ctx.sync()
    assert losses[-1] < losses[0], losses


@pytest.mark.parametrize("fused", [True, False])
def test_labels_outside_the_training_split_do_not_reach_the_gradient(pkg, ctx, fused):
    """(5) what makes it a mask: other valid labels on every non-training row leave every G_W and G_b and the training
    sums bitwise unchanged, and change the validation and test sums"""
    C = 5
    csr, X, Y, S = _model_data(pkg, C)
    Y2 = Y.copy()
    rng = np.random.default_rng(5)
    other = S != 0
    Y2[other] = (Y[other] + rng.integers(1, C, size=(int(other.sum()), 1))) % C
    assert (Y2[other] != Y[other]).all() and (Y2[~other] == Y[~other]).all()
    Xd = pkg.dn_matrix.from_numpy(X)
    res = []
    for labels in (Y, Y2):
        G = _gcn(pkg, csr, C, fused=fused)
        G.set_splits(S)
        G.train_forward(ctx, Xd, pkg.dn_matrix.from_numpy(labels))
        G.backward(ctx)
        ctx.sync()
        res.append(([(lin.G_W.numpy().copy(), lin.G_b.numpy().copy()) for lin in _lins(G)],
                    G.loss_layer.split_sums_host()))
    (g1, s1), (g2, s2) = res
    for k, ((w1, b1), (w2, b2)) in enumerate(zip(g1, g2)):
        _assert_bits_equal(w2, w1, f"G_W of linear {k}")
        _assert_bits_equal(b2, b1, f"G_b of linear {k}")
        assert np.abs(w1).max() > 0
    _assert_bits_equal(s2[0:2], s1[0:2], "training sums")
    assert s2[2] != s1[2] and s2[4] != s1[4], (s1, s2)          # the loss sums; a correct COUNT may come out equal by chance


@pytest.mark.parametrize("fused", [True, False])
def test_splits_off_is_the_model_without_splits(pkg, ctx, fused):
    """(6) after set_splits(None) an epoch is bitwise the epoch of a model that never had splits"""
    C = 5
    csr, X, Y, S = _model_data(pkg, C)
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    A, B = _gcn(pkg, csr, C, fused=fused), _gcn(pkg, csr, C, fused=fused)
    A.set_splits(S, train_set=1)
    A.train_forward(ctx, Xd, Yd)
    A.backward(ctx)                                   # no Adam step: the parameters are still the initial ones
    ctx.sync()
    A.set_splits(None)
    with pytest.raises(ValueError):
        A.split_metrics()
    out = []
    for G in (A, B):
        la = G.train_forward(ctx, Xd, Yd)
        G.backward(ctx)
        ctx.sync()
        grads = [(lin.G_W.numpy().copy(), lin.G_b.numpy().copy()) for lin in _lins(G)]
        G.adam_update(ctx, *ADAM)
        la2 = G.train_step(ctx, Xd, Yd, *ADAM)
        out.append((la, la2, grads, [(lin.W.numpy().copy(), lin.b.numpy().copy()) for lin in _lins(G)]))
    (la_a, la2_a, g_a, w_a), (la_b, la2_b, g_b, w_b) = out
    assert la_a == la_b and la2_a == la2_b
    for (x1, y1), (x2, y2) in zip(g_a + w_a, g_b + w_b):
        _assert_bits_equal(x1, x2, "splits off: gradient / parameter")
        _assert_bits_equal(y1, y2, "splits off: gradient / parameter")


@pytest.mark.parametrize("fused", [True, False])
def test_train_step_with_splits(pkg, ctx, fused):
    """(7) train_step = forward / backward / adam one by one, bit for bit, and split_metrics() is filled"""
    C = 5
    csr, X, Y, S = _model_data(pkg, C)
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    A, B = _gcn(pkg, csr, C, fused=fused), _gcn(pkg, csr, C, fused=fused)
    for G in (A, B):
        G.set_splits(pkg.dn_matrix.from_numpy(S.reshape(-1, 1)), train_set=0)
    for ep in range(2):
        la = A.train_forward(ctx, Xd, Yd)
        ma = A.split_metrics()
        A.backward(ctx)
        A.adam_update(ctx, *ADAM)
        ctx.sync()
        lb = B.train_step(ctx, Xd, Yd, *ADAM)
        mb = B.split_metrics()
        assert la == lb and lb == mb["train"], (ep, la, lb)
        assert ma == mb and set(mb) == {"train", "val", "test", "other", "counts"}
        assert mb["counts"] == {"train": 771, "val": 281, "test": 398, "other": 86}
        assert all(np.isfinite(mb[k]).all() for k in ("train", "val", "test", "other"))
        for la_, lb_ in zip(_lins(A), _lins(B)):
            _assert_bits_equal(la_.W.numpy(), lb_.W.numpy(), f"epoch {ep}: W")
            _assert_bits_equal(la_.b.numpy(), lb_.b.numpy(), f"epoch {ep}: b")


def test_an_empty_split_reports_nan_and_no_training_row_is_an_error(pkg, ctx):
    C = 5
    csr, X, Y, S = _model_data(pkg, C)
    G = _gcn(pkg, csr, C)
    with pytest.raises(ValueError):
        G.set_splits(np.full(N, 1, dtype=np.int32), train_set=0)
    S2 = np.where(S == 2, 1, S).astype(np.int32)                      # no test vertex
    G.set_splits(S2)
    G.train_forward(ctx, pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y))
    m = G.split_metrics()
    assert np.isnan(m["test"]).all() and np.isfinite(m["val"]).all() and m["counts"]["test"] == 0


# ---- the CLI -----------------------------------------------------------------------------------------------------------
BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mg-gcn_amd", "bin")


@pytest.mark.parametrize("args,train_set", [(["-P", "1"], 0), (["-P", "2", "-R", "1"], 0), (["-P", "1"], 2)])
def test_cli_train_set_matches_the_python_model(pkg, ctx, tmp_path, args, train_set):
    """(8) MGGCN_TRAIN_SET mg_gcn on a dataset with a mixed sets.bin: the epoch line (the training split) and the
    "[mggcn splits]" line at 1e-4 / 3 / n_split of the Python model's numbers, every epoch replayed from the weights the CLI
    started it with (MGGCN_DUMP_WEIGHTS), as test_cli_bf16_matches_the_python_model does"""
    n, F, C, E = 4096, 16, 6, 3
    ip, ix, dv = pkg.datasets.synth_powerlaw_csr(n, n * 12, 600, seed=31)
    rng = np.random.default_rng(32)
    X = rng.standard_normal((n, F), dtype=np.float32)
    Y = rng.integers(0, C, size=(n, 1)).astype(np.int32)
    Y[0, 0] = C - 1
    S = rng.choice(3, size=n, p=(0.6, 0.15, 0.25)).astype(np.int32)
    d = tmp_path / "permuted" / "synth"
    pkg.datasets.write_dataset(str(d), ip, ix, dv, X, Y, S)
    env = dict(os.environ, MGGCN_TRAIN_SET=str(train_set), MGGCN_DUMP_WEIGHTS=str(tmp_path / "w"), MGGCN_OVERSUBSCRIBE="1")
    r = subprocess.run([os.path.join(BIN, "mg_gcn")] + args + ["-E", str(E), "train", str(d), "2", "32", "32"],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stderr.strip().splitlines()[3:]
    epoch = [tuple(float(x) for x in ln.split()) for ln in lines if not ln.startswith("[")]
    splits = [ln.split() for ln in lines if ln.startswith("[mggcn splits]")]
    assert len(epoch) == E and len(splits) == E and all(len(e) == 4 for e in epoch), r.stderr[-3000:]
    P = int(args[1])
    sizes = [F, 32, 32, (C + P - 1) // P * P if "-R" in args else C]
    G = pkg.gcn(pkg.csr_matrix(ip, ix, dv, n), sizes)
    G.set_splits(S, train_set)
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    for e in range(E):
        for li, layer in enumerate(G.layers()):
            layer.W().init(pkg.datasets.read_dense(str(tmp_path / "w" / f"e{e}_W{li}.bin"), "<f4"))
            layer.b().init(pkg.datasets.read_dense(str(tmp_path / "w" / f"e{e}_b{li}.bin"), "<f4"))
        loss, acc = G.train_forward(ctx, Xd, Yd)
        m = G.split_metrics()
        assert int(epoch[e][0]) == e and abs(epoch[e][1] - loss) <= 1e-4 * abs(loss), (e, epoch[e], loss)
        assert abs(epoch[e][2] - acc) <= 3.0 / m["counts"][("train", "val", "test")[train_set]], (e, epoch[e], acc)
        w = splits[e]
        assert w[:3] == ["[mggcn", "splits]", str(e)] and w[3::3] == ["train", "val", "test"], w
        for k, name in enumerate(("train", "val", "test")):
            gl, ga = float(w[4 + 3 * k]), float(w[5 + 3 * k])
            print(f"[splits] cli {args} epoch {e} {name}: {gl} {ga} vs the Python model {m[name]}")
            assert abs(gl - m[name][0]) <= 1e-4 * abs(m[name][0]), (e, name, gl, m[name])
            assert abs(ga - m[name][1]) <= 3.0 / m["counts"][name], (e, name, ga, m[name])
    assert epoch[-1][1] < epoch[0][1]


def test_cli_without_train_set_prints_no_split_line(pkg, tmp_path):
    n, F, C = 512, 8, 3
    ip, ix, dv = pkg.datasets.synth_uniform_csr(n, 6, seed=1)
    rng = np.random.default_rng(2)
    d = tmp_path / "permuted" / "tiny"
    pkg.datasets.write_dataset(str(d), ip, ix, dv, rng.standard_normal((n, F), dtype=np.float32),
                               rng.integers(0, C, size=(n, 1)).astype(np.int32), rng.integers(0, 3, n).astype(np.int32))
    env = {k: v for k, v in os.environ.items() if k != "MGGCN_TRAIN_SET"}
    r = subprocess.run([os.path.join(BIN, "mg_gcn"), "-P", "1", "-E", "2", "train", str(d), "1", "8"], cwd=str(tmp_path),
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "[mggcn splits]" not in r.stderr and len(r.stderr.strip().splitlines()) == 5, r.stderr
