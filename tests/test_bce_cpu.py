"""Multi-label training, the parts that need no GPU: the host restatement of the loss (bce_ref.py) against torch, option
and target checks before any device work, and [n x C] label matrices through write_dataset / read_dataset /
prepare_dataset / prep.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bce_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_matches_torch_bce_with_logits():
    """loss and gradient of the fp64 restatement against binary_cross_entropy_with_logits (CPU, fp64, reduction="sum")
    and its autograd at 1e-12 relative, z = +-50 and +-800 included"""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(1)
    Z = (rng.standard_normal((64, 9)) * 6).astype(np.float32)
    Z[0, :4] = [50, -50, 800, -800]
    Z[1, :4] = [50, -50, 800, -800]
    T = (rng.random(Z.shape) < 0.3).astype(np.int32)
    T[0, :4], T[1, :4] = 1, 0
    z = torch.tensor(Z.astype(np.float64), requires_grad=True)
    t = torch.tensor((T != 0).astype(np.float64))
    want = F.binary_cross_entropy_with_logits(z, t, reduction="sum")
    want.backward()
    per = F.binary_cross_entropy_with_logits(z.detach(), t, reduction="none").numpy()
    got = bce_ref.loss64(Z, T)
    assert np.isfinite(got).all()
    assert np.abs(got - per).max() <= 1e-12 * np.abs(per).max()
    assert abs(got.sum() - float(want.detach())) <= 1e-12 * float(want.detach())
    g = bce_ref.grad64(Z, T, 1.0)
    assert np.abs(g - z.grad.numpy()).max() <= 1e-12 * np.abs(z.grad.numpy()).max()
    # the fp32 twin stays at fp32 rounding of the same numbers
    assert np.abs(bce_ref.loss32(Z, T) - got).max() <= 1e-6 * np.abs(got).max()
    assert np.abs(bce_ref.grad32(Z, T, 1.0) - g).max() <= 1e-6


def test_reference_special_values_and_counts():
    Z = np.array([[0.0, -0.0, np.inf, -np.inf, np.nan, 3.0, -3.0, 1e30]], dtype=np.float32)
    for tv in (0, 1):
        T = np.full(Z.shape, tv, dtype=np.int32)
        l = bce_ref.loss64(Z, T)
        assert not np.isnan(np.delete(l, 4)).any() and np.isnan(l[0, 4])
        assert l[0, 2] == (0.0 if tv else np.inf) and l[0, 3] == (np.inf if tv else 0.0)
    assert bce_ref.pred(Z).tolist() == [[False, False, True, False, False, True, False, True]]
    T = np.array([[1, 0, 1, 1, 1, 0, 1, 0]], dtype=np.int32)
    assert bce_ref.counts(Z, T)[0].tolist() == [1, 2, 4] and not bce_ref.counts(Z, T)[1:].any()
    S = np.array([7], dtype=np.int32)
    assert bce_ref.counts(Z, T, S)[3].tolist() == [1, 2, 4]
    assert np.isnan(bce_ref.micro_f1(0, 0, 0)) and bce_ref.micro_f1(1, 2, 4) == 2 / 8


def test_loss_option_and_targets_are_checked_before_device_work(pkg):
    G = sys.modules[pkg.gcn.__module__]
    assert G.check_loss("softmax") == "softmax" and G.check_loss("bce") == "bce"
    for bad in ("hinge", "BCE", None, 1):
        with pytest.raises(ValueError, match="loss"):
            G.check_loss(bad)
    with pytest.raises(ValueError, match="loss"):
        pkg.gcn(None, [8, 8, 3], loss="hinge")                     # before the graph is touched
    with pytest.raises(ValueError, match="loss"):
        pkg.dist.dist_gcn(None, None, None, [8, 4, 2], loss="hinge")
    with pytest.raises(ValueError, match="loss"):
        pkg.dist.dist_row_softmax_cross_entropy_loss("x_", False, True, loss="hinge")
    n, C = 6, 4
    good = pkg.dn_matrix(n, C, dtype=np.int32, device="cpu")
    G.check_targets("bce", good, n, C)
    G.check_targets("softmax", None, n, C)                          # the softmax loss keeps its own checks
    for bad in (pkg.dn_matrix(n, 1, dtype=np.int32, device="cpu"), pkg.dn_matrix(n, C, device="cpu"),
                pkg.dn_matrix(n + 1, C, dtype=np.int32, device="cpu"), np.zeros((n, C), dtype=np.int32)):
        with pytest.raises(ValueError, match="int32 targets"):
            G.check_targets("bce", bad, n, C)
    # the loss layer and the ops wrapper refuse before the library is called (ctx is never used)
    layer = G.sigmoid_bce_loss("x_", True, True)
    H = pkg.dn_matrix(n, C, device="cpu")
    with pytest.raises(ValueError, match="int32 targets"):
        layer(None, H, pkg.dn_matrix(n, 1, dtype=np.int32, device="cpu"))
    import torch
    sums = torch.zeros(16)
    with pytest.raises(ValueError, match="int32"):
        pkg.ops.sigmoid_bce(None, H, pkg.dn_matrix(n, C, device="cpu"), None, 0, 1.0, sums)
    with pytest.raises(ValueError, match="like the logits"):
        pkg.ops.sigmoid_bce(None, H, pkg.dn_matrix(n, C + 1, dtype=np.int32, device="cpu"), None, 0, 1.0, sums)
    with pytest.raises(ValueError, match="16 floats"):
        pkg.ops.sigmoid_bce(None, H, good, None, 0, 1.0, sums[:8])
    with pytest.raises(ValueError, match="train_set"):
        pkg.ops.sigmoid_bce(None, H, good, None, 3, 1.0, sums)
    with pytest.raises(ValueError, match="sets"):
        pkg.ops.sigmoid_bce(None, H, good, pkg.dn_matrix(n, 1, device="cpu"), 0, 1.0, sums)
    assert pkg.ops.BCE_SUMS == 16


def test_split_metrics_from_sums(pkg):
    """the host side of the layer: sixteen sums -> (loss, micro-F1) per split and the raw counts"""
    G = sys.modules[pkg.gcn.__module__]
    layer = G.sigmoid_bce_loss("x_", True, True)
    n, m = 10, 4
    S = pkg.dn_matrix(n, 1, dtype=np.int32, device="cpu")
    S.t[:] = 0
    S.t[6:] = 1
    layer.set_splits(S, None, train_set=1)
    layer._n, layer._m = n, m
    sums = np.array([12.0, 3, 1, 2, 8.0, 1, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0], dtype=np.float32)
    got = layer.split_metrics(sums)
    assert got["train"] == (12.0 / (6 * m), 2 * 3 / (2 * 3 + 1 + 2)) and got["confusion"]["train"] == (3.0, 1.0, 2.0)
    assert got["val"] == (8.0 / (4 * m), 0.5) and np.isnan(got["other"]).all()
    assert np.isnan(got["test"]).all() and got["counts"] == {"train": 6, "val": 4, "test": 0, "other": 0}
    assert layer.read(None, sums) == got["val"]
    layer.set_splits(None)
    assert layer.read(None, sums[:4], n=20) == (12.0 / (20 * m), 2 * 3 / (2 * 3 + 1 + 2))


def _graph(n, seed):
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    A = sp.random(n, n, density=0.2, random_state=seed, format="csr", dtype=np.float32)
    A.data[:] = 1
    return A, rng


def test_label_matrix_round_trips_through_the_dataset_files(pkg, tmp_path):
    ds = pkg.datasets
    n, C, P = 13, 5, 4
    A, rng = _graph(n, 3)
    X = rng.standard_normal((n, 6)).astype(np.float32)
    T = (rng.random((n, C)) < 0.3).astype(np.int32)
    T[:, 0] = np.arange(n) + 1                                       # every row recognisable (non-zero = positive)
    sets = rng.integers(0, 3, n)
    # write_dataset / read_dataset keep the matrix
    A.sort_indices()
    ds.write_dataset(str(tmp_path / "w"), A.indptr.astype(np.uint32), A.indices.astype(np.uint32), A.data, X, T, sets)
    _, X2, Y2, S2 = ds.read_dataset(str(tmp_path / "w"))
    assert Y2.shape == (n, C) and Y2.dtype == np.int32 and np.array_equal(Y2, T)
    assert S2.shape == (n, 1) and np.array_equal(S2.reshape(-1), sets)
    assert np.array_equal(ds.read_dense_rows(str(tmp_path / "w" / "labels.bin"), "<i4", 3, 9), T[3:9])
    ds.write_dataset(str(tmp_path / "w0"), A.indptr.astype(np.uint32), A.indices.astype(np.uint32), A.data, X, T)
    assert ds.read_dataset(str(tmp_path / "w0"))[3].shape == (n, 1)                 # default sets: n x 1 zeros
    # an n x 1 / 1-D input writes the bytes it always did
    for y in (np.arange(n), np.arange(n).reshape(n, 1), list(range(n))):
        ds.write_dataset(str(tmp_path / "w1"), A.indptr.astype(np.uint32), A.indices.astype(np.uint32), A.data, X, y)
        ds.write_dense(str(tmp_path / "old.bin"), np.asarray(y).reshape(-1, 1), "<u4")
        assert (tmp_path / "w1" / "labels.bin").read_bytes() == (tmp_path / "old.bin").read_bytes()
    # prepare_dataset: padding rows are all zero and in pad_set, a permutation moves the label rows with the vertices
    d0 = ds.prepare_dataset(str(tmp_path / "p" / "g"), A, X, T, sets, P=P, pad_set=3)
    _, X0, Y0, S0 = ds.read_dataset(d0)
    assert Y0.shape == (16, C) and np.array_equal(Y0[:n], T) and not Y0[n:].any() and (S0[n:] == 3).all()
    d1 = ds.prepare_dataset(str(tmp_path / "q" / "g"), A, X, T, sets, P=P, seed=7, pad_set=3)
    assert os.path.join("permuted", "g") in d1
    _, X1, Y1, S1 = ds.read_dataset(d1)
    perm = np.random.default_rng(7).permutation(16)
    assert np.array_equal(Y1, Y0[perm]) and np.array_equal(X1, X0[perm]) and np.array_equal(S1, S0[perm])
    assert sorted(Y1[:, 0].tolist()) == [0, 0, 0] + list(range(1, n + 1))
    # 1-D labels through prepare_dataset: as before
    d2 = ds.prepare_dataset(str(tmp_path / "r" / "g"), A, X, np.arange(n), sets, P=P)
    assert ds.read_dataset(d2)[2].shape == (16, 1)


def test_prep_command_line_takes_a_label_matrix(pkg, tmp_path):
    n, C = 10, 3
    rng = np.random.default_rng(4)
    edges = np.stack([np.arange(n), (np.arange(n) + 1) % n], axis=1)
    T = (rng.random((n, C)) < 0.4).astype(np.int64)
    np.save(tmp_path / "e.npy", edges)
    np.save(tmp_path / "x.npy", rng.standard_normal((n, 4)).astype(np.float32))
    np.save(tmp_path / "t.npy", T)
    np.save(tmp_path / "y.npy", np.arange(n))
    for labels, shape in (("t.npy", (12, C)), ("y.npy", (12, 1))):
        out = tmp_path / labels[0] / "g"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "mg-gcn_amd", "prep.py"), "--edges", str(tmp_path / "e.npy"),
                            "--features", str(tmp_path / "x.npy"), "--labels", str(tmp_path / labels), "--out", str(out),
                            "-P", "4", "--seed", "0", "--pad-set", "3"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        Y = pkg.datasets.read_dataset(r.stdout.splitlines()[0])[2]
        assert Y.shape == shape
        if shape[1] == C:
            assert np.array_equal(Y[:n], T) and not Y[n:].any()
