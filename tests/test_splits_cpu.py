"""Split-aware training, the parts that need no GPU: option checking before any device work, the padding set of
prepare_dataset, this rank's rows of sets.bin from the rank-local loader and the count all-reduce, over gloo."""
import datetime
import multiprocessing as mp
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def test_check_splits_rejects_bad_options(pkg):
    G = sys.modules[pkg.gcn.__module__]
    n = 12
    S = np.array([0, 1, 2, 3] * 3, dtype=np.int32)
    host, counts = G.check_splits(S, n, 0)
    assert host.shape == (n, 1) and host.dtype == np.int32 and counts == [3, 3, 3, 3]
    assert G.check_splits(S.astype(np.int64).reshape(n, 1), n, 2)[1] == [3, 3, 3, 3]
    assert G.split_counts(np.array([-1, 7, 0, 2, 2])) == [1, 0, 2, 2]
    for bad in (3, -1, 5, "0", None, 1.0 + 1e-9):
        with pytest.raises(ValueError, match="train_set"):
            G.check_splits(S, n, bad)
    with pytest.raises(ValueError, match="nothing to train on"):           # n_train == 0
        G.check_splits(np.where(S == 1, 3, S).astype(np.int32), n, 1)
    with pytest.raises(ValueError, match="integers"):                      # wrong length
        G.check_splits(S[:-1], n, 0)
    with pytest.raises(ValueError, match="integers"):                      # wrong dtype
        G.check_splits(S.astype(np.float32), n, 0)
    with pytest.raises(ValueError, match="integers"):                      # wrong shape
        G.check_splits(S.reshape(6, 2), n, 0)


def test_loss_layer_and_ops_check_their_splits_before_the_library(pkg):
    """host tensors: nothing here may reach the engine (there is no GPU to reach)"""
    G = sys.modules[pkg.gcn.__module__]
    n = 8
    S = pkg.dn_matrix(n, 1, dtype=np.int32, device="cpu")
    S.t[:] = 1
    layer = G.softmax_cross_entropy_loss("x_", False, True)
    with pytest.raises(ValueError, match="train_set"):
        layer.set_splits(S, [0, n, 0, 0], train_set=4)
    with pytest.raises(ValueError, match="nothing to train on"):
        layer.set_splits(S, [0, n, 0, 0], train_set=0)
    with pytest.raises(ValueError, match="nothing to train on"):
        layer.set_splits(S, None, train_set=2)                              # counted from S
    with pytest.raises(ValueError, match="int32"):
        layer.set_splits(pkg.dn_matrix(n, 1, device="cpu"), [n, 0, 0, 0])   # fp32 sets
    with pytest.raises(ValueError, match="counts"):
        layer.set_splits(S, [n, 0, 0], train_set=0)
    layer.set_splits(S, None, train_set=1)
    assert layer.counts == [0, n, 0, 0] and layer.train_set == 1
    layer.set_splits(None)
    assert layer.S is None
    H, Y = pkg.dn_matrix(n, 2000, device="cpu"), pkg.dn_matrix(n, 1, dtype=np.int32, device="cpu")
    ctx = None
    for m_bad in (H, pkg.dn_matrix(n, 0, device="cpu")):
        with pytest.raises(ValueError, match="1 <= m <= 1024"):
            pkg.ops.softmax_xent_split(ctx, m_bad, Y, S, 0, 1.0, None)
    H = pkg.dn_matrix(n, 5, device="cpu")
    with pytest.raises(ValueError, match="train_set"):
        pkg.ops.softmax_xent_split(ctx, H, Y, S, 3, 1.0, None)
    with pytest.raises(ValueError, match="sets"):
        pkg.ops.softmax_xent_split(ctx, H, Y, pkg.dn_matrix(n - 1, 1, dtype=np.int32, device="cpu"), 0, 1.0, None)
    with pytest.raises(ValueError, match="int32"):
        pkg.ops.select_rows_by_set(ctx, H, pkg.dn_matrix(n, 1, device="cpu"), 0)
    with pytest.raises(ValueError, match="n x 1"):
        pkg.ops.abssum_by_set(ctx, H, S, None)


def test_prepare_dataset_pad_set(pkg, tmp_path):
    import scipy.sparse as sp
    ds = pkg.datasets
    n0, F0, P = 13, 5, 8
    rng = np.random.default_rng(3)
    A = sp.random(n0, n0, 0.3, format="csr", random_state=4, dtype=np.float32)
    X = rng.standard_normal((n0, F0)).astype(np.float32)
    y = rng.integers(0, 4, n0)
    sets = rng.integers(0, 3, n0)
    a = ds.prepare_dataset(str(tmp_path / "a" / "g"), A, X, y, sets, P=P)
    b = ds.prepare_dataset(str(tmp_path / "b" / "g"), A, X, y, sets, P=P, pad_set=0)
    c = ds.prepare_dataset(str(tmp_path / "c" / "g"), A, X, y, sets, P=P, pad_set=3)
    for f in ("graph.bin", "features.bin", "labels.bin", "sets.bin"):
        da, db, dc = (open(os.path.join(d, f), "rb").read() for d in (a, b, c))
        assert da == db, f                                               # the default output is byte-identical
        assert (da == dc) == (f != "sets.bin"), f
    S0, S3 = ds.read_dense(os.path.join(a, "sets.bin"), "<i4").reshape(-1), ds.read_dense(os.path.join(c, "sets.bin"), "<i4").reshape(-1)
    assert S0.shape == (16,) and (S0[:n0] == sets).all() and (S0[n0:] == 0).all()
    assert (S3[:n0] == sets).all() and (S3[n0:] == 3).all()
    # permuted: the padding vertices keep their set wherever they land
    d = ds.prepare_dataset(str(tmp_path / "d" / "g"), A, X, y, sets, P=P, seed=5, pad_set=3)
    S = ds.read_dense(os.path.join(d, "sets.bin"), "<i4").reshape(-1)
    assert sorted(S.tolist()) == sorted(sets.tolist() + [3, 3, 3])
    with pytest.raises(ValueError, match="pad_set"):
        ds.prepare_dataset(str(tmp_path / "e" / "g"), A, X, y, sets, P=P, pad_set=4)


def _sets_worker(rank, P, port, dirname, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    import __graft_entry__ as ge
    pkg = ge.load_package()
    D = pkg.dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=P, timeout=datetime.timedelta(seconds=240))
    try:
        comm = D.host_comm()
        out = D.load_rank_local_host(comm, dirname)
        assert len(out) == 5                                             # the returned tuple keeps its shape
        info = out[4]
        counts = D.global_split_counts(comm, info["sets"], 0)
        try:
            D.global_split_counts(comm, np.where(info["sets"] == 2, 1, info["sets"]), 2)
            refused = False
        except ValueError:
            refused = True
        q.put((rank, info["sets"].copy(), info["p"], counts, refused))
    finally:
        dist.destroy_process_group()


def test_rank_local_sets_and_global_counts_over_gloo(pkg, tmp_path):
    """load_rank_local_host puts this rank's rows of sets.bin into info["sets"]; the four global counts come out of one
    all-reduce, the same on both ranks; rank 1 holds no training row and n_train == 0 is refused on every rank alike"""
    import scipy.sparse as sp
    P, n = 2, 64
    rng = np.random.default_rng(8)
    A = sp.random(n, n, 0.1, format="csr", random_state=9, dtype=np.float32)
    X = rng.standard_normal((n, 8)).astype(np.float32)
    y = rng.integers(0, 3, n)
    sets = rng.integers(0, 4, n)
    sets[n // 2:] = np.where(sets[n // 2:] == 0, 1, sets[n // 2:])       # no training row on rank 1
    d = pkg.datasets.prepare_dataset(str(tmp_path / "g"), A, X, y, sets, P=P)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_sets_worker, args=(r, P, port, d, q)) for r in range(P)]
    for pr in procs:
        pr.start()
    try:
        res = sorted([q.get(timeout=120) for _ in range(P)], key=lambda t: t[0])
        for pr in procs:
            pr.join(timeout=60)
            assert pr.exitcode == 0
    finally:                                  # a rank that never met the others must not outlive the test
        for pr in procs:
            if pr.is_alive():
                pr.terminate()
                pr.join(timeout=30)
    want = [int((sets == k).sum()) for k in range(3)] + [int((sets > 2).sum())]
    for rank, S, p, counts, refused in res:
        assert S.dtype == np.int32 and S.shape == (p[rank + 1] - p[rank], 1)
        np.testing.assert_array_equal(S.reshape(-1), sets[p[rank]:p[rank + 1]])
        assert counts == want and refused
    assert (res[1][1] != 0).all() and (res[0][1] == 0).any()


def test_cli_refuses_a_bad_train_set_with_one_line(tmp_path):
    """MGGCN_TRAIN_SET=5: an argument error before any device work or file is touched"""
    exe = os.path.join(ROOT, "mg-gcn_amd", "bin", "mg_gcn")
    for bad in ("5", "-1", "train", ""):
        r = subprocess.run([exe, "-P", "1", "-E", "1", "train", str(tmp_path / "missing"), "1", "8"], cwd=str(tmp_path),
                           env=dict(os.environ, MGGCN_TRAIN_SET=bad), capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and r.stdout == ""
        lines = r.stderr.strip().splitlines()
        assert len(lines) == 1 and "MGGCN_TRAIN_SET must be 0" in lines[0], r.stderr
    assert not (tmp_path / "csvs").exists()
