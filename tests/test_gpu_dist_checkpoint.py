"""save / load on the row partition (dist_gcn, P = 2, every schedule): a resumed run is the uninterrupted P = 2 run bit for
bit on every rank, the file written at P = 2 is the file the single-GPU model writes after loading it, and a file written
by the single-GPU model under dropout and layer norm continues at P = 2 with the masks of the file's epoch counter.

Fresh spawned children share the one GPU over gloo, as in test_dist_gpu.py; a child never raises between two collectives
(its peers would wait for it): it collects what it found and reports at the end."""
import filecmp
import traceback

import numpy as np
import pytest

from test_dist_gpu import _data
from test_gpu_dist_bf16 import _init, _spawn

pytestmark = pytest.mark.gpu
ADAM = (1e-2, 0.9, 0.999, 5e-4, 1e-8)
N, P = 1024, 2
SIZES = [24, 16, 32, 16, 6]              # residual_layer=True: one residual linear where the widths differ
SEED64 = 0xFEDCBA9876543210
KW = dict(residual_layer=True, norm="layer")
LOSS_BAR = 2e-6                          # test_gpu_gcn.py:296: two runs of the same kernels
CROSS_P_BAR = 1e-4                       # tests/test_dist_gpu.py: the row partition against the single-GPU result


def _sets():
    return np.random.default_rng(5).integers(0, 3, size=N).astype(np.int32)


def _inputs():
    """test_dist_gpu._data with the features scaled to 0.1: the residual branches add un-normalised activations to the
    last layer's logits, and with N(0, 1) features the softmax saturates until a row's loss is inf"""
    pkg, graph, X, Y = _data(N, SIZES[0], SIZES[-1])
    return pkg, graph, X * np.float32(0.1), Y


def _state(pkg, G):
    out = {}
    for name, owner, p, m, v in pkg.checkpoint.model_params(G):
        out[name] = getattr(owner, p).numpy().view(np.uint32)
        if getattr(owner, m) is not None:
            out["m." + name] = getattr(owner, m).numpy().view(np.uint32)
            out["v." + name] = getattr(owner, v).numpy().view(np.uint32)
    return out


def _differences(a, b):
    return [k for k in sorted(set(a) | set(b)) if k not in a or k not in b or not np.array_equal(a[k], b[k])]


def _worker(rank, P_, port, mode, single_file, dirname, q):
    dist = _init(rank, P_, port)
    try:
        pkg, (ip, ix, dv), X, Y = _inputs()
        D = pkg.dist
        dctx = D.dist_context(device_index=0)
        A = pkg.csr_matrix(ip, ix, dv, N)
        A.normalize(True)
        A_T = A.transpose()
        p = D.partition_bounds(N, P_)
        Ad, A_Td = D.dist_row_csr_matrix(dctx, A, p, p), D.dist_row_csr_matrix(dctx, A_T, p, p)
        Xd, Yd = D.dist_row_dn_matrix(dctx, X), D.dist_row_dn_matrix(dctx, Y)
        S = _sets()[p[rank]:p[rank + 1]]

        def model():
            G = D.dist_gcn(dctx, Ad, A_Td, SIZES, mode=mode, **KW)
            G.set_splits(dctx, S)
            G.set_dropout(0.5, SEED64)
            return G

        bad, rep = [], {}
        Ga = model()
        la = [Ga.train_step(dctx, Xd, Yd, *ADAM)[0] for _ in range(6)]
        Gb = model()
        dctx.sync()
        initial = _state(pkg, Gb)
        for _ in range(3):
            Gb.train_step(dctx, Xd, Yd, *ADAM)
        Gb.save(dctx, dirname + "/b.ckpt")
        Gc = model()
        for _, owner, attr, _, _ in pkg.checkpoint.model_params(Gc):
            t = getattr(owner, attr)
            t.init(np.full(t.shape(), 123.0, dtype=np.float32))
        Gc.set_dropout(0.0)
        Gc.load(dctx, dirname + "/b.ckpt")
        lc = [Gc.train_step(dctx, Xd, Yd, *ADAM)[0] for _ in range(3)]
        dctx.sync()
        sa, sc = _state(pkg, Ga), _state(pkg, Gc)
        if _differences(sa, sc):
            bad.append(("resumed != uninterrupted", _differences(sa, sc)))
        if [k for k in initial if np.array_equal(initial[k], sc[k])]:
            bad.append(("training did not move", [k for k in initial if np.array_equal(initial[k], sc[k])]))
        if (Gc.dropout_p, Gc.dropout_seed, Gc.dropout_epoch) != (0.5, SEED64, 6) or Ga.dropout_epoch != 6:
            bad.append(("dropout state", Gc.dropout_p, Gc.dropout_seed, Gc.dropout_epoch, Ga.dropout_epoch))
        steps = [o.step for o in pkg.checkpoint.model_owners(Gc)]
        if steps != [6] * len(steps) or steps != [o.step for o in pkg.checkpoint.model_owners(Ga)]:
            bad.append(("steps", steps))
        Gc.save(dctx, dirname + "/c6.ckpt")
        rep["state"], rep["la"], rep["lc"] = sa, la, lc
        # cross-P: the single-GPU model's file continues here
        Gd = model()
        Gd.set_dropout(0.0)
        Gd.load(dctx, single_file)
        if (Gd.dropout_p, Gd.dropout_seed, Gd.dropout_epoch) != (0.5, SEED64, 2):
            bad.append(("cross-P dropout state", Gd.dropout_p, Gd.dropout_seed, Gd.dropout_epoch))
        rep["cross"] = Gd.train_step(dctx, Xd, Yd, *ADAM)[0]
        rep["cross_epoch"] = Gd.dropout_epoch
        pred = Gd.predict(dctx, Xd)
        logits = Gd(dctx, Xd).local
        dctx.sync()
        if pred.shape != (p[rank + 1] - p[rank], 1) or pred.dtype != np.int32 or \
                not np.array_equal(pred[:, 0], np.argmax(logits.numpy(), axis=1)) or Gd.dropout_epoch != 3:
            bad.append(("predict is not the argmax of the rank's rows of a plain forward",))
        q.put((rank, rep, bad, None))
    except Exception:
        q.put((rank, None, None, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def single(pkg, tmp_path_factory):
    """the single-GPU model: two epochs under dropout 0.5 and layer norm, saved; its next epoch's loss"""
    _, (ip, ix, dv), X, Y = _inputs()
    ctx = pkg.context(0)
    base = tmp_path_factory.mktemp("dist_ckpt")

    def model():
        G = pkg.gcn(pkg.csr_matrix(ip, ix, dv.copy(), N), SIZES, **KW)
        G.set_splits(_sets())
        G.set_dropout(0.5, SEED64)
        return G
    G = model()
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    for _ in range(2):
        G.train_step(ctx, Xd, Yd, *ADAM)
    path = str(base / "single.ckpt")
    G.save(ctx, path)
    return dict(ctx=ctx, model=model, path=path, next_loss=G.train_step(ctx, Xd, Yd, *ADAM)[0], base=base)


@pytest.mark.parametrize("mode", ["allgather", "halo", "rounds"])
def test_row_partition_resumes_exactly_and_shares_the_file_with_one_gpu(pkg, single, mode):
    d = single["base"] / mode
    d.mkdir()
    res = _spawn(_worker, P, (mode, single["path"], str(d)))
    for rank, rep, bad, err in res:
        assert err is None, err
        assert not bad, (rank, bad)
        print(mode, rank, "losses", rep["la"][3:], rep["lc"], "cross-P", rep["cross"], single["next_loss"])
        for a, c in zip(rep["la"][3:], rep["lc"]):
            assert abs(a - c) <= LOSS_BAR * abs(a), (rank, rep["la"], rep["lc"])
        assert np.isfinite(single["next_loss"]) and np.isfinite(rep["la"] + rep["lc"]).all()
        assert abs(rep["cross"] - single["next_loss"]) <= CROSS_P_BAR * abs(single["next_loss"]), (rank, rep["cross"])
        assert rep["cross_epoch"] == 3
    assert not _differences(res[0][1]["state"], res[1][1]["state"])              # the replicas are bitwise equal
    # the file written at P = 2 is the file the single-GPU model writes after loading it
    G = single["model"]()
    G.load(single["ctx"], str(d / "c6.ckpt"))
    G.save(single["ctx"], str(d / "one.ckpt"))
    assert filecmp.cmp(str(d / "c6.ckpt"), str(d / "one.ckpt"), shallow=False)
    cfg, tensors = pkg.datasets.read_checkpoint(str(d / "c6.ckpt"))
    assert cfg["step"] == 6 and cfg["dropout"] == (0.5, SEED64, 6) and cfg["optimizer"]
    for k, v in res[0][1]["state"].items():
        np.testing.assert_array_equal(tensors[k].view(np.uint32), v, err_msg=k)
