"""save / load / predict on the row partition (dist_gat at P = 1, 2, 4): a resumed run is the uninterrupted run of the same P
bit for bit on every rank and rank 0's two final files are equal byte for byte; at P = 1 the files are gat's; a gat file
loads at P = 2 and 4 and a P = 4 file loads into gat, every rank holding the file's bits afterwards; a refused load raises on
every rank alike and nobody hangs; predict returns the rank's rows of gat.predict.

Fresh spawned children share the one GPU over gloo (at most four, next to the parent), started with _init / _spawn of
test_gpu_dist_bf16.py, whose queue read is the time limit of a step.  A child never raises between two collectives (its
peers would wait for it): it collects what it found and reports at the end.  The data is test_gpu_gat_checkpoint.py's."""
import os
import sys
import traceback

import numpy as np
import pytest

from test_gpu_dist_bf16 import _init, _spawn
from test_gpu_dist_gat import TOL                      # the bar dist_gat's epochs are held to there, at every P
from test_gpu_gat_checkpoint import (ADAM, CONFIGS, HEADS, LOSS_BAR, N, SEED64, SIZES, differences, graph_256, host_state,
                                     inputs, state_bits)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("v1-both-dropouts", "v2-dropout")


def _pkg():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as ge
    return ge.load_package()


def _file_bits(pkg, path):
    return {k: v.view(np.uint32) for k, v in pkg.datasets.read_checkpoint(path)[1].items()}


def _worker(rank, P, port, single, dirname, q):
    """``single``: name -> the file gat wrote after two epochs.  Per configuration: the resume within this P (files a4, b2,
    c4 in ``dirname``), then gat's file into this P -- the bits every rank holds, the next epoch's loss, predict -- and a
    refused load (the other variant's file) between two epochs"""
    dist = _init(rank, P, port)
    try:
        pkg = _pkg()
        D = pkg.dist
        dctx = D.dist_context(overlap=True, device_index=0)
        ip, ix, dv = graph_256()
        A = pkg.csr_matrix(ip.copy(), ix.copy(), dv.copy(), N)
        p = D.partition_bounds(N, P)
        Ad, ATd = D.dist_row_csr_matrix(dctx, A, p, p, keep_rows=True), D.dist_row_csr_matrix(dctx, A.transpose(), p, p)
        X, Y, _ = inputs()
        Xd, Yd = D.dist_row_dn_matrix(dctx, X), D.dist_row_dn_matrix(dctx, Y)
        bad, rep = [], {}

        def model(seed=True, **kw):
            G = D.dist_gat(dctx, Ad, ATd, SIZES, heads=HEADS, **kw)
            if seed:
                G.set_dropout(G.dropout_p, SEED64)
            return G

        def steps(G):
            return [o.step for o in pkg.checkpoint.model_owners(G)]

        for name in NAMES:
            kw = CONFIGS[name]
            q_attn = kw.get("attn_dropout", 0.0)
            files = {k: os.path.join(dirname, f"{name}_{k}.ckpt") for k in ("a4", "b2", "c4")}
            Ga = model(**kw)
            la = [Ga.train_step(dctx, Xd, Yd, *ADAM)[0] for _ in range(4)]
            Gb = model(**kw)
            dctx.sync()
            initial = state_bits(pkg, Gb)
            for _ in range(2):
                Gb.train_step(dctx, Xd, Yd, *ADAM)
            Ga.save(dctx, files["a4"])
            Gb.save(dctx, files["b2"])
            Gc = model(seed=False, variant=kw["variant"], fused=False)
            for _, owner, attr, _, _ in pkg.checkpoint.model_params(Gc):
                t = getattr(owner, attr)
                t.init(np.full(t.shape(), 123.0, dtype=np.float32))
            Gc.load(dctx, files["b2"])
            if host_state(Gc) != (0.5, q_attn, SEED64, 2) or steps(Gc) != [2] * 6:
                bad.append((name, "state after load", host_state(Gc), steps(Gc)))
            dctx.sync()
            if differences(state_bits(pkg, Gc), state_bits(pkg, Gb)):
                bad.append((name, "loaded != saved", differences(state_bits(pkg, Gc), state_bits(pkg, Gb))))
            lc = [Gc.train_step(dctx, Xd, Yd, *ADAM)[0] for _ in range(2)]
            dctx.sync()
            sa, sc = state_bits(pkg, Ga), state_bits(pkg, Gc)
            if differences(sa, sc) or len(sc) != 27:
                bad.append((name, "resumed != uninterrupted", differences(sa, sc), len(sc)))
            if [k for k in initial if np.array_equal(initial[k], sc[k])]:
                bad.append((name, "training did not move", [k for k in initial if np.array_equal(initial[k], sc[k])]))
            if host_state(Gc) != host_state(Ga) or host_state(Gc) != (0.5, q_attn, SEED64, 4) or steps(Gc) != [4] * 6 or steps(Ga) != [4] * 6:
                bad.append((name, "state after the resumed epochs", host_state(Gc), host_state(Ga), steps(Gc)))
            Gc.save(dctx, files["c4"])
            # gat's file continues here
            Gd = model(seed=False, variant=kw["variant"])
            Gd.load(dctx, single[name])
            dctx.sync()
            if host_state(Gd) != (0.5, q_attn, SEED64, 2) or steps(Gd) != [2] * 6:
                bad.append((name, "cross-form state", host_state(Gd), steps(Gd)))
            if differences(state_bits(pkg, Gd), _file_bits(pkg, single[name])):
                bad.append((name, "the rank does not hold the file's bits", differences(state_bits(pkg, Gd), _file_bits(pkg, single[name]))))
            pred = Gd.predict(dctx, Xd)
            logits = Gd(dctx, Xd).local
            dctx.sync()
            if pred.shape != (p[rank + 1] - p[rank], 1) or pred.dtype != np.int32 or Gd.dropout_epoch != 2 or \
                    not np.array_equal(pred[:, 0], np.argmax(logits.numpy(), axis=1)):
                bad.append((name, "predict is not the argmax of the rank's rows of a plain forward"))
            # a refused load: on every rank alike, before any collective, nothing changed -- and the next epoch runs
            other = single[[n for n in NAMES if n != name][0]]
            before, host = state_bits(pkg, Gd), host_state(Gd)
            try:
                Gd.load(dctx, other)
                refusal = None
            except ValueError as e:
                refusal = str(e)
            dctx.sync()
            if differences(state_bits(pkg, Gd), before) or host_state(Gd) != host or steps(Gd) != [2] * 6:
                bad.append((name, "a refused load changed the model"))
            cross = Gd.train_step(dctx, Xd, Yd, *ADAM)[0]
            rep[name] = dict(la=la, lc=lc, state=sa, pred=pred, refusal=refusal, other=other, cross=cross, epoch=Gd.dropout_epoch)
        q.put((rank, rep, bad, None))
    except Exception:
        q.put((rank, None, None, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def single(pkg, tmp_path_factory):
    """gat on the same data: per configuration the file after two epochs, the next epoch's loss, predict from the file's
    state, and the file after four epochs"""
    base = tmp_path_factory.mktemp("dist_gat_ckpt")
    ctx = pkg.context(0)
    ip, ix, dv = graph_256()
    X, Y, _ = inputs()
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)

    def model(seed=True, **kw):
        G = pkg.gat(pkg.csr_matrix(ip.copy(), ix.copy(), dv.copy(), N), SIZES, heads=HEADS, **kw)
        if seed:
            G.set_dropout(G.dropout_p, SEED64)
        return G
    out = dict(base=base, ctx=ctx, model=model, X=Xd, Y=Yd, b2={}, a4={}, pred={}, losses={})
    for name in NAMES:
        G = model(**CONFIGS[name])
        losses = [G.train_step(ctx, Xd, Yd, *ADAM)[0] for _ in range(2)]
        out["b2"][name] = str(base / f"single_{name}_b2.ckpt")
        G.save(ctx, out["b2"][name])
        out["pred"][name] = G.predict(ctx, Xd)
        losses += [G.train_step(ctx, Xd, Yd, *ADAM)[0] for _ in range(2)]
        out["a4"][name] = str(base / f"single_{name}_a4.ckpt")
        G.save(ctx, out["a4"][name])
        out["losses"][name] = losses
    return out


def _read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("P", [1, 2, 4])
def test_row_partition_resumes_exactly_and_shares_the_file_with_gat(pkg, single, P):
    d = single["base"] / f"P{P}"
    d.mkdir()
    res = _spawn(_worker, P, (single["b2"], str(d)))
    for rank, rep, bad, err in res:
        assert err is None, err
        assert not bad, (rank, bad)
    for name in NAMES:
        files = {k: str(d / f"{name}_{k}.ckpt") for k in ("a4", "b2", "c4")}
        want = single["losses"][name]
        other_variant = "v2" if CONFIGS[name]["variant"] == "v1" else "v1"
        for rank, rep, _, _ in res:
            r = rep[name]
            print(f"[dist-gat-ckpt] P={P} rank {rank} {name}: uninterrupted {r['la']}, resumed {r['lc']}, gat {want}, "
                  f"after gat's file {r['cross']}")
            assert np.isfinite(r["la"] + r["lc"] + want).all()
            for a, c in zip(r["la"][2:], r["lc"]):
                assert abs(a - c) <= LOSS_BAR * abs(a), (rank, name, r["la"], r["lc"])
            # a refused load: the same message on every rank, naming the file and the field
            assert r["refusal"] == f"{r['other']}: variant: file {other_variant}, model {CONFIGS[name]['variant']}", (rank, r["refusal"])
            # gat's file at this P: the next epoch against gat's own third epoch
            assert abs(r["cross"] - want[2]) <= TOL * abs(want[2]), (rank, name, r["cross"], want[2])
            assert r["epoch"] == 3
            assert not differences(r["state"], res[0][1][name]["state"])            # the replicas are bitwise equal
        # rank 0's two final files
        assert _read(files["a4"]) == _read(files["c4"]) and _read(files["a4"]) != _read(files["b2"])
        cfg, tensors = pkg.datasets.read_checkpoint(files["c4"])
        assert cfg["step"] == 4 and cfg["optimizer"] and cfg["dropout"] == (0.5, SEED64, 4) and cfg["model"] == "gat"
        assert cfg["variant"] == CONFIGS[name]["variant"] and cfg["attn_dropout"] == CONFIGS[name].get("attn_dropout", 0.0)
        for k, v in res[0][1][name]["state"].items():
            np.testing.assert_array_equal(tensors[k].view(np.uint32), v, err_msg=k)
        if P == 1:                                                                  # one rank is gat, and so are its files
            assert _read(files["b2"]) == _read(single["b2"][name]) and _read(files["a4"]) == _read(single["a4"][name])
        # predict: the ranks' rows, concatenated, are gat.predict
        pred = np.concatenate([rep[name]["pred"] for _, rep, _, _ in res])
        differing = int((pred != single["pred"][name]).sum())
        print(f"[dist-gat-ckpt] P={P} {name}: predictions that differ from gat's: {differing} of {N}")
        assert pred.shape == (N, 1) and differing == 0
        # the file written at this P loads into gat: the file's bits, and gat's next epoch against this P's own
        ctx = single["ctx"]
        G = single["model"](seed=False, variant=CONFIGS[name]["variant"])
        G.load(ctx, files["b2"])
        ctx.sync()
        assert not differences(state_bits(pkg, G), {k: v.view(np.uint32) for k, v in pkg.datasets.read_checkpoint(files["b2"])[1].items()})
        assert host_state(G) == (0.5, CONFIGS[name].get("attn_dropout", 0.0), SEED64, 2)
        got = G.train_step(ctx, single["X"], single["Y"], *ADAM)[0]
        mine = res[0][1][name]["la"][2]
        print(f"[dist-gat-ckpt] P={P} {name}: gat after this P's file {got}, this P's third epoch {mine}")
        assert abs(got - mine) <= TOL * abs(mine), (name, got, mine)
