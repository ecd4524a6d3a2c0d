"""bench.py's launcher side, on a machine WITHOUT a GPU (this container): plain `python bench.py --gpus 2` must start its ranks as
child processes itself -- here they fail loudly, because the product has no CPU path, and the parent relays
that: non-zero exit code, no JSON line, the engine's own message on stderr."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _no_gpu_here():
    import torch
    return not torch.cuda.is_available()


@pytest.mark.skipif(not _no_gpu_here(), reason="the point of this test is a host without a GPU")
def test_plain_bench_gpus_2_launches_its_ranks_and_relays_their_failure():
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--scale", "0.01"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0                               # the children's failure is the parent's exit code
    assert r.stdout.strip() == ""                          # no line
    # the ranks were started (the launcher reports a failed local rank) and died of the engine's own loud check, not of a launcher error
    assert "engine_error" in r.stderr and "no CPU path" in r.stderr and "local_rank" in r.stderr, r.stderr[-1500:]
    assert "must be launched with" not in r.stderr        # round 3's refusal is gone


class _Mat:
    def __init__(self, a):
        self.a = a

    def numpy(self):
        return self.a.copy()


class _Layer:
    def __init__(self, rng, n_in, n_out):
        self._W, self._b = _Mat(rng.standard_normal((n_in, n_out), dtype=np.float32)), _Mat(rng.standard_normal((1, n_out), dtype=np.float32))
        self._GW, self._Gb = _Mat(rng.standard_normal((n_in, n_out), dtype=np.float32)), _Mat(rng.standard_normal((1, n_out), dtype=np.float32))

    def W(self): return self._W
    def b(self): return self._b
    def GW(self): return self._GW
    def Gb(self): return self._Gb


def _bench_module():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_dump_outputs_writes_the_last_step_as_npy(tmp_path):
    """--dump-outputs: the last timed step's (loss, accuracy) as float64, every layer's W / b / G_W / G_b as float32, bit for bit"""
    bench = _bench_module()
    rng = np.random.default_rng(0)
    layers = [_Layer(rng, 24, 16), _Layer(rng, 16, 6)]
    names = bench.dump_outputs(str(tmp_path / "out"), (1.25, 0.5), layers)
    want = ["accuracy", "loss"] + [f"layer{i}_{k}" for i in range(2) for k in ("W", "b", "grad_W", "grad_b")]
    assert names == sorted(want)
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == sorted(n + ".npy" for n in want)
    loss, acc = np.load(tmp_path / "out" / "loss.npy"), np.load(tmp_path / "out" / "accuracy.npy")
    assert loss.dtype == np.float64 and loss.tolist() == [1.25] and acc.tolist() == [0.5]
    for i, layer in enumerate(layers):
        for k, m in (("W", layer.W()), ("b", layer.b()), ("grad_W", layer.GW()), ("grad_b", layer.Gb())):
            a = np.load(tmp_path / "out" / f"layer{i}_{k}.npy")
            assert a.dtype == np.float32 and np.array_equal(a, m.a)


def test_dump_outputs_samples_large_outputs_the_same_way_every_time(tmp_path):
    """outputs above the limit keep a fixed, seeded sample of their rows: at most the limit in all, identical from run to run"""
    bench = _bench_module()
    layers = [_Layer(np.random.default_rng(1), 512, 256), _Layer(np.random.default_rng(2), 256, 8)]
    limit = 256 << 10
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), (2.0, 0.25), layers, limit=limit)
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert sum((tmp_path / "a" / f).stat().st_size - 128 for f in files) <= limit     # 128: the .npy header
    W = np.load(tmp_path / "a" / "layer0_W.npy")
    assert W.shape[0] < 512 and W.shape[1] == 256
    rows = [np.flatnonzero((layers[0].W().a == r).all(axis=1)) for r in W]             # every kept row is a row of W, in order
    assert all(len(x) == 1 for x in rows) and np.all(np.diff([x[0] for x in rows]) > 0)
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
