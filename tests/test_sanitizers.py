"""The engine's host-only code under AddressSanitizer + UndefinedBehaviorSanitizer and under ThreadSanitizer, on the
CPU: `make -C tests/native sanitize` builds tests/native/plan_host_test.cpp twice with plain g++ and
runs both.  Under test: the SpMM plan builders' host passes (mg-gcn_amd/csrc/plan_host.cpp -- threaded; the packed entry
streams are decoded and replayed as an SpMM against the oracle), the host preprocessing (mg-gcn_amd/csrc/host_prep.cpp
-- threaded; bit-exact against the oracle) and the per-GPU command queues of the single-process host layer
(mg-gcn_amd/host/enqueue.hpp).  Second binary, tests/native/comm_sim_test.cpp: the peer-copy transport of libmggcn_comm.so
(mg-gcn_amd/csrc/comm.cpp compiled as is) on a MODEL of HIP's stream / event semantics (tests/native/hipsim/): every rank a device
of its own, queued operations executed in random and adversarial orders, P enqueue threads under ThreadSanitizer, and mutation
runs that drop event waits (one at a time, one kind at a time) and must be noticed; the RCCL transport's multi-rank branches on a
model of RCCL's contract (a collective runs when every rank's matching call has reached the head of its stream).  Third, tests/native/abisim.cpp: the C ABI
itself as CPU loops on that model, under mg-gcn_amd/host/tests/test_dist.cpp compiled as is -- the C++ host layer's distributed
classes (enqueue threads, compute / communication streams and the event edges between them, the three exchange schedules,
dist_gcn training) with every rank on a device of its own, again under adversarial schedules, the sanitizers and wait-dropping
mutation runs.
GPU sanitizers do not exist on this pool; the device side is covered by the parity tests."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_code_is_clean_under_asan_ubsan_and_tsan():
    r = subprocess.run(["make", "-s", "-j4", "-C", os.path.join(ROOT, "tests", "native"), "sanitize"], capture_output=True, text=True,
                       timeout=1500)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert out.count("ALL PASSED") == 6, out[-4000:]                  # three binaries, once per sanitizer build
    assert out.count("TEST PASSED: host layer on the stream model") == 8 and out.count("waits the host layer's cases fail") == 5, out[-4000:]
    assert out.count("scenarios of the two transports on the stream model, 0 failed") == 2, out[-4000:]
    assert "NOT NOTICED" not in out and "DEADLOCK" not in out
    assert "TEST FAILED" not in out and "ERROR: AddressSanitizer" not in out and "WARNING: ThreadSanitizer" not in out
    assert "runtime error" not in out                                # UndefinedBehaviorSanitizer


@pytest.mark.parametrize("transport,mode,threads", [("p2p", "allgather", "1"), ("rccl", "rounds", "1"), ("rccl", "halo", "0")])
def test_cli_on_the_stream_model_matches_the_dist_oracle(pkg, oracle, tmp_path, transport, mode, threads):
    """`mg_gcn -P 4 -R 1 -E 2 train ...` -- host/main.cpp and the whole C++ host layer compiled as is over the CPU model of the C ABI
    (tests/native/abisim.cpp), four ranks on devices of their own, peer copies or the modelled RCCL, one enqueue thread per rank
    (ThreadSanitizer build) or the reference's single thread: the epoch-0 loss and accuracy equal oracle.DistGcn's at 1e-4 (classes
    padded to a multiple of P, src/main.cpp:135).  The host layer's LOGIC end to end without a GPU; the HIP kernels are the GPU
    suite's business."""
    exe = os.path.join(ROOT, "tests", "native", "_build", "mg_gcn_sim_tsan")
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "native"), exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    n, F, C, P = 1536, 24, 6, 4
    ip, ix, dv = pkg.datasets.synth_powerlaw_csr(n, n * 20, 900, seed=17)
    rng = np.random.default_rng(18)
    X = rng.standard_normal((n, F), dtype=np.float32)
    Y = rng.integers(0, C, size=(n, 1)).astype(np.int32)
    Y[0, 0] = C - 1
    d = tmp_path / "permuted" / "synth"
    pkg.datasets.write_dataset(str(d), ip, ix, dv, X, Y)
    env = dict(os.environ, MGGCN_COMM_TRANSPORT=transport, MGGCN_DIST_MODE=mode, MGGCN_ENQUEUE_THREADS=threads, HIPSIM_POLICY="0",
               HIPSIM_SEED="9", TSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, "-P", str(P), "-R", "1", "-E", "2", "train", str(d), "2", "16", "16"], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ThreadSanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stderr.strip().splitlines()
    got = [tuple(float(x) for x in ln.split()) for ln in lines if len(ln.split()) == 4 and ln.split()[0].isdigit()]
    assert [int(g[0]) for g in got] == [0, 1]
    O = oracle.DistGcn(oracle.Csr(ip, ix, dv, n), [F, 16, 16, C], P)
    want = O.train_forward(X, Y)
    assert abs(got[0][1] - want[0]) <= 1e-4 * want[0] and abs(got[0][2] - want[1]) <= 3.0 / n, (got, want)
    assert got[1][1] < got[0][1]                                      # and it trains


def test_cli_train_set_on_the_stream_model_matches_the_oracle(pkg, oracle, tmp_path):
    """MGGCN_TRAIN_SET=0 `mg_gcn` over the CPU model of the C ABI on a dataset with a mixed sets.bin, `-P 1` (gcn) and `-P 4 -R 1`
    (dist_gcn, one enqueue thread per rank under ThreadSanitizer): the C++ split-aware loss route without a GPU.  Every epoch is
    replayed from the weights the CLI started it with (MGGCN_DUMP_WEIGHTS) in oracle.Gcn of the same sizes (classes padded to a
    multiple of P with -R 1); each split's loss and accuracy come from the oracle's probabilities in numpy (fp64 |log p_y|,
    first-maximum argmax), as tests/test_gpu_splits.py::_oracle_split_epoch does.  The epoch line (the training split) and the
    "[mggcn splits]" line at the bars of the two CLI tests: 1e-4 relative on a loss, 3 / (rows of the split) on an accuracy.
    Third run: MGGCN_TRAIN_SET unset, `-P 4 -R 1`, the plain route of the same dist class, against the oracle over all vertices."""
    exe = os.path.join(ROOT, "tests", "native", "_build", "mg_gcn_sim_tsan")
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "native"), exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    n, F, C, E = 1536, 24, 6, 2
    names = ("train", "val", "test")
    ip, ix, dv = pkg.datasets.synth_powerlaw_csr(n, n * 20, 900, seed=41)
    rng = np.random.default_rng(42)
    X = rng.standard_normal((n, F), dtype=np.float32)
    Y = rng.integers(0, C, size=(n, 1)).astype(np.int32)
    Y[0, 0] = C - 1
    S = rng.choice(4, size=n, p=(0.5, 0.2, 0.25, 0.05)).astype(np.int32)          # 3: a vertex in no split
    rows = {name: S == k for k, name in enumerate(names)}
    assert all(rows[name].any() for name in names) and (S == 3).any()
    d = tmp_path / "permuted" / "synth"
    pkg.datasets.write_dataset(str(d), ip, ix, dv, X, Y, S)
    y = Y.reshape(-1)

    def run(args, train_set, tag):
        env = {k: v for k, v in os.environ.items() if k != "MGGCN_TRAIN_SET"}
        env.update(MGGCN_COMM_TRANSPORT="p2p", MGGCN_DIST_MODE="allgather", MGGCN_ENQUEUE_THREADS="1", HIPSIM_POLICY="0",
                   HIPSIM_SEED="9", TSAN_OPTIONS="halt_on_error=1", MGGCN_DUMP_WEIGHTS=str(tmp_path / tag))
        if train_set is not None:
            env["MGGCN_TRAIN_SET"] = str(train_set)
        r = subprocess.run([exe] + args + ["-E", str(E), "train", str(d), "2", "16", "16"], cwd=str(tmp_path), env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "ThreadSanitizer" not in r.stderr, r.stderr[-3000:]
        lines = r.stderr.strip().splitlines()
        epoch = [tuple(float(x) for x in ln.split()) for ln in lines if len(ln.split()) == 4 and ln.split()[0].isdigit()]
        splits = [ln.split() for ln in lines if ln.startswith("[mggcn splits]")]
        assert [int(e[0]) for e in epoch] == list(range(E)), r.stderr[-3000:]
        assert len(splits) == (E if train_set is not None else 0), r.stderr[-3000:]
        P = int(args[1])
        sizes = [F, 16, 16, (C + P - 1) // P * P if "-R" in args else C]
        O = oracle.Gcn(oracle.Csr(ip, ix, dv, n), sizes, f64acc=True)
        for e in range(E):
            for li, layer in enumerate(O.layers):
                layer.lin.W = pkg.datasets.read_dense(str(tmp_path / tag / f"e{e}_W{li}.bin"), "<f4")
                layer.lin.b = pkg.datasets.read_dense(str(tmp_path / tag / f"e{e}_b{li}.bin"), "<f4")
                assert layer.lin.W.shape == (sizes[li], sizes[li + 1]) and layer.lin.b.shape == (1, sizes[li + 1])
            Pr = oracle.softmax_cross_entropy(O.forward(X), Y, f64acc=True)[3]
            nll = np.abs(np.log(Pr.astype(np.float64)[np.arange(n), y]))
            hit = Pr.argmax(axis=1) == y
            if train_set is None:                                     # the plain route: over all vertices
                ol, oa = float(nll.sum() / n), float(hit.sum() / n)
                print(f"[sim cli] {tag} epoch {e}: {epoch[e][1:3]} vs the oracle {(ol, oa)}")
                assert abs(epoch[e][1] - ol) <= 1e-4 * abs(ol) and abs(epoch[e][2] - oa) <= 3.0 / n, (tag, e, epoch[e], ol, oa)
                continue
            per = {name: (float(nll[m].sum() / m.sum()), float(hit[m].sum() / m.sum()), int(m.sum())) for name, m in rows.items()}
            ol, oa, cnt = per[names[train_set]]
            assert abs(epoch[e][1] - ol) <= 1e-4 * abs(ol) and abs(epoch[e][2] - oa) <= 3.0 / cnt, (tag, e, epoch[e], ol, oa)
            w = splits[e]
            assert w[:3] == ["[mggcn", "splits]", str(e)] and w[3::3] == list(names), w
            for k, name in enumerate(names):
                gl, ga = float(w[4 + 3 * k]), float(w[5 + 3 * k])
                ol, oa, cnt = per[name]
                print(f"[sim cli] {tag} epoch {e} {name}: {gl} {ga} vs the oracle {(ol, oa)}, {cnt} rows")
                assert abs(gl - ol) <= 1e-4 * abs(ol), (tag, e, name, gl, ol)
                assert abs(ga - oa) <= 3.0 / cnt, (tag, e, name, ga, oa)
        assert epoch[-1][1] < epoch[0][1], (tag, epoch)              # and it trains

    run(["-P", "1"], 0, "w_p1")
    run(["-P", "4", "-R", "1"], 0, "w_p4")
    run(["-P", "4", "-R", "1"], None, "w_plain")
