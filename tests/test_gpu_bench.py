"""bench.py keeps its contract: exactly ONE JSON line on stdout (whatever the libraries print), with the fields the
driver reads -- at N = 1 and, as a rehearsal over gloo on one GPU, through the N > 1 code path."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUIRED = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline"}


def _one_json_line(stdout: str) -> dict:
    lines = [ln for ln in stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, f"stdout must hold one line, got {len(lines)}: {lines[:3]}"
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_single_gpu_prints_one_json_line():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--scale", "0.05", "--steps", "2", "--warmup", "1", "--full"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = _one_json_line(r.stdout)
    assert REQUIRED <= set(out) and "cpu_baseline" in out
    assert out["n_gpus"] == 1 and out["steps"] == 2 and out["warmup"] == 1 and out["higher_is_better"] is False
    assert out["value"] > 0 and abs(out["value"] - out["ms_per_step"]) < 1e-9
    rf = out["roofline"]
    assert rf["bound"] == "hbm" and rf["peak"] == 8000.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-4
    cb = out["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["loss_matches_gpu_first"] is True
    assert out["loss_first_last"][1] < out["loss_first_last"][0]
    # extra keys, never the headline: the reference's own interface on the same workload and the symmetric stand-in
    assert out["cli_epoch_ms"] > 0 and out["cli_setup_s"] >= 0 and out["cli_epochs"] == 8
    assert abs(out["cli_loss_first"] - out["loss_first_last"][0]) <= 1e-4 * out["loss_first_last"][0]   # same model, same data
    assert out["symmetric_epoch_ms"] > 0 and out["symmetric_spmm_ms_per_call"] > 0
    assert "traffic_kernel_source_current" in rf and rf["traffic"] is None      # counters exist for the full-size shape only
    assert out["hoisted_first_aggregation"]["epoch_ms"] > 0 and out["hoisted_first_aggregation"]["spmm_per_epoch"] == 6


@pytest.mark.gpu
@pytest.mark.parametrize("force_dist", [False, True], ids=["single", "dist_one_rank"])
def test_plain_bench_measures_the_headline_only(force_dist):
    """without --full the line holds the headline and what the timed epochs measured themselves (`roofline`), nothing that
    takes runs of its own: no CPU oracle, no CLI, no hoisted or symmetric epochs, no comm pass, no other piece count"""
    env = dict(os.environ)
    if force_dist:
        env.update(MGGCN_BENCH_FORCE_DIST="1", MASTER_PORT="29548", MGGCN_DIST_SELF_GATHER="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--scale", "0.05", "--steps", "2", "--warmup", "1"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = _one_json_line(r.stdout)
    assert REQUIRED <= set(out) and out["steps"] == 2 and out["warmup"] == 1 and out["value"] == out["ms_per_step"] > 0
    assert out["roofline"]["calls_timed"] > 0 and out["loss_first_last"][1] < out["loss_first_last"][0]
    moved = {"cpu_baseline", "hoisted_first_aggregation", "symmetric_epoch_ms", "comm", "alt_chunks"}
    assert not moved & set(out) and not [k for k in out if k.startswith("cli_")], sorted(out)


@pytest.mark.gpu
def test_bench_dump_outputs_holds_the_last_timed_step(tmp_path):
    """--dump-outputs DIR: --steps sets the timed steps, and DIR holds what the last of them computed -- its loss (the line's
    last loss), accuracy, and every layer's parameters and gradients, finite, float32 / float64, 64 MB at most"""
    import numpy as np
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--scale", "0.02", "--steps", "3", "--warmup", "1",
                        "--no-extras", "--no-cpu-baseline", "--dump-outputs", str(d)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = _one_json_line(r.stdout)
    sizes = out["config"]["sizes"]
    nl = len(sizes) - 1
    calls = sum(1 if i == 0 else 2 for i in range(nl) if min(sizes[i], sizes[i + 1]) == 128)     # d = 128 SpMMs per step
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["roofline"]["calls_timed"] == 3 * calls
    want = {"loss", "accuracy"} | {f"layer{i}_{k}" for i in range(nl) for k in ("W", "b", "grad_W", "grad_b")}
    assert {p.stem for p in d.iterdir()} == want and all(p.suffix == ".npy" for p in d.iterdir())
    assert sum(p.stat().st_size for p in d.iterdir()) <= 64 << 20
    arrays = {p.stem: np.load(p) for p in d.iterdir()}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrays.values())
    assert round(float(arrays["loss"][0]), 5) == out["loss_first_last"][1]
    for i in range(nl):
        assert arrays[f"layer{i}_W"].shape == arrays[f"layer{i}_grad_W"].shape == (sizes[i], sizes[i + 1])
        assert np.abs(arrays[f"layer{i}_grad_W"]).max() > 0


def _rehearsal(args, port_env=None):
    """plain `python bench.py --gpus 2 ...` -- NO launcher: bench.py starts its ranks itself"""
    env = dict(os.environ, MGGCN_BENCH_REHEARSAL="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "HSA_ENABLE_IPC_MODE_LEGACY", "MGGCN_HOST_THREADS"):
        env.pop(k, None)                                # bench.py must set what its ranks need by itself
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--scale", "0.05"] + args,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return _one_json_line(r.stdout)


@pytest.mark.gpu
def test_bench_whose_ranks_fail_still_times_the_product_cli():
    """A first contact of torch.distributed / RCCL with a node that fails must not cost the line: plain `python bench.py --gpus 2`
    whose ranks exit without one (test hook MGGCN_BENCH_FAIL_RANKS) times `mg_gcn -P 2 -R 1 ...` on the same dataset from the
    launching process and says so (`value_source`, `ranks_error`)."""
    env = dict(os.environ, MGGCN_BENCH_REHEARSAL="1", MGGCN_BENCH_FAIL_RANKS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--scale", "0.05"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    out = _one_json_line(r.stdout)
    assert REQUIRED <= set(out) and out["roofline"] is None
    assert out["n_gpus"] == 2 and out["value"] == out["cli_epoch_ms"] > 0 and out["steps"] == out["cli_epochs"] - 2
    assert "mg_gcn -P 2" in out["value_source"] and "exited with code" in out["ranks_error"]
    assert out["cli_transport"] == "p2p" and out["cli_loss_first"] > 0
    assert out["config"]["parallelism"] == "rows2-allgather" and out["config"]["sizes"][-1] % 2 == 0


@pytest.mark.gpu
def test_bench_whose_ranks_fail_after_the_timed_epochs_keeps_the_headline():
    """... and ranks that go down in the extras AFTER the timed epochs (test hook) cost only the extras: the headline rank 0 had
    parked for the launching process is printed, with `extras_error`."""
    env = dict(os.environ, MGGCN_BENCH_REHEARSAL="1", MGGCN_BENCH_FAIL_RANKS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--scale", "0.05"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    out = _one_json_line(r.stdout)
    assert REQUIRED <= set(out) and out["n_gpus"] == 2 and out["value"] > 0 and out["roofline"]["achieved"] > 0
    assert "exited with code" in out["extras_error"] and "comm" not in out and "value_source" not in out
    assert out["loss_first_last"][1] < out["loss_first_last"][0]


@pytest.mark.gpu
def test_bench_multi_rank_rehearsal_prints_one_json_line():
    out = _rehearsal(["--full"])
    assert REQUIRED <= set(out)
    assert out["n_gpus"] == 2 and out["scaling"] == "strong" and out["config"]["parallelism"].startswith("rows2")
    assert out["loss_first_last"][1] < out["loss_first_last"][0]
    # the line says what it exchanged over (the first hardware SCALE run must be self-explaining)
    comm = out["comm"]
    assert comm["backend"] == "gloo" and comm["world_size"] == 2 and comm["rehearsal_gloo_on_one_gpu"] is True
    assert [d["rank"] for d in comm["devices"]] == [0, 1] and all("name" in d and "device" in d for d in comm["devices"])
    assert comm["mode"] == "allgather" and comm["overlap"] is True and "rccl_version" in comm
    assert comm["exchange_ms"] > 0 and comm["exposed_ms"] >= 0 and comm["overlap_frac"] is not None
    assert comm["chunks"] == 2 and out["alt_chunks"]["chunks"] == 4 and out["alt_chunks"]["epoch_ms"] > 0      # the other piece count, same run
    # the PRODUCT path next to it: `mg_gcn -P 2 -R 1 train <the same files>` after the ranks have let go of the GPU
    # (two ranks wrapped over this box's one GPU: peer-copy transport, one enqueue thread per rank)
    assert out["cli_epoch_ms"] > 0 and out["cli_epochs"] == 8 and out["cli_setup_s"] >= 0
    assert out["cli_transport"] == "p2p" and out["cli_enqueue_threads"] == 1
    assert out["cli_host_issue_ms"] > 0 and out["cli_rank0_spmm_ms_per_epoch"] > 0 and out["cli_rank0_gemm_ms_per_epoch"] > 0
    assert out["cli_rank0_spmm_ms_per_epoch"] < out["cli_epoch_ms"] * 1.05            # rank 0's SpMM timers of one epoch fit in the epoch
    # same data, same seed-99 parameters, same padded class count: the two forms start at the same loss
    assert abs(out["cli_loss_first"] - out["loss_first_last"][0]) <= 1e-4 * out["loss_first_last"][0]


@pytest.mark.gpu
def test_bench_rehearsal_schedules_are_within_2x_of_each_other():
    """with a one-epoch warm-up the three exchange schedules must already be in steady state -- the round-3
    rehearsals showed the all-gather schedule at 4x the others (gloo's list-form all_gather, not plan builds:
    profiles/experiments/gloo_allgather_r04.log; fixed in dist.gloo_all_gather_rows)."""
    ms = {mode: _rehearsal(["--mode", mode, "--no-extras"])["value"] for mode in ("allgather", "rounds", "halo")}
    assert max(ms.values()) <= 2.0 * min(ms.values()), ms


@pytest.mark.gpu
def test_bench_distributed_path_over_rccl_with_one_rank():
    """The N > 1 code path of bench.py -- process group over the REAL backend (nccl = RCCL, device_id), rank-local
    dataset load through device-staged host collectives, dist_gcn with the K-piece all-gather on ProcessGroupNCCL work
    handles, the comm report (all_gather_object, RCCL version, the exchange-event pass) -- with the one rank a one-GPU
    box allows (MGGCN_BENCH_FORCE_DIST=1).  What it cannot show is a second rank; what it does show is that nothing on
    that path is gloo-only."""
    env = dict(os.environ, MGGCN_BENCH_FORCE_DIST="1", MASTER_PORT="29549", MGGCN_DIST_SELF_GATHER="1")   # one rank: exchange anyway
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--scale", "0.05", "--full"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out = _one_json_line(r.stdout)
    assert REQUIRED <= set(out) and out["n_gpus"] == 1 and out["config"]["parallelism"] == "rows1-allgather"
    comm = out["comm"]
    assert comm["backend"] == "nccl" and comm["world_size"] == 1 and comm["rehearsal_gloo_on_one_gpu"] is False
    assert comm["rccl_version"] and comm["devices"][0]["device"] == 0 and "gfx950" in comm["devices"][0]["arch"]
    assert comm["exchange_ms"] >= 0 and comm["exposed_ms"] >= 0
    assert out["loss_first_last"][1] < out["loss_first_last"][0]
    # the CLI legs of the N > 1 line, here with the one rank: RCCL from the rank's enqueue thread, the peer-copy transport,
    # and the reference's one-thread form -- all three at the Python form's first loss
    for leg, transport, threads in (("cli", "rccl", 1), ("cli_p2p", "p2p", 1), ("cli_serial", "rccl", 0), ("cli_p2p_push", "p2p-push", 1)):
        assert out[f"{leg}_epoch_ms"] > 0 and out[f"{leg}_transport"] == transport and out[f"{leg}_enqueue_threads"] == threads, out
        assert abs(out[f"{leg}_loss_first"] - out["loss_first_last"][0]) <= 1e-4 * out["loss_first_last"][0]
