"""Which sweep tasks share a launch round (csrc/plan_host.h: "tasks in non-increasing padded length; a launch round is a
contiguous chunk of that order"), checked on the CPU by tests/native/round_order_test.cpp: a plain g++ build of the
driver against csrc/plan_host.cpp, run once.  The driver builds every case with MGGCN_SPMM_SORT_ROUNDS = 1 and = 0 in
one process and asserts sortedness, that the sorted plan is a permutation of the unsorted one (row tables and entry
sequences task by task), that the sum over the rounds of the longest task does not grow (and shrinks where the tasks
come in two classes), and that the host thread count does not change the plan."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mg-gcn_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/native/round_order_test.cpp"
    exe = str(tmp_path_factory.mktemp("round_order") / "round_order_test")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-pthread", "-I", CSRC, os.path.join(ROOT, "tests", "native", "round_order_test.cpp"),
                           os.path.join(CSRC, "plan_host.cpp"), "-o", exe])
    return exe


def test_round_order_driver(driver):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MGGCN_")}
    r = subprocess.run([driver], env=env, capture_output=True, text=True, timeout=120)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout and "FAILURE" not in r.stderr
    passed = re.findall(r"^TEST PASSED: (even rows|heavy rows) d_hint=(\d+) tasks=128 rounds=4 ", r.stdout, flags=re.M)
    assert sorted(passed) == sorted([("even rows", "0"), ("even rows", "41"), ("heavy rows", "0"), ("heavy rows", "41")])
    assert "TEST FAILED" not in r.stdout
    # the miniature has the benchmark graph's ratio: 1 820 rows over 128 tasks, and the heavy case slices rows
    assert all(int(n) > 0 for n in re.findall(r"heavy rows d_hint=\d+ .* split_rows=(\d+)", r.stdout))
