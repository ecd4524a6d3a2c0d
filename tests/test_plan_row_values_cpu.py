"""The row-value entry stream of a sweep plan (csrc/plan_host.h: SweepHost::row_values), checked on the CPU by
tests/native/row_values_test.cpp: a plain g++ build of the driver against csrc/plan_host.cpp, run once.  The driver
asserts the builder's detection, the per-task value table (sliced rows included), the padding contract, that tasks,
padded lengths, task order, rounds and the generic stream are those of a build with MGGCN_SPMM_ROW_VALUES=0, that the
row stream expands back into the generic one bit for bit, and that the host thread count does not change the plan."""
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
    assert cxx, "g++ is needed to build tests/native/row_values_test.cpp"
    exe = str(tmp_path_factory.mktemp("row_values") / "row_values_test")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-pthread", "-Wall", "-Wextra", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "row_values_test.cpp"), os.path.join(CSRC, "plan_host.cpp"), "-o", exe])
    return exe


def test_row_values_driver(driver):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MGGCN_")}
    r = subprocess.run([driver], env=env, capture_output=True, text=True, timeout=120)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout and "FAILURE" not in r.stderr
    assert "TEST FAILED" not in r.stdout
    passed = re.findall(r"^TEST PASSED: (short rows|with sliced rows) d_hint=(\d+) .* run_pad=(\d+) .* split_rows=(\d+) sliced_row_values=(\d+)$",
                        r.stdout, flags=re.M)
    assert sorted((c, d) for c, d, *_ in passed) == sorted((c, d) for c in ("short rows", "with sliced rows") for d in ("0", "16", "41"))
    for c, d, run_pad, split_rows, sliced in passed:
        assert (int(run_pad) == 2) == (d == "0"), (c, d, run_pad)                 # pairs in the wide form, groups in the narrow
        assert (int(split_rows) > 0) == (c == "with sliced rows") and (int(sliced) > 0) == (c == "with sliced rows")
    assert "TEST PASSED: column range" in r.stdout
