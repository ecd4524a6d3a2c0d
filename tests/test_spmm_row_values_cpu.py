"""The row-value instances of the float4 sweep kernels (spmm_sweep_pair_rowv_kernel, spmm_sweep_quad_lds_rowv_kernel;
csrc/spmm_sweep.hip) keep the accumulator planes in v[64:127] behind the allocator's back like the kernels they are
made from: the guards of tests/test_abi_host.py, applied to the new names, and two of their own -- the batch of the
pair kernel is one s_load_dwordx8, and no vector-memory wait stands at a run boundary in front of the value fetch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FAMILIES = ("spmm_sweep_pair_rowv_kernel", "spmm_sweep_quad_lds_rowv_kernel")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("rowv") / "sweep.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-S",
                        "--cuda-device-only", os.path.join(ROOT, "mg-gcn_amd", "csrc", "spmm_sweep.hip"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_text()


def test_row_value_kernels_keep_the_register_contract(asm):
    hi = re.compile(r"\bv(6[4-9]|[7-9][0-9]|[12][0-9][0-9])\b|v\[(6[4-9]|[7-9][0-9]|[12][0-9][0-9]):")
    kern, inside, seen = None, False, set()
    for line in asm.split("\n"):
        m = re.match(r"^(_Z\S*):", line)
        if m:
            kern = m.group(1)
        if "ASMSTART" in line:
            inside = True
            continue
        if "ASMEND" in line:
            inside = False
            continue
        if kern and any(f in kern for f in FAMILIES):
            seen.add("pair" if "pair" in kern else "quad")
            st = line.strip()
            if not inside and st and not st.startswith((".", ";")):
                assert not hi.search(st), f"{kern}: compiler-generated instruction touches a reserved register: {st}"
                assert not re.search(r"\bm0\b", st.split(";")[0]), f"{kern}: compiler-generated instruction uses m0: {st}"
    assert seen == {"pair", "quad"}
    meta = asm[asm.index("amdhsa.kernels"):]
    checked = 0
    for b in re.split(r"\n\s*- \.agpr_count:", "\n" + meta)[1:]:
        blk = ".agpr_count:" + b
        nm = re.search(r"\.name:\s+(\S+)", blk)
        if not nm or not any(f in nm.group(1) for f in FAMILIES):
            continue
        checked += 1
        assert re.search(r"\.agpr_count:\s+0\b", blk), (nm.group(1), blk[:400])
        assert re.search(r"\.vgpr_count:\s+128\b", blk), (nm.group(1), blk[:400])
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", blk), (nm.group(1), blk[:400])
    assert checked == 12, checked         # (pair<general|FAST> + quad_lds<4|8|12|16>) x B in fp32 | bf16


def test_row_value_loops_rotate_the_priority_and_load_half_the_batch(asm):
    for fam in FAMILIES:
        bodies = re.findall(r"^(_Z\S*%s[^\s:]*):[^\n]*\n(.*?)s_endpgm" % fam, asm, flags=re.S | re.M)
        assert bodies, fam
        for name, body in bodies:
            assert {int(x) for x in re.findall(r"s_setprio (\d)", body)} == {0, 1, 2, 3}, name
            assert len(re.findall(r"buffer_load_dwordx[24]\b", body)) == 4, name       # four gathers in flight, as before
            # the run's value comes out of a register the scalar loads filled: every v_readlane with a scalar lane
            # select (the row) is reached without a vector-memory wait of its own
            lines = [ln.split(";")[0].strip() for ln in body.split("\n")]
            picks = [i for i, ln in enumerate(lines) if re.match(r"v_readlane_b32 s\d+, v\d+, s\d+", ln)]
            assert picks, name
            for i in picks:
                assert not re.match(r"s_waitcnt\b.*vmcnt", lines[i - 1]), (name, lines[i - 2:i + 1])
            if "pair" in fam:
                assert re.search(r"s_load_dwordx8\b", body), name                          # a batch = eight packed words
