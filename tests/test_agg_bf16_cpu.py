"""bf16 aggregation (mggcn_spmm_csr_bf16 / mggcn_convert_f32_bf16), the parts that need no GPU: the C ABI and its
binding, the device code of the new kernels (register contract, no scratch, the conversion instruction), the host
rounding helper the GPU tests use, and the errors raised before any device work."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from bf16_ref import bf16_bits, round_bf16, widen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NEW_FAMILIES = ("spmm_sweep_pair_b16_kernel", "spmm_sweep_quad_lds_b16_kernel")   # reserved-VGPR scheme


def test_header_declares_the_bf16_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mggcn.h")).read(), flags=re.S)
    spmm = re.search(r"void\s+mggcn_spmm_csr_bf16\s*\(([^;]*)\);", text)
    conv = re.search(r"void\s+mggcn_convert_f32_bf16\s*\(([^;]*)\);", text)
    assert spmm and conv
    assert re.search(r"const\s+uint16_t\s*\*\s*B\b", spmm.group(1)) and "const float *values" in spmm.group(1)
    assert re.search(r"uint16_t\s*\*\s*dst\b", conv.group(1)) and re.search(r"const\s+float\s*\*\s*src\b", conv.group(1))
    # the new entries are additions: the ABI version stays 1
    assert re.search(r"MGGCN_ABI_VERSION\s+1\b", open(os.path.join(ROOT, "include", "mggcn.h")).read())


def test_library_exports_and_binding_types_them(pkg):
    lib = ctypes.CDLL(pkg._lib.LIB_PATH)
    for name in ("mggcn_spmm_csr_bf16", "mggcn_convert_f32_bf16"):
        assert hasattr(lib, name), name
        assert name in pkg._lib.PROTOTYPES, name
    # same argument list as the fp32 SpMM: only B's element type differs
    assert pkg._lib.PROTOTYPES["mggcn_spmm_csr_bf16"] == pkg._lib.PROTOTYPES["mggcn_spmm_csr_f32"]
    assert len(pkg._lib.PROTOTYPES["mggcn_convert_f32_bf16"][1]) == 7
    assert pkg._lib.load().mggcn_abi_version() == 1


def _asm(tmp_path, fname):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path / (fname + ".s")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        "-S", "--cuda-device-only", os.path.join(ROOT, "mg-gcn_amd", "csrc", fname), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_text()


def _metadata(text):
    """kernel name -> its block of the amdhsa.kernels metadata"""
    meta = text[text.index("amdhsa.kernels"):]
    out = {}
    for b in re.split(r"\n\s*- \.agpr_count:", "\n" + meta)[1:]:
        blk = ".agpr_count:" + b
        nm = re.search(r"\.name:\s+(\S+)", blk)
        if nm:
            out[nm.group(1)] = blk
    return out


def test_bf16_sweep_kernels_keep_the_register_contract(tmp_path):
    """The bf16 pair / narrow kernels keep the fp32 kernels' accumulator planes in v[64:127] behind the allocator's back:
    the same guards as the fp32 ones (tests/test_abi_host.py), applied to the new names."""
    text = _asm(tmp_path, "spmm_sweep.hip")
    hi = re.compile(r"\bv(6[4-9]|[7-9][0-9]|[12][0-9][0-9])\b|v\[(6[4-9]|[7-9][0-9]|[12][0-9][0-9]):")
    kern, inside, seen = None, False, set()
    for line in text.split("\n"):
        m = re.match(r"^(_Z\S*):", line)
        if m:
            kern = m.group(1)
        if "ASMSTART" in line:
            inside = True
            continue
        if "ASMEND" in line:
            inside = False
            continue
        if kern and any(f in kern for f in NEW_FAMILIES):
            seen.add("pair" if "pair" in kern else "quad")
            st = line.strip()
            if not inside and st and not st.startswith((".", ";")):
                assert not hi.search(st), f"{kern}: compiler-generated instruction touches a reserved register: {st}"
                assert not re.search(r"\bm0\b", st.split(";")[0]), f"{kern}: compiler-generated instruction uses m0: {st}"
    assert seen == {"pair", "quad"}
    for fam in NEW_FAMILIES:
        bodies = re.findall(r"^(_Z\S*%s[^\s:]*):[^\n]*\n(.*?)s_endpgm" % fam, text, flags=re.S | re.M)
        assert bodies, fam
        for name, body in bodies:
            assert {int(x) for x in re.findall(r"s_setprio (\d)", body)} == {0, 1, 2, 3}, name
            # one dwordx2 per lane and entry pair / group: half the fp32 kernels' bytes, no dwordx4 gathers left
            assert re.search(r"buffer_load_dwordx2\b", body) and not re.search(r"buffer_load_dwordx4\b", body), name
    meta = _metadata(text)
    contract = [n for n in meta if any(f in n for f in NEW_FAMILIES)]
    assert len(contract) == 6, contract          # pair<general|FAST> + quad_lds<4|8|12|16>
    for n in contract:
        blk = meta[n]
        assert re.search(r"\.agpr_count:\s+0\b", blk), (n, blk[:400])
        assert re.search(r"\.vgpr_count:\s+128\b", blk), (n, blk[:400])


@pytest.mark.parametrize("fname", ["spmm_sweep.hip", "spmm.hip", "elementwise.hip"])
def test_every_bf16_kernel_compiles_without_scratch(tmp_path, fname):
    meta = _metadata(_asm(tmp_path, fname))
    mine = [n for n in meta if "b16" in n or "bf16" in n]
    want = {"spmm_sweep.hip": 6 + 2 + 1, "spmm.hip": 8, "elementwise.hip": 2}[fname]
    assert len(mine) == want, mine
    for n in mine:
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta[n]), (n, meta[n][:400])
        assert re.search(r"\.agpr_count:\s+0\b", meta[n]), (n, meta[n][:400])


def test_bf16_epilogues_issue_their_stores_back_to_back(tmp_path):
    """the straight-line epilogue guard of test_abi_host.py, for the bf16 pair and narrow kernels"""
    text = _asm(tmp_path, "spmm_sweep.hip")
    for pat, store_re, least in [(r"spmm_sweep_pair_b16_kernel", r"global_store_dwordx4\b", 12),
                                 (r"spmm_sweep_quad_lds_b16_kernelILi16E", r"global_store_dword\b", 48)]:
        bodies = re.findall(r"^(_Z\S*%s[^\s:]*):[^\n]*\n(.*?)s_endpgm" % pat, text, flags=re.S | re.M)
        assert bodies, pat
        for name, body in bodies:
            best = cur = 0
            for line in body.split("\n"):
                st = line.split(";")[0].strip()
                if re.match(store_re, st):
                    cur += 1
                    best = max(best, cur)
                elif re.match(r"s_waitcnt\b.*vmcnt", st):
                    cur = 0
            assert best >= least, f"{name}: longest run of stores without a vmcnt wait is {best} (< {least})"


def test_conversion_is_the_hardware_cast(tmp_path):
    """a plain cast (v_cvt_pk_bf16_f32 keeps every NaN a NaN), not integer rounding on the f32 bits"""
    text = _asm(tmp_path, "elementwise.hip")
    bodies = dict(re.findall(r"^(_Z\S*convert_f32_bf16\S*):[^\n]*\n(.*?)s_endpgm", text, flags=re.S | re.M))
    assert len(bodies) == 2
    for name, body in bodies.items():
        assert "v_cvt_pk_bf16_f32" in body, name
        assert "0x7fff" not in body.lower(), name


def test_round_bf16_helper_equals_torchs_cast():
    torch = pytest.importorskip("torch")
    specials = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, -np.nan,
                         np.finfo(np.float32).max, -np.finfo(np.float32).max, np.finfo(np.float32).tiny,
                         1e-40, -1e-40, 1e-45, 3.3895314e38, 3.3895e38], dtype=np.float32)
    # ties: the dropped half is exactly 0x8000, with even and odd kept parts; one ulp either side of a tie
    base = np.array([0x3F800000, 0x3F810000, 0x00010000, 0x00030000, 0x7F7E0000, 0x7F7F0000, 0xBF810000, 0x80030000],
                    dtype=np.uint32)
    ties = np.concatenate([base | 0x8000, base | 0x7FFF, base | 0x8001]).view(np.float32)
    nans = np.array([0x7F800001, 0xFFFFFFFF, 0x7FBFFFFF, 0xFFC00001, 0x7FFF8000], dtype=np.uint32).view(np.float32)
    rand = np.random.default_rng(0).integers(0, 2 ** 32, size=200_000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    x = np.concatenate([specials, ties, nans, rand])
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = bf16_bits(x)
    # a NaN stays a NaN; its bits are not part of the contract (torch's own vectorised and scalar casts differ there)
    nan = np.isnan(x)
    assert nan.sum() >= 7 and np.isnan(widen(want[nan])).all() and np.isnan(widen(got[nan])).all()
    np.testing.assert_array_equal(got[~nan], want[~nan])
    assert np.isnan(round_bf16(nans)).all()
    fin = np.isfinite(x)
    np.testing.assert_array_equal(widen(got)[fin], torch.from_numpy(x[fin]).to(torch.bfloat16).float().numpy())


def test_cli_refuses_bf16_with_more_than_one_gpu(tmp_path):
    exe = os.path.join(ROOT, "mg-gcn_amd", "bin", "mg_gcn")
    for args in (["-P", "2"], ["-P", "1", "-R", "1"]):
        env = dict(os.environ, MGGCN_AGG_DTYPE="bf16")
        r = subprocess.run([exe] + args + ["train", str(tmp_path / "nope"), "1", "8"], cwd=str(tmp_path), env=env,
                           capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "MGGCN_AGG_DTYPE=bf16 is single-GPU only" in r.stderr, (args, r.stderr)
        assert len(r.stderr.strip().splitlines()) == 1, r.stderr          # before any device work or output
    r = subprocess.run([exe, "train", str(tmp_path / "nope"), "1", "8"], cwd=str(tmp_path), capture_output=True, text=True,
                       env=dict(os.environ, MGGCN_AGG_DTYPE="fp8"), timeout=60)
    assert r.returncode != 0 and "must be f32 or bf16" in r.stderr


def test_python_options_are_checked_before_device_work(pkg):
    ip, ix, dv = pkg.datasets.synth_uniform_csr(64, 4, seed=1)
    A = pkg.csr_matrix(ip, ix, dv, 64)
    with pytest.raises(ValueError, match="hoist_first_aggregation"):
        pkg.gcn(A, [8, 8, 3], hoist_first_aggregation=True, agg_dtype="bf16")
    with pytest.raises(ValueError, match="agg_dtype"):
        pkg.gcn(A, [8, 8, 3], agg_dtype="fp16")
