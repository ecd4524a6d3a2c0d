"""Dropout (mggcn_dropout_f32), the parts that need no GPU: the generator's known answers and the keep fraction of the
host restatement the GPU tests compare against, the C ABI and its binding, and the errors raised before any device work."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import dropout_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_philox_known_answers(ctr, key, want):
    assert tuple(int(w) for w in dropout_ref.philox4x32_10(ctr, key)) == want


def test_words_follow_the_counter_layout():
    """element (r, c) is word c & 3 of the call with counter (c >> 2, r low, r high, stream) and key (seed low, seed high)"""
    seed, stream, row0 = 0x0123456789ABCDEF, 77, 2 ** 32 - 2
    w = dropout_ref.words(4, 11, row0, seed, stream)
    assert w.shape == (4, 11) and w.dtype == np.uint32
    for i, c in [(0, 0), (1, 3), (2, 4), (3, 10)]:
        r = row0 + i
        one = dropout_ref.philox4x32_10((c >> 2, r & 0xFFFFFFFF, r >> 32, stream), (seed & 0xFFFFFFFF, seed >> 32))
        assert int(w[i, c]) == int(one[c & 3]), (i, c)


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_keep_fraction(p):
    n = 64 * 128
    keep = dropout_ref.mask(64, 128, 0, p, seed=0, stream=0)
    assert abs(keep.mean() - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / n), keep.mean()


def test_threshold_and_scale():
    assert dropout_ref.params(0.0) == (0, np.float32(1.0))
    assert dropout_ref.params(0.5) == (2 ** 31, np.float32(2.0))
    t, s = dropout_ref.params(0.999)
    assert t == int(np.floor(np.float64(0.999) * 2.0 ** 32)) < 2 ** 32 and s == np.float32(1.0 / (1.0 - 0.999))
    assert dropout_ref.mask(8, 8, 0, 0.0, 1, 2).all()                       # p = 0 keeps everything


def test_header_declares_the_entry_point():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mggcn.h")).read(), flags=re.S)
    decl = re.search(r"void\s+mggcn_dropout_f32\s*\(([^;]*)\);", text)
    assert decl
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == 10
    assert re.fullmatch(r"const\s+float\s*\*\s*in", args[1]) and re.fullmatch(r"float\s*\*\s*out", args[2])
    assert [a.split()[0] for a in args[3:]] == ["size_t", "size_t", "uint64_t", "uint32_t", "float", "uint64_t", "uint32_t"]
    assert re.search(r"MGGCN_ABI_VERSION\s+1\b", open(os.path.join(ROOT, "include", "mggcn.h")).read())    # an addition


def test_library_exports_and_binding_types_it(pkg):
    lib = ctypes.CDLL(pkg._lib.LIB_PATH)
    assert hasattr(lib, "mggcn_dropout_f32")
    restype, argtypes = pkg._lib.PROTOTYPES["mggcn_dropout_f32"]
    assert restype is None and len(argtypes) == 10
    assert argtypes[3:] == [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_float,
                            ctypes.c_uint64, ctypes.c_uint32]


def test_ops_dropout_parameters_match_the_restatement(pkg):
    for p in (0.0, 0.1, 0.5, 0.9, 0.999, 1.0 - 2.0 ** -40):
        t, s = pkg.ops.dropout_params(p)
        rt, rs = dropout_ref.params(p)
        assert t == rt and 0 <= t < 2 ** 32 and np.float32(s) == rs, p


@pytest.mark.parametrize("p", [1.0, -0.1, 1.5, float("nan"), float("inf"), "x"])
def test_bad_probabilities_raise_before_any_device_work(pkg, p):
    """no context, buffer or graph is touched: None stands in for all of them"""
    with pytest.raises(ValueError):
        pkg.ops.dropout(None, None, None, p, 0, 0)
    with pytest.raises(ValueError):
        pkg.gcn(None, [8, 8, 3], dropout=p)
    with pytest.raises(ValueError):
        pkg.dist.dist_gcn(None, None, None, [8, 8, 3], dropout=p)


def test_set_dropout_checks_its_arguments(pkg):
    import sys

    class model(sys.modules[pkg.gcn.__module__].dropout_option):
        def __init__(self, n_layers):
            self.layers_ = [type("layer", (), {"dropout": "unset"})() for _ in range(n_layers)]
            self._init_dropout(0.0, n_layers)
    M = model(3)
    for p in (-0.1, 1.0):
        with pytest.raises(ValueError):
            M.set_dropout(p)
    assert M.dropout_p == 0.0                                                # a refused call changes nothing
    M.set_dropout(0.25, seed=2 ** 64 + 5, epoch=3)
    assert (M.dropout_p, M.dropout_seed, M.dropout_epoch) == (0.25, 5, 3)
    M._arm_dropout(False)                                                    # a plain forward: nothing armed, no epoch spent
    assert [l.dropout for l in M.layers_] == [None] * 3 and M.dropout_epoch == 3
    M._arm_dropout(True)
    t, s = dropout_ref.params(0.25)
    assert [l.dropout for l in M.layers_] == [None, (t, float(s), 5, 3 * 64 + 1), (t, float(s), 5, 3 * 64 + 2)]
    assert M.dropout_epoch == 4
    M.set_dropout(0.0)
    M._arm_dropout(True)                                                     # p = 0: nothing armed, nothing launched
    assert [l.dropout for l in M.layers_] == [None] * 3 and M.dropout_epoch == 0
    big = model(65)
    big.set_dropout(0.0)                                                     # more than 64 layers are fine without dropout
    with pytest.raises(ValueError, match="64"):
        big.set_dropout(0.5)
    with pytest.raises(ValueError, match="64"):
        pkg.gcn(None, [4] * 67, dropout=0.5)


def test_cli_refuses_bad_dropout_options(tmp_path):
    exe = os.path.join(ROOT, "mg-gcn_amd", "bin", "mg_gcn")

    def run(args, **env):
        return subprocess.run([exe] + args + ["train", str(tmp_path / "nope"), "1", "8"], cwd=str(tmp_path),
                              env=dict(os.environ, **env), capture_output=True, text=True, timeout=60)
    for value, msg in (("1.5", "must be in [0, 1)"), ("-0.25", "must be in [0, 1)"), ("1", "must be in [0, 1)"),
                       ("x", "must be a number"), ("0.5x", "must be a number"), ("nan", "must be in [0, 1)")):
        r = run([], MGGCN_DROPOUT=value)
        assert r.returncode != 0 and "MGGCN_DROPOUT " + msg in r.stderr, (value, r.stderr)
        assert len(r.stderr.strip().splitlines()) == 1, r.stderr              # before any device work or output
    for args in (["-P", "2"], ["-P", "1", "-R", "1"]):
        r = run(args, MGGCN_DROPOUT="0.5")
        assert r.returncode != 0 and "MGGCN_DROPOUT is single-GPU only" in r.stderr, (args, r.stderr)
        assert len(r.stderr.strip().splitlines()) == 1, r.stderr
    r = run([], MGGCN_DROPOUT="0.5", MGGCN_DROPOUT_SEED="seven")
    assert r.returncode != 0 and "MGGCN_DROPOUT_SEED must be an unsigned 64-bit integer" in r.stderr, r.stderr
