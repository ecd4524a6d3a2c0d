"""The checkpoint file without a GPU: the numpy reader and writer (datasets.write_checkpoint / read_checkpoint), the
host-only C++ twin (mg-gcn_amd/host/checkpoint.hpp) as a stand-alone program under AddressSanitizer + UBSan, and the
option checks of model_selector and of the command line that come before any device work."""
import os
import subprocess
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [24, 16, 32, 16, 6]                 # one residual linear per differing pair of widths, plain adds elsewhere
HEADER = 8 + 4 + 4 + 4 * len(SIZES) + 16 + 8 + 24 + 4       # magic .. tensor count (INTEGRATION.md "Checkpoint file")


def _state(pkg, optimizer=True, seed=0):
    """random tensors for residual + layer norm (+ optimiser section)"""
    ds = pkg.datasets
    rng = np.random.default_rng(seed)
    cfg = {"sizes": SIZES, "residual_layer": True, "norm": "layer", "loss": "bce",
           "dropout": (0.5, 0xFEDCBA9876543210, 7), "step": 3 if optimizer else 0, "optimizer": optimizer}
    tensors = {}
    for name, shape in ds.checkpoint_tensors(SIZES, True, "layer"):
        for k in (("", "m.", "v.") if optimizer else ("",)):
            tensors[k + name] = rng.standard_normal(shape, dtype=np.float32)
    tensors["W0"][0, :4] = np.array([0x7FC00001, 0x80000000, 0x00000001, 0xFF800000], dtype=np.uint32).view(np.float32)
    return cfg, tensors


def _boundaries(pkg, optimizer=True):
    """the offset at which every section of the file ends"""
    at, out = HEADER, [HEADER]
    shapes = pkg.datasets.checkpoint_tensors(SIZES, True, "layer")
    for name, (r, c) in shapes:
        for step in (4, len(name), 8, 4 * r * c):
            at += step
            out.append(at)
    if optimizer:
        for _, (r, c) in shapes:
            for _ in range(2):
                at += 4 * r * c
                out.append(at)
    return out


def _bad_files(pkg, tmp_path, good: bytes):
    """[(label, path)] of the malformed files: every strict prefix through the header, the section boundaries +- 1 through
    the payload, one trailing byte, a wrong magic, version + 1"""
    ends = _boundaries(pkg)
    assert ends[-1] == len(good)
    cuts = set(range(0, HEADER + 1))
    for e in ends:
        cuts.update(x for x in (e - 1, e, e + 1) if 0 <= x < len(good))
    cases = [(f"prefix {k}", good[:k]) for k in sorted(cuts)]
    cases.append(("trailing byte", good + b"\0"))
    cases.append(("wrong magic", b"MGGCNCKQ" + good[8:]))
    cases.append(("version + 1", good[:8] + np.array([2], dtype="<u4").tobytes() + good[12:]))
    out = []
    for k, (label, data) in enumerate(cases):
        path = tmp_path / f"bad_{k}.ckpt"
        path.write_bytes(data)
        out.append((label, str(path)))
    return out


def test_round_trip_is_bitwise_and_the_bytes_are_a_function_of_the_state(pkg, tmp_path):
    ds = pkg.datasets
    for optimizer in (True, False):
        cfg, tensors = _state(pkg, optimizer)
        a, b = str(tmp_path / f"a{optimizer}.ckpt"), str(tmp_path / f"b{optimizer}.ckpt")
        ds.write_checkpoint(a, cfg, tensors)
        ds.write_checkpoint(b, dict(cfg), {k: v.copy() for k, v in reversed(list(tensors.items()))})
        assert open(a, "rb").read() == open(b, "rb").read()
        assert os.path.getsize(a) == _boundaries(pkg, optimizer)[-1]
        got_cfg, got = ds.read_checkpoint(a)
        assert got_cfg == dict(cfg, dropout=tuple(cfg["dropout"]))
        assert sorted(got) == sorted(tensors)
        for name, want in tensors.items():
            assert got[name].dtype == np.float32 and got[name].shape == want.shape
            np.testing.assert_array_equal(got[name].view(np.uint32), want.view(np.uint32), err_msg=name)


def test_malformed_files_raise_the_format_error_naming_the_file(pkg, tmp_path):
    ds = pkg.datasets
    cfg, tensors = _state(pkg)
    good = str(tmp_path / "good.ckpt")
    ds.write_checkpoint(good, cfg, tensors)
    bad = _bad_files(pkg, tmp_path, open(good, "rb").read())
    assert len(bad) > HEADER + 3
    for label, path in bad:
        with pytest.raises(ds.format_error) as e:
            ds.read_checkpoint(path)
        assert path in str(e.value), (label, str(e.value))
    with pytest.raises(ds.format_error, match="version 2"):
        ds.read_checkpoint(bad[-1][1])


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    """the C++ reader / writer with its own main, built by plain g++ under the sanitizers; never loaded into Python"""
    exe = tmp_path_factory.mktemp("ckpt_tool") / "checkpoint_tool"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "mg-gcn_amd", "host"),
                        os.path.join(ROOT, "tests", "native", "checkpoint_tool.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return str(exe)


def _run_tool(tool, src, dst):
    return subprocess.run([tool, src, dst], capture_output=True, text=True, timeout=60,
                          env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))


def test_cpp_reader_and_writer_agree_with_numpy_byte_for_byte(pkg, tool, tmp_path):
    for optimizer in (True, False):
        cfg, tensors = _state(pkg, optimizer, seed=1)
        src, dst = str(tmp_path / f"py{optimizer}.ckpt"), str(tmp_path / f"cpp{optimizer}.ckpt")
        pkg.datasets.write_checkpoint(src, cfg, tensors)
        r = _run_tool(tool, src, dst)
        assert r.returncode == 0 and r.stderr == "", r.stderr
        assert r.stdout.split() == ["ok", str(len(tensors) // (3 if optimizer else 1)), str(int(optimizer)), str(cfg["step"])]
        assert open(src, "rb").read() == open(dst, "rb").read()


def test_cpp_reader_refuses_malformed_files_with_a_clean_sanitizer_report(pkg, tool, tmp_path):
    cfg, tensors = _state(pkg)
    good = str(tmp_path / "good.ckpt")
    pkg.datasets.write_checkpoint(good, cfg, tensors)
    for label, path in _bad_files(pkg, tmp_path, open(good, "rb").read()):
        r = _run_tool(tool, path, str(tmp_path / "out.ckpt"))
        assert r.returncode == 3, (label, r.returncode, r.stderr)
        lines = r.stderr.strip().splitlines()
        assert len(lines) == 1 and lines[0].startswith("checkpoint_error: " + path), (label, r.stderr)   # nothing from a sanitizer
    assert not os.path.exists(str(tmp_path / "out.ckpt"))


def test_model_selector_checks_its_options_before_any_device_work(pkg):
    def model(S, counts=(10, 5, 5, 0)):
        return types.SimpleNamespace(loss_layer=types.SimpleNamespace(S=S, counts=list(counts)), dropout_p=0.0)
    with pytest.raises(ValueError, match="metric"):
        pkg.model_selector(model(object()), metric="auc")
    with pytest.raises(ValueError, match="set_splits"):
        pkg.model_selector(model(None))
    with pytest.raises(ValueError, match="val"):
        pkg.model_selector(model(object(), (10, 0, 5, 0)))
    with pytest.raises(ValueError, match="patience"):
        pkg.model_selector(model(object()), patience=0)
    with pytest.raises(ValueError, match="split"):
        pkg.model_selector(model(object()), split="other")
    sel = pkg.model_selector(model(object()), metric="score", patience=2)
    assert (sel.clean, sel.stop, sel.best_epoch, sel.best_value, sel.history) == (False, False, None, None, [])
    dropped = model(object())
    dropped.dropout_p = 0.5
    assert pkg.model_selector(dropped).clean and not pkg.model_selector(dropped, clean=False).clean


def test_load_refuses_a_configuration_mismatch_by_name(pkg):
    """the comparison that gcn.load and dist_gcn.load make first, on host data alone"""
    mismatch = pkg.checkpoint.config_mismatch
    model = {"sizes": [24, 16, 16, 5], "residual_layer": False, "norm": None, "loss": "softmax"}
    assert mismatch(dict(model), model) is None
    assert mismatch(dict(model, sizes=[24, 16, 5]), model) == "sizes: file [24, 16, 5], model [24, 16, 16, 5]"
    assert mismatch(dict(model, norm="layer", loss="bce"), model) == "norm: file layer, model None"
    assert mismatch(dict(model, loss="bce"), model) == "loss: file bce, model softmax"
    assert mismatch(dict(model, residual_layer=True), model) == "residual_layer: file True, model False"


def test_cli_refuses_bad_checkpoint_and_selection_options(tmp_path):
    """one stderr line each, before any file is opened or any device is touched (the data directory does not exist)"""
    exe = os.path.join(ROOT, "mg-gcn_amd", "bin", "mg_gcn")

    def run(args, command="train", **env):
        clean = {k: v for k, v in os.environ.items() if not k.startswith("MGGCN_")}
        return subprocess.run([exe] + args + [command, str(tmp_path / "nope"), "1", "8"], cwd=str(tmp_path),
                              env=dict(clean, **env), capture_output=True, text=True, timeout=60)

    def refused(r, msg):
        assert r.returncode != 0 and msg in r.stderr, r.stderr
        assert len(r.stderr.strip().splitlines()) == 1, r.stderr
        assert not os.path.exists(str(tmp_path / "csvs"))
    for value in ("0", "x", "-1", "1.5", ""):
        refused(run([], MGGCN_PATIENCE=value, MGGCN_TRAIN_SET="0"), "MGGCN_PATIENCE must be a positive integer")
    refused(run([], MGGCN_SELECT="auc", MGGCN_TRAIN_SET="0"), "MGGCN_SELECT must be loss or score, not 'auc'")
    for var, value in (("MGGCN_PATIENCE", "2"), ("MGGCN_SELECT", "loss"), ("MGGCN_SELECT", "score"), ("MGGCN_SAVE_BEST", "best.ckpt")):
        refused(run([], **{var: value}), var + " needs MGGCN_TRAIN_SET")
    for var in ("MGGCN_LOAD", "MGGCN_SAVE", "MGGCN_SAVE_BEST", "MGGCN_PREDICTIONS"):
        refused(run([], **{var: "", "MGGCN_TRAIN_SET": "0"}), var + " must name a file")
    refused(run([], "predict"), "predict needs MGGCN_LOAD")
    refused(run(["-P", "1", "-R", "1"], "predict", MGGCN_LOAD="m.ckpt"), "predict is single-GPU only")
    refused(run(["-P", "2"], "predict", MGGCN_LOAD="m.ckpt"), "predict is single-GPU only")
    refused(run([], "bogus"), "Unknown command.")
    refused(run([], "predictx", MGGCN_LOAD="m.ckpt"), "Unknown command.")
