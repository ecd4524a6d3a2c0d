"""Version 3 of the checkpoint file (the attention models: gat, dist_gat) without a GPU: the numpy reader and writer, the
host-only C++ twin (mg-gcn_amd/host/checkpoint.hpp) as the stand-alone program tests/native/checkpoint_tool.cpp under
AddressSanitizer + UBSan, two committed fixtures that pin the layout, and the configuration comparison load makes first.
A gcn configuration still writes version 1 and reads back with the keys it always had."""
import os
import struct
import subprocess
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ckpt")
SIZES = [16, 32, 32, 5]
HEADS = [4, 2, 1]
L = len(SIZES)
# magic, version, L, sizes | residual_layer, norm, loss | model, variant, heads, attn_slope, attention dropout | optimizer |
# dropout p, seed, epoch, step | tensor count (INTEGRATION.md "Checkpoint file")
OFF_SIZES = 16
OFF_OPTIONS = OFF_SIZES + 4 * L
OFF_MODEL = OFF_OPTIONS + 12
OFF_HEADS = OFF_MODEL + 8
OFF_SLOPE = OFF_HEADS + 4 * (L - 1)
OFF_ATTN_P = OFF_SLOPE + 8
OFF_OPTIMIZER = OFF_ATTN_P + 8
HEADER = OFF_OPTIMIZER + 4 + 8 + 24 + 4
SPECIAL = np.array([0x7FC00001, 0x80000000, 0x00000001, 0xFF800000], dtype=np.uint32).view(np.float32)  # NaN, -0.0, denormal, -inf


def _config(variant, optimizer=True, sizes=SIZES, heads=HEADS):
    return {"model": "gat", "variant": variant, "sizes": list(sizes), "heads": list(heads), "attn_slope": 0.2,
            "attn_dropout": 0.3 if variant == "v1" else 0.0, "residual_layer": False, "norm": None, "loss": "softmax",
            "dropout": (0.5, 0xFEDCBA9876543210, 7), "step": 3 if optimizer else 0, "optimizer": optimizer}


def _state(pkg, variant, optimizer=True, seed=0, sizes=SIZES, heads=HEADS):
    cfg = _config(variant, optimizer, sizes, heads)
    rng = np.random.default_rng(seed)
    tensors = {}
    for name, shape in pkg.datasets.checkpoint_tensors(sizes, False, None, model="gat", variant=variant):
        for k in (("", "m.", "v.") if optimizer else ("",)):
            tensors[k + name] = rng.standard_normal(shape, dtype=np.float32)
    tensors["W0"][0, :4] = SPECIAL
    tensors["att0"][0, :4] = SPECIAL[::-1]
    return cfg, tensors


def _boundaries(pkg, variant, optimizer=True, sizes=SIZES):
    """the offset at which every section of the file ends"""
    at, out = HEADER + 4 * (len(sizes) - L) * 2, []
    out.append(at)
    shapes = pkg.datasets.checkpoint_tensors(sizes, False, None, model="gat", variant=variant)
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


def _patch(good: bytes, at: int, fmt: str, value) -> bytes:
    raw = struct.pack("<" + fmt, value)
    return good[:at] + raw + good[at + len(raw):]


def _bad_files(pkg, tmp_path, good_v1: bytes, good_v2: bytes):
    """[(label, path, what the message must contain or None)]"""
    ends = _boundaries(pkg, "v1")
    assert ends[-1] == len(good_v1)
    cuts = set(range(0, HEADER + 1))
    for e in ends:
        cuts.update(x for x in (e - 1, e, e + 1) if 0 <= x < len(good_v1))
    cases = [(f"prefix {k}", good_v1[:k], None) for k in sorted(cuts)]
    cases.append(("trailing byte", good_v1 + b"\0", "trailing"))
    cases.append(("trailing byte v2", good_v2 + b"\0", "trailing"))
    cases.append(("wrong magic", b"MGGCNCKQ" + good_v1[8:], "magic"))
    cases.append(("version 2", _patch(good_v1, 8, "I", 2), "version 2"))
    cases.append(("version 4", _patch(good_v1, 8, "I", 4), "version 4"))
    cases.append(("version 1 stamped on an attention file", _patch(good_v1, 8, "I", 1), None))
    cases.append(("model 0", _patch(good_v1, OFF_MODEL, "I", 0), "model"))
    cases.append(("model 2", _patch(good_v1, OFF_MODEL, "I", 2), "model"))
    cases.append(("variant 0", _patch(good_v1, OFF_MODEL + 4, "I", 0), "variant"))
    cases.append(("variant 3", _patch(good_v1, OFF_MODEL + 4, "I", 3), "variant"))
    cases.append(("variant 2 on a v1 body", _patch(good_v1, OFF_MODEL + 4, "I", 2), None))
    cases.append(("a head of 0", _patch(good_v1, OFF_HEADS, "I", 0), "heads"))
    cases.append(("a head of 17", _patch(good_v1, OFF_HEADS + 4, "I", 17), "heads"))
    cases.append(("a head of 2^32 - 1", _patch(good_v1, OFF_HEADS + 8, "I", 0xFFFFFFFF), "heads"))
    cases.append(("a head that does not divide", _patch(good_v1, OFF_HEADS, "I", 5), "divide"))
    cases.append(("a width of 1025", _patch(_patch(good_v1, OFF_SIZES + 4, "I", 1025), OFF_HEADS, "I", 1), "1024"))
    cases.append(("a width of 2^32 - 1", _patch(_patch(good_v2, OFF_SIZES + 8, "I", 0xFFFFFFFF), OFF_HEADS + 4, "I", 1), "1024"))
    cases.append(("residual_layer 1", _patch(good_v1, OFF_OPTIONS, "I", 1), "unknown option value"))
    cases.append(("norm 1", _patch(good_v1, OFF_OPTIONS + 4, "I", 1), "unknown option value"))
    cases.append(("norm 1 v2", _patch(good_v2, OFF_OPTIONS + 4, "I", 1), "unknown option value"))
    cases.append(("loss 2", _patch(good_v1, OFF_OPTIONS + 8, "I", 2), "unknown option value"))
    cases.append(("optimizer 2", _patch(good_v1, OFF_OPTIMIZER, "I", 2), "unknown option value"))
    cases.append(("q > 0 with variant 2", _patch(good_v2, OFF_ATTN_P, "d", 0.25), "v2"))
    cases.append(("q = 1", _patch(good_v1, OFF_ATTN_P, "d", 1.0), "attention dropout"))
    cases.append(("q = NaN", _patch(good_v1, OFF_ATTN_P, "d", float("nan")), "attention dropout"))
    cases.append(("q < 0", _patch(good_v1, OFF_ATTN_P, "d", -0.5), "attention dropout"))
    out = []
    for k, (label, data, needle) in enumerate(cases):
        path = tmp_path / f"bad_{k}.ckpt"
        path.write_bytes(data)
        out.append((label, str(path), needle))
    return out


def _good_bytes(pkg, tmp_path):
    out = []
    for variant in ("v1", "v2"):
        path = str(tmp_path / f"good_{variant}.ckpt")
        pkg.datasets.write_checkpoint(path, *_state(pkg, variant))
        out.append(open(path, "rb").read())
    return out


def test_the_offsets_of_this_file_are_the_writers(pkg, tmp_path):
    """the constants the malformed cases patch at: each field reads back from where the table says it is"""
    v1, v2 = _good_bytes(pkg, tmp_path)
    for raw, variant in ((v1, 1), (v2, 2)):
        assert raw[:8] == b"MGGCNCKP" and struct.unpack_from("<II", raw, 8) == (3, L)
        assert list(struct.unpack_from(f"<{L}I", raw, OFF_SIZES)) == SIZES
        assert struct.unpack_from("<III", raw, OFF_OPTIONS) == (0, 0, 0)
        assert struct.unpack_from("<II", raw, OFF_MODEL) == (1, variant)
        assert list(struct.unpack_from(f"<{L - 1}I", raw, OFF_HEADS)) == HEADS
        assert struct.unpack_from("<dd", raw, OFF_SLOPE) == (0.2, 0.3 if variant == 1 else 0.0)
        assert struct.unpack_from("<IdQQQI", raw, OFF_OPTIMIZER) == (1, 0.5, 0xFEDCBA9876543210, 7, 3, 3 * (L - 1))


def test_round_trip_is_bitwise_and_the_bytes_are_a_function_of_the_state(pkg, tmp_path):
    ds = pkg.datasets
    for variant in ("v1", "v2"):
        for optimizer in (True, False):
            cfg, tensors = _state(pkg, variant, optimizer)
            a, b = str(tmp_path / f"a{variant}{optimizer}.ckpt"), str(tmp_path / f"b{variant}{optimizer}.ckpt")
            ds.write_checkpoint(a, cfg, tensors)
            ds.write_checkpoint(b, dict(reversed(list(cfg.items()))), {k: v.copy() for k, v in reversed(list(tensors.items()))})
            assert open(a, "rb").read() == open(b, "rb").read()
            assert os.path.getsize(a) == _boundaries(pkg, variant, optimizer)[-1]
            got_cfg, got = ds.read_checkpoint(a)
            assert got_cfg == cfg
            assert sorted(got) == sorted(tensors)
            out = 2 if variant == "v2" else 1
            assert got["W1"].shape == (32, 32 * out) and got["b1"].shape == (1, 32 * out) and got["att1"].shape == (3 - out, 32)
            for name, want in tensors.items():
                assert got[name].dtype == np.float32 and got[name].shape == want.shape
                np.testing.assert_array_equal(got[name].view(np.uint32), want.view(np.uint32), err_msg=name)
            np.testing.assert_array_equal(got["W0"][0, :4].view(np.uint32), SPECIAL.view(np.uint32))
            np.testing.assert_array_equal(got["att0"][0, :4].view(np.uint32), SPECIAL[::-1].view(np.uint32))


def test_the_writer_refuses_what_the_reader_would(pkg, tmp_path):
    ds = pkg.datasets
    cfg, tensors = _state(pkg, "v1")
    for change in (dict(heads=[4, 2]), dict(heads=[5, 2, 1]), dict(heads=[0, 2, 1]), dict(heads=[4, 32, 1]), dict(variant="v3"),
                   dict(attn_dropout=1.0), dict(norm="layer"), dict(residual_layer=True), dict(model="sage")):
        with pytest.raises(ds.format_error):
            ds.write_checkpoint(str(tmp_path / "no.ckpt"), dict(cfg, **change), tensors)
    cfg2, tensors2 = _state(pkg, "v2")
    with pytest.raises(ds.format_error, match="v2"):
        ds.write_checkpoint(str(tmp_path / "no.ckpt"), dict(cfg2, attn_dropout=0.25), tensors2)
    with pytest.raises(ds.format_error, match="tensor W0 has"):         # v1's tensors are not v2's
        ds.write_checkpoint(str(tmp_path / "no.ckpt"), cfg2, tensors)
    assert not os.path.exists(str(tmp_path / "no.ckpt"))


def test_a_gcn_configuration_still_writes_version_1(pkg, tmp_path):
    ds = pkg.datasets
    cfg = {"sizes": SIZES, "residual_layer": True, "norm": "layer", "loss": "bce", "dropout": (0.5, 9, 7), "step": 3,
           "optimizer": True}
    rng = np.random.default_rng(4)
    assert ds.checkpoint_tensors(SIZES, True, "layer") == ds.checkpoint_tensors(SIZES, True, "layer", model="gcn", variant=None)
    tensors = {k + n: rng.standard_normal(s, dtype=np.float32) for n, s in ds.checkpoint_tensors(SIZES, True, "layer")
               for k in ("", "m.", "v.")}
    a, b = str(tmp_path / "a.ckpt"), str(tmp_path / "b.ckpt")
    ds.write_checkpoint(a, cfg, tensors)
    ds.write_checkpoint(b, dict(cfg, model="gcn"), tensors)
    raw = open(a, "rb").read()
    assert raw == open(b, "rb").read()
    assert struct.unpack_from("<I", raw, 8) == (1,)
    # version 1 has no attention block: the optimiser flag follows the loss
    assert struct.unpack_from("<IIII", raw, OFF_OPTIONS) == (1, 1, 1, 1)
    got_cfg, _ = ds.read_checkpoint(a)
    assert got_cfg == cfg and sorted(got_cfg) == sorted(cfg)


# ---- the committed fixtures --------------------------------------------------------------------------------------------------------
FIXTURES = {"gat_v1.ckpt": dict(variant="v1", optimizer=True, seed=1), "gat_v2.ckpt": dict(variant="v2", optimizer=False, seed=2)}
FIXTURE_SIZES, FIXTURE_HEADS = [3, 4, 2], [2, 1]


def _fixture_state(pkg, variant, optimizer, seed):
    return _state(pkg, variant, optimizer, seed, FIXTURE_SIZES, FIXTURE_HEADS)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_the_writer_reproduces_the_committed_fixtures(pkg, tmp_path, name):
    """tests/golden/ckpt/*.ckpt were written by write_checkpoint from _fixture_state: a change of the layout shows here"""
    want = open(os.path.join(GOLDEN, name), "rb").read()
    assert 200 <= len(want) <= 1000
    cfg, tensors = _fixture_state(pkg, **FIXTURES[name])
    path = str(tmp_path / name)
    pkg.datasets.write_checkpoint(path, cfg, tensors)
    assert open(path, "rb").read() == want
    got_cfg, got = pkg.datasets.read_checkpoint(os.path.join(GOLDEN, name))
    assert got_cfg == cfg and sorted(got) == sorted(tensors)
    for k, v in tensors.items():
        np.testing.assert_array_equal(got[k].view(np.uint32), v.view(np.uint32), err_msg=k)
    # the header, spelled out: version 3, two layers, gat, the variant, heads [2, 1], slope 0.2
    variant = 1 if FIXTURES[name]["variant"] == "v1" else 2
    assert want[:8] == b"MGGCNCKP" and struct.unpack_from("<5I", want, 8) == (3, 3, 3, 4, 2)
    assert struct.unpack_from("<3I", want, 28) == (0, 0, 0)
    assert struct.unpack_from("<4Idd", want, 40) == (1, variant, 2, 1, 0.2, 0.3 if variant == 1 else 0.0)
    assert struct.unpack_from("<IdQQQI", want, 72) == (int(FIXTURES[name]["optimizer"]), 0.5, 0xFEDCBA9876543210, 7,
                                                       3 if FIXTURES[name]["optimizer"] else 0, 6)
    assert struct.unpack_from("<I2sII", want, 112) == (2, b"W0", 3, 8 if variant == 2 else 4)


# ---- malformed files ---------------------------------------------------------------------------------------------------------------
def test_malformed_files_raise_the_format_error_naming_the_file(pkg, tmp_path):
    ds = pkg.datasets
    bad = _bad_files(pkg, tmp_path, *_good_bytes(pkg, tmp_path))
    assert len(bad) > HEADER + 20
    for label, path, needle in bad:
        with pytest.raises(ds.format_error) as e:
            ds.read_checkpoint(path)
        assert path in str(e.value), (label, str(e.value))
        assert needle is None or needle in str(e.value), (label, str(e.value))


def test_version_2_is_still_refused_by_both_kinds_of_body(pkg, tmp_path):
    """2 was never written: a version-1 body and a version-3 body stamped with it are refused alike"""
    ds = pkg.datasets
    v3 = str(tmp_path / "v3.ckpt")
    ds.write_checkpoint(v3, *_state(pkg, "v1"))
    v1 = str(tmp_path / "v1.ckpt")
    ds.write_checkpoint(v1, {"sizes": [3, 2], "loss": "softmax"}, {"W0": np.zeros((3, 2), np.float32), "b0": np.zeros((1, 2), np.float32)})
    for src in (v1, v3):
        raw = open(src, "rb").read()
        open(src, "wb").write(_patch(raw, 8, "I", 2))
        with pytest.raises(ds.format_error, match="version 2"):
            ds.read_checkpoint(src)


# ---- the C++ reader on the same files ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    """the C++ reader / writer with its own main, built by plain g++ under the sanitizers; never loaded into Python"""
    exe = tmp_path_factory.mktemp("gat_ckpt_tool") / "checkpoint_tool"
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
    for variant in ("v1", "v2"):
        for optimizer in (True, False):
            cfg, tensors = _state(pkg, variant, optimizer, seed=1)
            src, dst = str(tmp_path / f"py{variant}{optimizer}.ckpt"), str(tmp_path / f"cpp{variant}{optimizer}.ckpt")
            pkg.datasets.write_checkpoint(src, cfg, tensors)
            r = _run_tool(tool, src, dst)
            assert r.returncode == 0 and r.stderr == "", r.stderr
            assert r.stdout.split() == ["ok", str(3 * (L - 1)), str(int(optimizer)), str(cfg["step"])]
            assert open(src, "rb").read() == open(dst, "rb").read()
    for name in sorted(FIXTURES):
        dst = str(tmp_path / name)
        r = _run_tool(tool, os.path.join(GOLDEN, name), dst)
        assert r.returncode == 0 and r.stderr == "", r.stderr
        assert open(os.path.join(GOLDEN, name), "rb").read() == open(dst, "rb").read()


def test_cpp_reader_refuses_malformed_files_with_a_clean_sanitizer_report(pkg, tool, tmp_path):
    for label, path, _ in _bad_files(pkg, tmp_path, *_good_bytes(pkg, tmp_path)):
        r = _run_tool(tool, path, str(tmp_path / "out.ckpt"))
        assert r.returncode == 3, (label, r.returncode, r.stderr)
        lines = r.stderr.strip().splitlines()
        assert len(lines) == 1 and lines[0].startswith("checkpoint_error: " + path), (label, r.stderr)   # nothing from a sanitizer
    assert not os.path.exists(str(tmp_path / "out.ckpt"))


# ---- what load compares first ------------------------------------------------------------------------------------------------------
def test_load_refuses_a_configuration_mismatch_by_name(pkg):
    mismatch = pkg.checkpoint.config_mismatch
    model = {k: v for k, v in _config("v1").items() if k not in ("step", "optimizer")}
    gcn = {"sizes": SIZES, "residual_layer": False, "norm": None, "loss": "softmax"}
    assert mismatch(dict(model), model) is None
    assert mismatch(dict(model, dropout=(0.0, 0, 0), attn_dropout=0.0), model) is None      # state, not configuration
    assert mismatch(model, gcn) == "model: file gat, model gcn"
    assert mismatch(gcn, model) == "model: file gcn, model gat"
    assert mismatch(dict(model, variant="v1"), dict(model, variant="v2")) == "variant: file v1, model v2"
    assert mismatch(dict(model, heads=[4, 1]), dict(model, heads=[2, 1])) == "heads: file [4, 1], model [2, 1]"
    assert mismatch(dict(model, sizes=[16, 32, 5], heads=[4, 1]), model) == "sizes: file [16, 32, 5], model [16, 32, 32, 5]"
    assert mismatch(dict(model, attn_slope=0.1), model) == "attn_slope: file 0.1, model 0.2"
    assert mismatch(dict(model, loss="bce"), model) == "loss: file bce, model softmax"
    # the order: model, variant, sizes, heads, attn_slope, residual_layer, norm, loss
    other = dict(model, variant="v2", sizes=[16, 5], heads=[1], attn_slope=0.5, loss="bce")
    for key in ("variant", "sizes", "heads", "attn_slope", "loss"):
        assert mismatch(other, model).startswith(key + ": "), key
        other[key] = model[key]
    assert mismatch(other, model) is None
    # a gcn pair without the new keys gives the strings it always gave
    assert mismatch(dict(gcn, norm="layer", loss="bce"), gcn) == "norm: file layer, model None"


def test_the_models_have_the_members_and_the_selector_defaults_to_clean_under_attention_dropout(pkg):
    for cls in (pkg.gat, pkg.dist_gat.dist_gat):
        assert issubclass(cls, pkg.checkpoint.checkpoint_option)
        for member in ("save", "load", "predict", "checkpoint_config"):
            assert callable(getattr(cls, member))

    def model(**kw):
        return types.SimpleNamespace(loss_layer=types.SimpleNamespace(S=object(), counts=[10, 5, 5, 0]), **kw)
    assert not pkg.model_selector(model(dropout_p=0.0, attn_dropout_p=0.0)).clean
    assert pkg.model_selector(model(dropout_p=0.0, attn_dropout_p=0.3)).clean
    assert pkg.model_selector(model(dropout_p=0.5, attn_dropout_p=0.0)).clean
    assert not pkg.model_selector(model(dropout_p=0.0, attn_dropout_p=0.3), clean=False).clean
    # checkpoint_config of an attention model, on a stand-in that has what it reads
    stand_in = types.SimpleNamespace(sizes=SIZES, heads=HEADS, variant="v2", attn_slope=0.2, attn_dropout_p=0.0, loss="bce",
                                     dropout_p=0.5, dropout_seed=3, dropout_epoch=4)
    assert pkg.checkpoint.checkpoint_option.checkpoint_config(stand_in) == {
        "model": "gat", "variant": "v2", "sizes": SIZES, "heads": HEADS, "attn_slope": 0.2, "attn_dropout": 0.0,
        "residual_layer": False, "norm": None, "loss": "bce", "dropout": (0.5, 3, 4)}
