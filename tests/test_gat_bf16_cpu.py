"""bf16 gathers of the attention models (gat(agg_dtype="bf16"); include/mggcn.h: mggcn_gat*_bf16), the parts that need no
GPU: the twelve entries are declared, bound with their twins' arity and exported; a wrong agg_dtype, the GATv2 export under
bf16 and a wrong operand of an ops wrapper are refused before any device work; and the three new translation units keep
every instantiation free of scratch and spills."""
import ctypes
import os
import re
from importlib import import_module

import numpy as np
import pytest

from test_agg_bf16_cpu import _asm, _metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = ([f"mggcn_gat_{c}{d}_bf16" for d in ("", "_drop") for c in ("forward", "backward_dst", "backward_src")]
           + [f"mggcn_{k}_{c}_bf16" for k in ("gatv2", "gatdot") for c in ("forward", "backward_dst", "backward_src")])
# the gathered operands of every entry: const uint16_t * there, const float * in the twin
GATHERED = {"gat_forward": ["Z"], "gat_backward_dst": ["Z"], "gat_backward_src": ["G"],
            "gatv2_forward": ["Zs"], "gatv2_backward_dst": ["Zs"], "gatv2_backward_src": ["Zd", "G"],
            "gatdot_forward": ["Zk", "Zv"], "gatdot_backward_dst": ["Zk", "Zv"], "gatdot_backward_src": ["Zq", "G"]}


def _params(text, name):
    m = re.search(r"\bvoid\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, f"{name} is not declared in include/mggcn.h"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_the_twelve_entries_are_declared_bound_and_exported(pkg):
    assert len(ENTRIES) == 12 and sorted(ENTRIES) == sorted(pkg._lib.GAT_BF16_ENTRIES)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mggcn.h")).read(), flags=re.S)
    lib = ctypes.CDLL(pkg._lib.LIB_PATH)
    for name in ENTRIES:
        twin = name[:-len("bf16")] + "f32"
        mine, theirs = _params(text, name), _params(text, twin)
        gathered = GATHERED[name[len("mggcn_"):-len("_bf16")].replace("_drop", "")]
        # the twin's argument list, with the gathered operands as images and nothing else changed
        want = [p.replace("const float *", "const uint16_t *") if p.split("*")[-1].strip() in gathered else p for p in theirs]
        assert mine == want, (name, mine, want)
        assert sum("uint16_t" in p for p in mine) == len(gathered), (name, mine)
        restype, argtypes = pkg._lib.PROTOTYPES[name]
        assert restype is None and len(argtypes) == len(mine), name
        assert pkg._lib.PROTOTYPES[name] == pkg._lib.PROTOTYPES[twin]
        assert hasattr(lib, name), name
    assert pkg._lib.load().mggcn_abi_version() == 1
    for name in ("gat_forward", "gat_backward_dst", "gat_backward_src", "gatv2_forward", "gatv2_backward_dst",
                 "gatv2_backward_src", "gatdot_forward", "gatdot_backward_dst", "gatdot_backward_src"):
        assert callable(getattr(pkg.ops, name + "_bf16")), name
    for rec in ("mggcn_gat_backward_src_rec_bf16", "mggcn_gatv2_backward_src_rec_bf16", "mggcn_gatv2_alpha_bf16"):
        assert not hasattr(lib, rec) and rec not in pkg._lib.PROTOTYPES          # no record form, no export


def _tiny(pkg, n=8):
    return pkg.csr_matrix(np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32), np.ones(n, dtype=np.float32), n)


@pytest.mark.parametrize("variant", ["v1", "v2", "dot"])
def test_a_wrong_agg_dtype_is_refused_before_any_device_work(pkg, variant):
    gcn = import_module(pkg.__name__ + ".gcn")
    with pytest.raises(ValueError) as mine:
        pkg.gat(_tiny(pkg), [16, 32, 5], variant=variant, agg_dtype="fp16")
    with pytest.raises(ValueError) as theirs:
        gcn._check_agg_dtype("fp16")
    assert str(mine.value) == str(theirs.value) and "agg_dtype" in str(mine.value)
    gat = import_module(pkg.__name__ + ".gat")
    for cls, args in ((gat.attention, ("0_", 8, 8, 32, 4)), (gat.attention_v2, ("0_", 8, 32, 4)), (gat.attention_dot, ("0_", 8, 32, 4))):
        with pytest.raises(ValueError, match="agg_dtype"):
            cls(*args, agg_dtype="fp16")


def _stand_in(pkg, variant, agg_dtype):
    gat = import_module(pkg.__name__ + ".gat")
    G = gat.gat.__new__(gat.gat)
    G.variant, G.agg_dtype, G.layers_, G.heads = variant, agg_dtype, [], [4, 1]
    return gat, G


def test_the_v2_export_is_refused_under_bf16(pkg):
    """attention_weights, gatv2_layer.alpha and attention_v2.alpha name agg_dtype with None in the place of the context; a
    v1 model with bf16 and a GATv2 model with f32 get past the refusal (to the checks that follow it)"""
    gat, G = _stand_in(pkg, "v2", "bf16")
    with pytest.raises(ValueError, match="agg_dtype"):
        G.attention_weights(None, None)
    attn = gat.attention_v2.__new__(gat.attention_v2)
    attn.agg_dtype = "bf16"
    with pytest.raises(ValueError, match="agg_dtype"):
        attn.alpha(None, None, None, None)
    layer = gat.gatv2_layer.__new__(gat.gatv2_layer)
    layer.name, layer.H, layer.attn = "0_", object(), attn
    with pytest.raises(ValueError, match="agg_dtype"):
        layer.alpha(None)
    for variant, agg_dtype in (("v1", "bf16"), ("v2", "f32")):
        _, ok = _stand_in(pkg, variant, agg_dtype)
        with pytest.raises(ValueError, match="out of range"):             # the first check after the refusals
            ok.attention_weights(None, None, layers=[0])
    attn.agg_dtype = "f32"
    layer.H = None
    with pytest.raises(ValueError, match="no forward has run"):
        layer.alpha(None)
    v1 = gat.gat_layer.__new__(gat.gat_layer)
    v1.name, v1.H, v1.attn = "0_", None, gat.attention.__new__(gat.attention)
    v1.attn.agg_dtype = "bf16"
    with pytest.raises(ValueError, match="no forward has run"):
        v1.alpha(None)


def test_defaults_own_nothing(pkg):
    gat = import_module(pkg.__name__ + ".gat")
    for cls in (gat.attention, gat.attention_v2, gat.attention_dot):
        a = cls.__new__(cls)
        assert a.agg_dtype == "f32" and a.Z16 is None and a.G16 is None
    assert gat.gat.Z_image_buffer is None and gat.gat.G_image_buffer is None


def test_ops_refuse_bad_operands_before_the_library(pkg):
    """the wrappers raise ValueError on stand-ins that own no device memory: an fp32 operand where an image belongs, an image
    where an fp32 operand belongs, and images of the wrong shape"""
    import torch

    class M:
        def __init__(self, n, m): self.N, self.Mm = n, m
        def n(self): return self.N
        def m(self): return self.Mm
        def shape(self): return (self.N, self.Mm)
        def buffer(self): raise AssertionError("the library must not be reached")

    class I(pkg.ops.bf16_image):
        def buffer(self): raise AssertionError("the library must not be reached")

    img = lambda n, m: I(torch.zeros((n, m), dtype=torch.int16))
    ops = pkg.ops
    F = _tiny(pkg)
    with pytest.raises(ValueError, match="2-byte"):
        ops.bf16_image(torch.zeros((8, 32), dtype=torch.float32))
    with pytest.raises(ValueError, match="2-D"):
        ops.bf16_image(torch.zeros(8, dtype=torch.int16))
    assert img(8, 96).columns(32, 64).shape() == (8, 32) and img(8, 96).columns(32, 64).ld() == 96
    # an fp32 matrix where an image belongs, in every wrapper
    image = "bf16 image"
    with pytest.raises(ValueError, match=image):
        ops.gat_forward_bf16(None, F, M(8, 32), M(8, 4), M(8, 4), M(8, 32), M(8, 4), 4)
    with pytest.raises(ValueError, match=image):
        ops.gat_backward_dst_bf16(None, F, M(8, 32), M(8, 4), M(8, 4), M(8, 4), M(8, 32), M(8, 32), M(8, 4), M(8, 4), 4)
    with pytest.raises(ValueError, match=image):
        ops.gat_backward_src_bf16(None, F, M(8, 32), M(8, 4), M(8, 4), M(8, 4), M(8, 4), M(8, 32), M(2, 32), M(8, 4), M(8, 4),
                                  M(8, 32), 4)
    with pytest.raises(ValueError, match=image):
        ops.gatv2_forward_bf16(None, F, M(8, 32), M(8, 32), M(1, 32), M(8, 32), M(8, 4), 4)
    with pytest.raises(ValueError, match=image):
        ops.gatv2_backward_dst_bf16(None, F, M(8, 32), M(8, 32), M(1, 32), M(8, 4), M(8, 32), M(8, 32), M(8, 4), M(8, 32), M(8, 32), 4)
    with pytest.raises(ValueError, match=image):
        ops.gatv2_backward_src_bf16(None, F, M(8, 32), img(8, 32), M(1, 32), M(8, 4), M(8, 4), M(8, 32), M(8, 32), 4)    # G
    with pytest.raises(ValueError, match=image):
        ops.gatdot_forward_bf16(None, F, M(8, 32), img(8, 32), M(8, 32), M(8, 32), M(8, 4), 4)                          # Zv
    with pytest.raises(ValueError, match=image):
        ops.gatdot_backward_dst_bf16(None, F, M(8, 32), M(8, 32), img(8, 32), M(8, 4), M(8, 32), M(8, 32), M(8, 4), M(8, 32), 4)
    with pytest.raises(ValueError, match=image):
        ops.gatdot_backward_src_bf16(None, F, M(8, 32), M(8, 32), M(8, 32), M(8, 4), M(8, 4), img(8, 32), M(8, 32), M(8, 32), 4)
    # an image in an own-row role, and an image handed to the fp32 wrapper
    with pytest.raises(ValueError, match="stays fp32"):
        ops.gatv2_forward_bf16(None, F, img(8, 32), img(8, 32), M(1, 32), M(8, 32), M(8, 4), 4)
    with pytest.raises(ValueError, match=image):
        ops.gatdot_forward(None, F, M(8, 32), img(8, 32), img(8, 32), M(8, 32), M(8, 4), 4)
    # images of the wrong shape: the fp32 wrappers' checks
    with pytest.raises(ValueError, match="shape mismatch"):
        ops.gat_forward_bf16(None, F, img(9, 32), M(8, 4), M(8, 4), M(8, 32), M(8, 4), 4)
    with pytest.raises(ValueError, match="not divisible"):
        ops.gat_forward_bf16(None, F, img(8, 30), M(8, 4), M(8, 4), M(8, 30), M(8, 4), 4)
    with pytest.raises(ValueError, match="shape mismatch"):
        ops.gat_backward_src_bf16(None, F, M(8, 32), M(8, 4), M(8, 4), M(8, 4), M(8, 4), img(7, 32), M(2, 32), M(8, 4), M(8, 4),
                                  M(8, 32), 4)
    with pytest.raises(ValueError, match="neither"):
        ops.gatv2_forward_bf16(None, F, img(8, 48), M(8, 32), M(1, 32), M(8, 32), M(8, 4), 4)
    with pytest.raises(ValueError, match="shape mismatch"):
        ops.gatv2_backward_src_bf16(None, F, M(8, 64), img(9, 64), M(1, 32), M(8, 4), M(8, 4), img(8, 32), M(8, 64), 4)
    with pytest.raises(ValueError, match="shape mismatch"):
        ops.gatdot_forward_bf16(None, F, M(8, 96), img(9, 96), img(8, 96), M(8, 32), M(8, 4), 4)
    with pytest.raises(ValueError, match="shape mismatch"):
        ops.gatdot_backward_src_bf16(None, F, img(7, 96), M(8, 96), M(8, 96), M(8, 4), M(8, 4), img(7, 32), M(8, 96), M(8, 96), 4)
    with pytest.raises(ValueError, match="drop must be"):
        ops.gat_forward_bf16(None, F, img(8, 32), M(8, 4), M(8, 4), M(8, 32), M(8, 4), 4, drop=(1, 2.0, 3))


# per new translation unit: the prefix of its kernels' names and the instantiations of each kernel -- gat_dispatch's five
# (VEC, NT, U), x DROP on the three v1 kernels; no REC form
B16_KERNELS = {
    "gat_b16.hip": ("gat.hip", "gat_", dict(gat_forward_kernel=10, gat_backward_dst_kernel=10, gat_backward_src_kernel=10)),
    "gatv2_b16.hip": ("gatv2.hip", "gatv2_", dict(gatv2_forward_kernel=5, gatv2_backward_dst_kernel=5,
                                                  gatv2_backward_src_kernel=5)),
    "gatdot_b16.hip": ("gatdot.hip", "gatdot_", dict(gatdot_forward_kernel=5, gatdot_backward_dst_kernel=5,
                                                     gatdot_backward_src_kernel=5)),
}


def _fields(blk):
    return {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
            for k in ("private_segment_fixed_size", "vgpr_spill_count", "vgpr_count", "agpr_count")}


@pytest.mark.parametrize("source", sorted(B16_KERNELS))
def test_no_bf16_instantiation_uses_scratch(tmp_path, source):
    """csrc/gat_b16.hip, gatv2_b16.hip and gatdot_b16.hip compiled for gfx950 to assembly: the resource metadata of every
    kernel whose name contains the file's prefix reports a private segment of zero bytes and zero spilled vector registers,
    these are the instantiations of B16_KERNELS and nothing else, every one of them on uint16_t ("t" in the mangled name); the VGPR counts are printed next
    to those of the fp32 twin"""
    twin_source, prefix, counts = B16_KERNELS[source]
    mine = {n: _fields(b) for n, b in _metadata(_asm(tmp_path, source)).items() if prefix in n}
    twin = {n: _fields(b) for n, b in _metadata(_asm(tmp_path, twin_source)).items()}
    assert len(mine) == sum(counts.values()), sorted(mine)
    for name, field in sorted(mine.items()):
        assert prefix in name
        # the same instantiation on float: the element type, the last template argument (gat_b16.hip: the last before the
        # pack of edge operands, "J...E", which is empty on an image), t -> f
        i = name.index("JEEEv" if source == "gat_b16.hip" else "EEv")
        assert name[i - 1] == "t", name
        twin_name = name[:i - 1] + "f" + name[i:]
        assert twin_name in twin, (name, twin_name)
        print(f"[{source}] {name}: {field}  fp32 twin vgpr_count {twin[twin_name]['vgpr_count']}")
        assert field["private_segment_fixed_size"] == 0 and field["vgpr_spill_count"] == 0, (name, field)
    for kernel, count in counts.items():
        assert sum(kernel in k for k in mine) == count, (kernel, sorted(mine))
