"""The fixed-order reduction tree (csrc/reduce.h, DESIGN.md "the reduction tree"), pinned to the bit.

For fixed inputs the outputs of the reduction entry points -- mggcn_abssum_f32, mggcn_abssum_by_set_f32, G_gamma / G_beta of
mggcn_layer_norm_backward_f32 and G_att of mggcn_gat_scores_backward_f32 -- equal the bit patterns recorded in
tests/golden/reduction_bits.json.  The fixture was recorded from the build of the commit BEFORE the tree moved into one
header, never from the code under test: a change of the order of any level (wave sum, the four waves through LDS, the
per-workgroup partials, the final kernel's slices) shows up here as a changed bit.

Inputs are exact integer arithmetic (no library random generator: the same floats on every numpy), and the per-element terms
of these entry points hold no exp / log, so the bits depend on the order of the additions alone.

Shapes (the smallest that reach every branch of the tree):
  abssum, abssum_by_set (256 elements per workgroup, grid cap kAsumBlocks = 1024)
    n = 100                less than a wave's worth per wave, one workgroup
    n = 300                two workgroups, the second ragged
    n = 2 * 1024 * 256 + 77  past the grid cap; every thread of the final kernel adds four partials
  layer-norm backward (16 rows per workgroup at these widths, grid cap kLayerNormBlocks = 1024; the final kernel sums 64 of
  the 2 m columns per workgroup from four slices of workgroups)
    m = 20 behind a misaligned pointer (element form; 2 m < 64: one final workgroup), m = 40 (2 m = 80: a ragged second
    final workgroup, the G_gamma / G_beta boundary inside the first), m = 132 (float4 form)
    n_rows = 100 (seven workgroups), 3 (fewer workgroups than slices), 2 * 16384 + 5 (past the cap), 0 (the zeros path)
    n_rows = 100 again with the leaky flag, and with G_gamma / G_beta adjacent in one buffer (otherwise two allocations)
  GAT scores backward (grid cap kGatColsumBlocks = 512)
    (K, dh) = (2, 5): 16 row slots per workgroup; (2, 65): width 130, one row slot, five final workgroups, the last ragged
    n = 100; past the cap: (2, 5) at n = 2 * 8192 + 3, (2, 65) at n = 1030; n_dst = 7 != n_src; n = 0; ld = 16 > width"""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reduction_bits.json")
SETS = np.array([-1, 0, 1, 2, 3, 7], dtype=np.int32)
LEAKY = 1                                    # MGGCN_LN_LEAKY_RELU


def values(n, c):
    """x[i] = ((i * 2654435761 + c) mod 2^32 >> 8) / 2^23 - 1: multiples of 2^-23 in [-1, 1), exact in fp32"""
    i = np.arange(n, dtype=np.uint64)
    k = ((i * np.uint64(2654435761) + np.uint64(c)) & np.uint64(0xFFFFFFFF)) >> np.uint64(8)
    return (k.astype(np.float64) / 2.0 ** 23 - 1.0).astype(np.float32)


def sets(n):
    return SETS[np.arange(n) % len(SETS)]


def _cases():
    c = {}
    for n in (100, 300, 2 * 1024 * 256 + 77):
        c[f"abssum n={n}"] = ("abssum", dict(n=n))
        c[f"abssum_by_set n={n}"] = ("abssum_by_set", dict(n=n))
    for m in (20, 40, 132):
        offset = 1 if m == 20 else 0
        for n in (100, 3, 2 * 16384 + 5, 0):
            c[f"layer_norm m={m} n={n}"] = ("layer_norm", dict(m=m, n=n, offset=offset))
        c[f"layer_norm m={m} n=100 leaky"] = ("layer_norm", dict(m=m, n=100, offset=offset, flags=LEAKY))
        c[f"layer_norm m={m} n=100 adjacent"] = ("layer_norm", dict(m=m, n=100, offset=offset, adjacent=True))
    for K, dh in ((2, 5), (2, 65)):
        c[f"gat K={K} dh={dh} n=100"] = ("gat", dict(K=K, dh=dh, n_dst=100, n_src=100))
        c[f"gat K={K} dh={dh} n=0"] = ("gat", dict(K=K, dh=dh, n_dst=0, n_src=0))
    c["gat K=2 dh=5 n=16387"] = ("gat", dict(K=2, dh=5, n_dst=2 * 8192 + 3, n_src=2 * 8192 + 3))
    c["gat K=2 dh=65 n=1030"] = ("gat", dict(K=2, dh=65, n_dst=1030, n_src=1030))
    c["gat K=2 dh=5 n_dst=7 n_src=100"] = ("gat", dict(K=2, dh=5, n_dst=7, n_src=100))
    c["gat K=2 dh=65 n_dst=100 n_src=7"] = ("gat", dict(K=2, dh=65, n_dst=100, n_src=7))
    c["gat K=2 dh=5 n=100 ld=16"] = ("gat", dict(K=2, dh=5, n_dst=100, n_src=100, ld=16))
    return c


CASES = _cases()


def _torch():
    import torch
    return torch


def _dev(a, offset=0):
    """a device copy of ``a`` whose first element sits ``offset`` elements into an aligned allocation"""
    torch = _torch()
    a = np.ascontiguousarray(a).reshape(-1)
    t = torch.zeros(offset + max(a.size, 1), dtype=torch.from_numpy(a[:0]).dtype, device="cuda")
    if a.size:
        t[offset:offset + a.size] = torch.from_numpy(a).cuda()
    return t[offset:]


def _out(n):
    """n floats that no kernel result equals by accident"""
    return _torch().full((max(n, 1),), 123.0, dtype=_torch().float32, device="cuda")


def _bits(*tensors):
    return np.concatenate([t.cpu().numpy().reshape(-1).view(np.uint32) for t in tensors])


def _abssum(lib, st, n):
    X, r = _dev(values(n, 1)), _out(1)
    _torch().cuda.synchronize()
    lib.mggcn_abssum_f32(st, X.data_ptr(), n, r.data_ptr())
    lib.mggcn_stream_synchronize(st)
    return _bits(r)


def _abssum_by_set(lib, st, n):
    X, S, r = _dev(values(n, 2)), _dev(sets(n)), _out(4)
    _torch().cuda.synchronize()
    lib.mggcn_abssum_by_set_f32(st, X.data_ptr(), S.data_ptr(), n, r.data_ptr())
    lib.mggcn_stream_synchronize(st)
    return _bits(r)


def _layer_norm(lib, st, m, n, offset=0, flags=0, adjacent=False):
    """G_gamma then G_beta; G_in is written and not looked at"""
    G, act, xhat = (_dev(values(n * m, c), offset) for c in (3, 4, 5))
    rstd, gamma = _dev(values(n, 6) + np.float32(2.0)), _dev(values(m, 7))
    G_in = _dev(np.zeros(n * m, dtype=np.float32), offset)
    if adjacent:
        both = _out(2 * m)
        Gg, Gb = both[:m], both[m:]
    else:
        Gg, Gb = _out(m), _out(m)
    _torch().cuda.synchronize()
    lib.mggcn_layer_norm_backward_f32(st, G.data_ptr(), act.data_ptr(), xhat.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                                      G_in.data_ptr(), Gg.data_ptr(), Gb.data_ptr(), n, m, flags)
    lib.mggcn_stream_synchronize(st)
    return _bits(Gg[:m], Gb[:m])


def _gat(lib, st, K, dh, n_dst, n_src, ld=None):
    width = K * dh
    ld = width if ld is None else ld
    dsd, Zd = _dev(values(n_dst * K, 8)), _dev(values(n_dst * ld, 9))
    dss, Zs = _dev(values(n_src * K, 10)), _dev(values(n_src * ld, 11))
    G_att = _out(2 * width)
    _torch().cuda.synchronize()
    lib.mggcn_gat_scores_backward_f32(st, dsd.data_ptr(), Zd.data_ptr(), ld, n_dst, dss.data_ptr(), Zs.data_ptr(), ld, n_src,
                                      K, dh, G_att.data_ptr())
    lib.mggcn_stream_synchronize(st)
    return _bits(G_att[:2 * width])


RUN = {"abssum": _abssum, "abssum_by_set": _abssum_by_set, "layer_norm": _layer_norm, "gat": _gat}


def run_case(lib, st, name):
    """the uint32 bit patterns of case ``name`` on stream ``st`` (also what records the fixture)"""
    kind, args = CASES[name]
    return RUN[kind](lib, st, **args)


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _check(golden, name, got):
    want = np.array(golden[name], dtype=np.uint32)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (name, bad[:8], got[bad[:8]].view(np.float32), want[bad[:8]].view(np.float32), bad.size)


def test_the_fixture_covers_the_case_table(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_recorded_bits(ctx, golden, name):
    _check(golden, name, run_case(ctx.lib, ctx.stream(0), name))


def test_column_sums_share_one_growing_scratch(ctx, golden):
    """layer norm and GAT on one fresh stream, one after the other, each needing more column partials than the one before
    (1024 x 2 x 20, 512 x 2 x 130, 1024 x 2 x 132 floats): the scratch grows between its users and each keeps its bits"""
    lib = ctx.lib
    ctx.set()
    st = lib.mggcn_stream_create(0)
    try:
        for name in ("layer_norm m=20 n=100", "gat K=2 dh=65 n=1030", "layer_norm m=132 n=32773", "gat K=2 dh=5 n=100",
                     "abssum n=300"):
            _check(golden, name, run_case(lib, st, name))
    finally:
        lib.mggcn_stream_destroy(st)
