"""bf16 aggregation on the row partition, the parts that need no GPU: the new C entry is declared, bound and exported, the
host-staged gloo collectives carry torch.bfloat16 shards bit for bit (and fp32 ones as before), and a wrong agg_dtype
is refused before any device work."""
import ctypes
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gather_rows_bf16_is_declared_bound_and_exported(pkg):
    text = open(os.path.join(ROOT, "include", "mggcn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bvoid\s+mggcn_gather_rows_bf16\s*\(([^)]*)\)\s*;", text)
    assert m, "mggcn_gather_rows_bf16 is not declared in include/mggcn.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert len(params) == 8, params
    assert params[1] == "const uint16_t *src" and params[6] == "uint16_t *dst", params
    assert params[3] == "const uint32_t *indices", params
    restype, argtypes = pkg._lib.PROTOTYPES["mggcn_gather_rows_bf16"]
    assert restype is None and len(argtypes) == 8
    assert hasattr(ctypes.CDLL(pkg._lib.LIB_PATH), "mggcn_gather_rows_bf16")
    assert pkg._lib.load().mggcn_abi_version() == 1
    assert callable(pkg.ops.gather_rows_bf16)
    comm = open(os.path.join(ROOT, "include", "mggcn_comm.h")).read()
    assert "bf16" not in comm                                  # the C++ exchange library stays fp32-only


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


SPECIALS = np.array([0x7FC0, 0x7FC1, 0xFFFF, 0x7F81, 0x7F80, 0xFF80, 0x8000, 0x0000, 0x0001, 0x807F, 0x3F80],
                    dtype=np.uint16)              # NaNs with payloads, +-inf, -0, +0, denormals, 1.0
SHAPES = [(5, 41), (5, 128), (0, 41), (0, 128)]


def _shard_bits(rank, rows, d):
    """the bf16 bit patterns of rank's shard: random 16-bit words (every class of value) with the specials planted"""
    bits = np.random.default_rng(100 * rank + d).integers(0, 1 << 16, size=(rows, d), dtype=np.uint16)
    flat = bits.reshape(-1)
    k = min(SPECIALS.size, flat.size)
    flat[:k] = SPECIALS[:k]
    flat[flat.size - k:] = SPECIALS[:k][::-1]
    return bits


def _shard_f32(rank, rows, d):
    return np.random.default_rng(7 + rank).standard_normal((rows, d)).astype(np.float32)


def _worker(rank, P, port, out_q):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    D = ge.load_package().dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=P)
    try:
        out = {}
        for rows, d in SHAPES:
            mine16 = torch.from_numpy(_shard_bits(rank, rows, d).view(np.int16)).view(torch.bfloat16)
            mine32 = torch.from_numpy(_shard_f32(rank, rows, d))
            g16 = D.gloo_all_gather_rows(mine16, P)
            assert g16.dtype == torch.bfloat16 and tuple(g16.shape) == (P * rows, d)
            g32 = D.gloo_all_gather_rows(mine32, P)
            assert g32.dtype == torch.float32
            b16, b32 = [], []
            for root in range(P):
                t = D.gloo_broadcast_rows(mine16 if rank == root else None, (rows, d), torch.bfloat16, root, rank)
                assert t.dtype == torch.bfloat16 and tuple(t.shape) == (rows, d)
                b16.append(t.view(torch.int16).numpy().copy())
                t = D.gloo_broadcast_rows(mine32 if rank == root else None, (rows, d), torch.float32, root, rank)
                b32.append(t.numpy().copy())
            out[(rows, d)] = (g16.view(torch.int16).numpy().copy(), g32.numpy().copy(), b16, b32)
        out_q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_gloo_helpers_carry_bf16_shards_bit_for_bit():
    """world size 2: all-gather and broadcast of bf16 shards (widths 41 and 128, 5 rows and none) equal the concatenation
    of the ranks' bit patterns; the same calls on fp32 shards give what they gave.  (The all-gather placed the rank's own
    rows through numpy, which has no bf16: it raised before the bf16 path existed.)"""
    P = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, P, port, q)) for r in range(P)]
    for pr in procs:
        pr.start()
    res = sorted([q.get(timeout=120) for _ in range(P)], key=lambda t: t[0])
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    for rows, d in SHAPES:
        want16 = [_shard_bits(r, rows, d).view(np.int16) for r in range(P)]
        want32 = [_shard_f32(r, rows, d) for r in range(P)]
        if rows:
            cat = np.concatenate(want16).view(np.uint16)
            assert np.isin(SPECIALS, cat).all()
        for rank, out in res:
            g16, g32, b16, b32 = out[(rows, d)]
            assert g16.dtype == np.int16 and g16.shape == (P * rows, d)
            np.testing.assert_array_equal(g16, np.concatenate(want16))
            np.testing.assert_array_equal(g32.view(np.uint32), np.concatenate(want32).view(np.uint32))
            for root in range(P):
                np.testing.assert_array_equal(b16[root], want16[root])
                np.testing.assert_array_equal(b32[root].view(np.uint32), want32[root].view(np.uint32))


def test_a_wrong_agg_dtype_is_refused_before_any_device_work(pkg):
    D = pkg.dist
    with pytest.raises(ValueError, match="agg_dtype"):
        D.dist_sparse_linear("0_", None, None, None, None, "allgather", agg_dtype="fp16")
    with pytest.raises(ValueError, match="agg_dtype"):
        D.dist_gcn(None, None, None, [8, 4, 2], mode="halo", agg_dtype="fp16")
    with pytest.raises(ValueError, match="agg_dtype"):
        D.dist_gcn_layer(None, "0_", None, None, 8, 4, True, agg_dtype="fp16")
    for ok in ("f32", "bf16"):
        op = D.dist_sparse_linear("0_", None, None, None, None, "rounds", ok)       # the new argument is the last one
        assert op.agg_dtype == ok and op.mode == "rounds"


def test_the_pack_kernels_move_16_bytes_per_lane_without_scratch(tmp_path):
    """device code of the three instances of the halo pack: no scratch, no AGPRs; the 16-byte instance loads and stores
    dwordx4, its four loads ahead of its four stores in the unrolled body"""
    from test_agg_bf16_cpu import _asm, _metadata
    text = _asm(tmp_path, "elementwise.hip")
    meta = _metadata(text)
    mine = [n for n in meta if "gather_rows_u16_kernel" in n]
    assert len(mine) == 3, mine                           # uint4 / uint32_t / uint16_t
    for n in mine:
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta[n]), n
        assert re.search(r"\.agpr_count:\s+0\b", meta[n]), n
    wide = [n for n in mine if "HIP_vector_type" in n]
    assert len(wide) == 1, mine
    body = re.search(r"^%s:[^\n]*\n(.*?)s_endpgm" % re.escape(wide[0]), text, flags=re.S | re.M).group(1)
    ops_ = re.findall(r"\b(global_load_dwordx4|global_store_dwordx4)\b", body)
    assert ops_.count("global_load_dwordx4") >= 5 and ops_.count("global_store_dwordx4") >= 5, ops_
    run = "".join("L" if o.startswith("global_load") else "S" for o in ops_)
    assert "LLLLSSSS" in run, run
