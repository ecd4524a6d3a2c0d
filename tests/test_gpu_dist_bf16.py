"""bf16 aggregation on the row partition (dist_gcn(agg_dtype="bf16")): the bf16 halo pack kernel bit for bit, the partitioned
operator against the fp32 operator on the rounded operand bit for bit (every schedule), the exchange's byte account, the
model against the bf16-wrapped exact-accumulation oracle, and the RCCL transport with one rank.

Multi-rank cases: fresh spawned children that share the one GPU over gloo, as in test_dist_gpu.py.  A child never raises
between two collectives (its peers would wait for it): it collects what it found and reports at the end.

Grid cap of mggcn_gather_rows_bf16 (elementwise.hip kGatherBf16Blocks = kNumCU * 8 = 2048 workgroups of 4 waves, each wave
carrying 64 / L rows, L = lanes per row = the power of two that covers a row's 16- / 4- / 2-byte units, at most 64):
  PACK_WAVES = 8192 waves per pass;  d = 8 on the 16-byte path: 1 unit, L = 1, 64 rows per wave, 524 288 rows per pass;
  d = 41 on the element path: 41 units, L = 64, one row per wave, 8 192 rows per pass.
One-line mutants the two multi-pass cases catch and the small cases do not: the row loop's stride without the rows-per-wave
factor (k += waves: rows of the second pass are copied by the wrong lanes' rows and the tail is never reached -- below one
pass the loop body runs once), and a stride of gridDim.x * rows_per_wave (one wave per workgroup assumed).  The small
cases catch rows-per-wave missing from the row index (k = wave + sub) at n_indices just over one wave's rows.
"""
import os
import sys
import traceback

import numpy as np
import pytest
import torch.multiprocessing as mp

from bf16_ref import round_bf16
from test_dist_gpu import _data, _free_port
from test_gpu_agg_bf16 import GRAD_BAR, TOL, W_SOLID_BAR, _bf16_oracle, _relerr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADAM = (1e-2, 0.9, 0.999, 5e-4, 1e-8)
# gradients (and the well-conditioned weights) above the first layer: 1e-4; the first layer: test_gpu_agg_bf16.GRAD_BAR
# (1e-2: rounding-midpoint flips of its cancelling X^T T sums, DESIGN.md 3.5 "Parity")
GRAD_BAR_ABOVE = 1e-4


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


def _torch():
    import torch
    return torch


# ---- the kernel ------------------------------------------------------------------------------------------------------
SENTINEL = 0x1234
SPECIALS = np.array([0x7FC0, 0x7FC1, 0xFFFF, 0x7F81, 0xFFA5, 0x7F80, 0xFF80, 0x8000, 0x0000, 0x0001, 0x807F, 0x007F],
                    dtype=np.uint16)                  # NaN payloads, +-inf, -0, +0, denormals
PACK_WAVES = 256 * 8 * 4                              # kGatherBf16Blocks workgroups x 4 waves (module docstring)


def _path(d, ld_s, ld_d, off_s, off_d):
    """bytes per lane the launcher picks (torch allocations are at least 256-byte aligned; offsets in elements)"""
    if d % 8 == 0 and ld_s % 8 == 0 and ld_d % 8 == 0 and off_s % 8 == 0 and off_d % 8 == 0:
        return 16
    if d % 2 == 0 and ld_s % 2 == 0 and ld_d % 2 == 0 and off_s % 2 == 0 and off_d % 2 == 0:
        return 4
    return 2


def _rows_per_wave(d, path):
    units, L = d // (path // 2), 1
    while L < 64 and L < units:
        L *= 2
    return 64 // L


def _source(n_src, d, seed):
    """random 16-bit patterns with the special ones planted in every row (rotating, so that a width-1 row gets one)"""
    bits = np.random.default_rng(seed).integers(0, 1 << 16, size=(n_src, d), dtype=np.uint16)
    for r in range(n_src):
        k = min(d, SPECIALS.size)
        cols = (np.arange(k) * 7 + r) % d if d >= SPECIALS.size else np.arange(k)
        bits[r, cols] = np.roll(SPECIALS, r)[:k]
    return bits


def _indices(n_idx, n_src, seed):
    """a descending run, then random rows with repeats"""
    rnd = np.random.default_rng(seed).integers(0, n_src, size=n_idx)
    down = np.arange(n_src - 1, -1, -1)[:n_idx]
    idx = np.concatenate([down, rnd])[:n_idx]
    if n_idx >= 4:
        idx[-1] = idx[-2] = idx[1]                                        # a repeat for certain
    return idx.astype(np.uint32)


def _pack(pkg, ctx, bits, idx, pad_s, pad_d, off_s, off_d, slack_rows=2):
    """runs ops.gather_rows_bf16 from a padded, offset image of ``bits``; returns (whole dst allocation, expected)"""
    torch = _torch()
    n_src, d = bits.shape
    ld_s, ld_d = d + pad_s, d + pad_d
    n_dst = len(idx) + slack_rows
    src_flat = np.full(off_s + n_src * ld_s, 0x4321, dtype=np.uint16)
    src_flat[off_s:].reshape(n_src, ld_s)[:, :d] = bits
    src_t = torch.from_numpy(src_flat.view(np.int16)).cuda()
    dst_t = torch.full((off_d + n_dst * ld_d,), SENTINEL, dtype=torch.int16, device="cuda")
    idx_t = torch.from_numpy(idx.astype(np.int64)).to(torch.int32).cuda() if len(idx) else \
        torch.empty(0, dtype=torch.int32, device="cuda")
    src_v = src_t[off_s:].view(n_src, ld_s)[:, :d]
    dst_v = dst_t[off_d:].view(n_dst, ld_d)[:, :d]
    pkg.ops.gather_rows_bf16(ctx, src_v, idx_t, dst_v)
    ctx.sync()
    want = np.full(off_d + n_dst * ld_d, SENTINEL, dtype=np.uint16)
    if len(idx):
        want[off_d:].reshape(n_dst, ld_d)[:len(idx), :d] = bits[idx.astype(np.int64)]
    return dst_t.cpu().numpy().view(np.uint16), want


LAYOUTS = [(0, 0, 0, 0), (8, 8, 0, 0), (5, 5, 0, 0), (8, 5, 0, 0), (2, 6, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1),
           (8, 8, 1, 1), (8, 8, 2, 0), (8, 8, 0, 2), (8, 16, 8, 8)]       # (pad src, pad dst, offset src, offset dst)


@pytest.mark.parametrize("d", [1, 7, 41, 64, 100, 128, 136])
def test_pack_is_bit_exact_on_every_lane_path(pkg, ctx, d):
    n_src = 203
    bits = _source(n_src, d, seed=d)
    assert np.isin(SPECIALS, bits).all() or d < SPECIALS.size
    paths = set()
    for li, (pad_s, pad_d, off_s, off_d) in enumerate(LAYOUTS):
        path = _path(d, d + pad_s, d + pad_d, off_s, off_d)
        paths.add(path)
        rpw = _rows_per_wave(d, path)
        sizes = sorted({0, 1, max(rpw - 1, 1), rpw + 1, 4 * rpw + 1, 9 * 4 * rpw + 3})     # ... and more than one workgroup
        for n_idx in sizes:
            got, want = _pack(pkg, ctx, bits, _indices(n_idx, n_src, seed=li * 100 + n_idx), pad_s, pad_d, off_s, off_d)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (d, (pad_s, pad_d, off_s, off_d), path, n_idx, bad[:8], got[bad[:8]], want[bad[:8]])
    assert paths == ({16, 4, 2} if d % 8 == 0 else {4, 2} if d % 2 == 0 else {2}), paths


@pytest.mark.parametrize("d,path", [(8, 16), (41, 2)])
def test_pack_beyond_one_grid_pass(pkg, ctx, d, path):
    """two full passes of the capped grid and a ragged third, every row compared"""
    assert _path(d, d, d, 0, 0) == path
    per_pass = PACK_WAVES * _rows_per_wave(d, path)
    assert per_pass == {8: 524_288, 41: 8_192}[d]
    n_idx = 2 * per_pass + 37
    bits = _source(1009, d, seed=3)
    got, want = _pack(pkg, ctx, bits, _indices(n_idx, 1009, seed=4), 0, 0, 0, 0)
    rows = np.flatnonzero((got.reshape(-1, d) != want.reshape(-1, d)).any(axis=1))
    assert rows.size == 0, (d, rows.size, rows[:8])


# ---- children ----------------------------------------------------------------------------------------------------------
def _init(rank, P, port, backend="gloo"):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    if backend == "nccl":
        import torch
        os.environ["MGGCN_DIST_SELF_GATHER"] = "1"          # one rank: the exchange over ProcessGroupNCCL still runs
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=rank, world_size=P, device_id=torch.device("cuda", 0))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=P)
    return dist


def _spawn(target, P, args):
    """P fresh children; every result, in rank order.  A child that dies fails the case; nothing is retried."""
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = _free_port()
    procs = [mpc.Process(target=target, args=(r, P, port) + tuple(args) + (q,)) for r in range(P)]
    for pr in procs:
        pr.start()
    res = sorted([q.get(timeout=300) for _ in range(P)], key=lambda t: t[0])
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    return res


# ---- the operator -----------------------------------------------------------------------------------------------------
def _operand(n, d):
    return np.random.default_rng(1000 + d).standard_normal((n, d), dtype=np.float32)


def _op_worker(rank, P, port, n, cases, q):
    """per case (mode, chunks, d, overlap): dist_sparse_linear(agg_dtype="bf16") on B against the fp32 operator on
    round_bf16(B), forward (discard x flags) and backward (discard), each bf16 call twice; reports the mismatches and the
    rank's forward shard"""
    dist = _init(rank, P, port)
    try:
        import torch
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        pkg, (ip, ix, dv), _, _ = _data(n, 1, 2)
        D = pkg.dist
        A = pkg.csr_matrix(ip, ix, dv, n)
        A.normalize(True)
        A_T = A.transpose()
        p = D.partition_bounds(n, P)
        rows = n // P
        dctxs, mats, bad, shards = {}, {}, [], {}
        for mode, chunks, d, overlap in cases:
            if overlap not in dctxs:
                dctxs[overlap] = D.dist_context(overlap=overlap, device_index=0)
            dctx = dctxs[overlap]
            if (chunks, overlap) not in mats:
                mats[(chunks, overlap)] = (D.dist_row_csr_matrix(dctx, A, p, p, chunks), D.dist_row_csr_matrix(dctx, A_T, p, p, chunks))
            Ad, ATd = mats[(chunks, overlap)]
            dev = dctx.ctx.device
            big = n * d if mode != "rounds" else rows * d
            ops = {}
            for agg, dt in (("bf16", torch.bfloat16), ("f32", torch.float32)):
                ops[agg] = D.dist_sparse_linear("t_", Ad, ATd, torch.empty(big, dtype=dt, device=dev),
                                                torch.empty(rows * d, dtype=dt, device=dev), mode, agg)
            B = _operand(n, d)
            Bd, Brd = D.dist_row_dn_matrix(dctx, B), D.dist_row_dn_matrix(dctx, round_bf16(B))
            C0 = np.random.default_rng(d + rank).standard_normal((rows, d), dtype=np.float32)
            for direction, discard, flags in [("fwd", True, 0), ("fwd", True, 1), ("fwd", False, 0), ("fwd", False, 1),
                                              ("bwd", True, 0), ("bwd", False, 0)]:
                C = [D.dist_row_dn_matrix(dctx, (n, d)) for _ in range(3)]
                for c in C:
                    c.local.init(C0)
                dctx.sync()
                for op, operand, c in ((ops["bf16"], Bd, C[0]), (ops["f32"], Brd, C[1]), (ops["bf16"], Bd, C[2])):
                    if direction == "fwd":
                        op(dctx, operand, c, discard, flags)
                    else:
                        op.backward(dctx, operand, c, discard)
                dctx.sync()
                got, want, again = (c.local.numpy().view(np.uint32) for c in C)
                key = (mode, chunks, d, overlap, direction, discard, flags)
                if not np.array_equal(got, want):
                    bad.append(key + ("bf16 != f32 on the rounded operand", int((got != want).sum())))
                if not np.array_equal(got, again):
                    bad.append(key + ("second call differs", int((got != again).sum())))
                if (direction, discard, flags) == ("fwd", True, 0):
                    shards[(mode, chunks, d, overlap)] = C[0].local.numpy().copy()
            if ops["bf16"].bcast[0].dtype != torch.bfloat16 or ops["bf16"].agg_buffer.dtype != torch.bfloat16:
                bad.append((mode, chunks, d, overlap, "buffers are not bf16"))
        q.put((rank, bad, shards, None))
    except Exception:
        q.put((rank, None, None, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def _op_cases():
    cases = [(mode, chunks, d, True) for mode, chunks in (("allgather", 1), ("allgather", 3), ("halo", None), ("rounds", None))
             for d in (128, 100, 41)]
    return cases + [("allgather", 3, d, False) for d in (128, 41)]          # the exchange on the compute stream


@pytest.mark.parametrize("P,n", [(2, 1536), (3, 1536), (3, 1002)])
def test_partitioned_bf16_operator_equals_fp32_on_the_rounded_operand(pkg, oracle, P, n):
    """n = 1536 at P = 2: every piece boundary a multiple of 8 rows; n = 1002 at P = 3 with 3 pieces: bounds 0 / 111 / 222 /
    334, views at odd element offsets at d = 41"""
    if n == 1002:
        assert pkg.dist.chunk_bounds(n // P, 3) == [0, 111, 222, 334]
    cases = _op_cases()
    res = _spawn(_op_worker, P, (n, cases))
    for rank, bad, shards, err in res:
        assert err is None, err
        assert not bad, (rank, bad[:6], len(bad))
    _, (ip, ix, dv), _, _ = _data(n, 1, 2)
    Ao = oracle.Csr(ip, ix, dv, n)
    oracle.normalize(Ao, True)
    refs = {}
    for case in cases:
        d = case[2]
        if d not in refs:
            refs[d] = oracle.spmm(Ao, round_bf16(_operand(n, d)), f64acc=True)
        got = np.concatenate([shards[case] for _, _, shards, _ in res])
        err = np.abs(got - refs[d]).max() / np.abs(refs[d]).max()
        print(f"[dist-bf16] P={P} n={n} {case}: {err:.3e} of the largest entry")
        assert err <= TOL, (case, err)


# ---- the byte account ---------------------------------------------------------------------------------------------------
def _bytes_worker(rank, P, port, n, F, C, hidden, q):
    dist = _init(rank, P, port)
    try:
        pkg, (ip, ix, dv), X, Y = _data(n, F, C)
        D = pkg.dist
        dctx = D.dist_context(overlap=True, device_index=0)
        A = pkg.csr_matrix(ip, ix, dv, n)
        A.normalize(True)
        A_T = A.transpose()
        p = D.partition_bounds(n, P)
        sizes = [F] + hidden + [(C + P - 1) // P * P]
        Ad, ATd = D.dist_row_csr_matrix(dctx, A, p, p), D.dist_row_csr_matrix(dctx, A_T, p, p)
        Xd, Yd = D.dist_row_dn_matrix(dctx, X), D.dist_row_dn_matrix(dctx, Y)
        out = {}
        for mode in ("allgather", "halo", "rounds"):
            for agg in ("f32", "bf16"):
                G = D.dist_gcn(dctx, Ad, ATd, sizes, fused=True, mode=mode, agg_dtype=agg)
                dctx.exchange_bytes = 0
                loss, _ = G.train_forward(dctx, Xd, Yd)
                G.backward(dctx)
                dctx.sync()
                out[(mode, agg)] = (int(dctx.exchange_bytes), str(G.bcast_buffer.dtype), G.bcast_buffer.numel() * G.bcast_buffer.element_size(),
                                    str(G.bcast_buffer2.dtype), G.bcast_buffer2.numel() * G.bcast_buffer2.element_size(), loss)
        q.put((rank, out, None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_bf16_exchange_moves_exactly_half_the_bytes():
    res = _spawn(_bytes_worker, 2, (1536, 20, 5, [16, 16]))
    for rank, out, err in res:
        assert err is None, err
        for mode in ("allgather", "halo", "rounds"):
            b32, dt32, n32, dt32b, n32b, l32 = out[(mode, "f32")]
            b16, dt16, n16, dt16b, n16b, l16 = out[(mode, "bf16")]
            print(f"[dist-bf16] rank {rank} {mode}: exchange bytes f32 {b32}, bf16 {b16}; receive buffer {n32} -> {n16} bytes")
            assert b32 > 0 and b16 > 0 and 2 * b16 == b32, (rank, mode, b32, b16)
            assert (dt32, dt32b) == ("torch.float32", "torch.float32")
            assert (dt16, dt16b) == ("torch.bfloat16", "torch.bfloat16")
            assert 2 * n16 == n32 and 2 * n16b == n32b
            assert abs(l16 - l32) <= 1e-2 * abs(l32)                       # the same model, rounded operands


# ---- the model ----------------------------------------------------------------------------------------------------------
def _model_worker(rank, P, port, n, F, C, hidden, mode, epochs, backend, chunks, overlap, resync, S, q):
    """test_dist_gpu._worker with agg_dtype="bf16" (and the splits when S is given): per epoch (loss, acc, [G_W], [G_b],
    [(W, b) after Adam]); the parameters continue from the oracle's after every epoch"""
    dist = _init(rank, P, port, backend)
    try:
        pkg, (ip, ix, dv), X, Y = _data(n, F, C)
        D = pkg.dist
        dctx = D.dist_context(overlap=overlap, device_index=0)
        A = pkg.csr_matrix(ip, ix, dv, n)
        A.normalize(True)
        A_T = A.transpose()
        p = D.partition_bounds(n, P)
        sizes = [F] + hidden + [(C + P - 1) // P * P]
        G = D.dist_gcn(dctx, D.dist_row_csr_matrix(dctx, A, p, p, chunks), D.dist_row_csr_matrix(dctx, A_T, p, p, chunks),
                       sizes, fused=True, mode=mode, agg_dtype="bf16")
        if S is not None:
            G.set_splits(dctx, S[p[rank]:p[rank + 1]].copy())
        Xd, Yd = D.dist_row_dn_matrix(dctx, X), D.dist_row_dn_matrix(dctx, Y)
        out, bad = [], []
        for ep in range(epochs):
            if ep == epochs - 1 and epochs > 1:         # last epoch through the one-sync step
                loss, acc = G.train_step(dctx, Xd, Yd, *ADAM)
                out.append((loss, acc, None, None, None))
                continue
            loss, acc = G.train_forward(dctx, Xd, Yd)
            G.backward(dctx)
            dctx.sync()
            grads = [l.GW().local.numpy().copy() for l in G.layers()]
            gb = [l.Gb().local.numpy().copy() for l in G.layers()]
            G.adam_update(dctx, *ADAM)
            dctx.sync()
            out.append((loss, acc, grads, gb, [(l.W().local.numpy().copy(), l.b().local.numpy().copy()) for l in G.layers()]))
            for l, (W, b) in zip(G.layers(), resync[ep]):
                l.W().local.init(W)
                l.b().local.init(b)
            dctx.sync()
        q.put((rank, out, str(G.bcast_buffer.dtype), None))
    except Exception:
        q.put((rank, None, None, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def _oracle_run(oracle, n, F, C, hidden, P, epochs, S):
    """the bf16-wrapped oracle's own epochs (classes padded to a multiple of P, as the partitioned model pads them)"""
    _, (ip, ix, dv), X, Y = _data(n, F, C)
    sizes = [F] + hidden + [(C + P - 1) // P * P]
    O = _bf16_oracle(oracle, ip, ix, dv, n, sizes, False)
    want, resync = [], []
    for _ in range(epochs):
        if S is None:
            ol, oa = O.train_forward(X, Y)
            O.backward()
        else:
            from test_gpu_splits import _oracle_split_epoch
            per, _ = _oracle_split_epoch(oracle, O, X, Y, S, 0)
            ol, oa = per["train"][:2]
        want.append((ol, oa, [l.lin.G_W.copy() for l in O.layers], [l.lin.G_b.copy() for l in O.layers]))
        O.adam_update()
        resync.append([(l.lin.W.copy(), l.lin.b.copy()) for l in O.layers])
    return want, resync, sizes


def _assert_model(rank, out, want, resync, n_acc):
    for e, ((loss, acc, grads, gb, Wb), (ol, oa, oG, oGb)) in enumerate(zip(out, want)):
        print(f"[dist-bf16] rank {rank} epoch {e}: loss {loss!r} (oracle {ol!r}), acc {acc!r} (oracle {oa!r})")
        assert abs(loss - ol) <= TOL * abs(ol), (rank, e, loss, ol)
        assert abs(acc - oa) <= 3.0 / n_acc, (rank, e, acc, oa)
        if grads is None:
            continue
        for li, (g, og, b, ob) in enumerate(zip(grads, oG, gb, oGb)):
            eg, eb = _relerr(g, og), _relerr(b, ob)
            print(f"[dist-bf16]   layer {li}: G_W {eg:.3e}, G_b {eb:.3e}")
            assert eg <= GRAD_BAR.get(li, GRAD_BAR_ABOVE), (rank, e, li, "G_W", eg)
            assert eb <= GRAD_BAR.get(li, GRAD_BAR_ABOVE), (rank, e, li, "G_b", eb)
            for Pm, Po, gr in ((Wb[li][0], resync[e][li][0], og), (Wb[li][1], resync[e][li][1], ob)):
                assert np.abs(Pm - Po).max() <= 2.05 * ADAM[0], (rank, e, li)              # never more than a sign flip
                solid = np.abs(gr) > 1e-2 * np.abs(gr).max()                              # well-conditioned entries
                ew = np.abs(Pm - Po)[solid].max() / np.abs(Po).max()
                assert ew <= W_SOLID_BAR.get(li, TOL), (rank, e, li, Pm.shape, ew)


def _model_case(pkg, ctx, oracle, P, mode, chunks, n, F, C, hidden, sets=False, backend="gloo", epochs=3, single=True):
    S = None
    if sets:
        S = np.random.default_rng(23).choice(4, size=n, p=(0.5, 0.2, 0.25, 0.05)).astype(np.int32)
    want, resync, sizes = _oracle_run(oracle, n, F, C, hidden, P, epochs, S)
    res = _spawn(_model_worker, P, (n, F, C, hidden, mode, epochs, backend, chunks, True, resync, S))
    n_acc = n if S is None else int((S == 0).sum())
    for rank, out, dtype, err in res:
        assert err is None, err
        assert dtype == "torch.bfloat16"
        _assert_model(rank, out, want, resync, n_acc)
        assert out[-1][0] < out[0][0] or epochs == 1                                      # trains
        assert [o[0] for o in out] == [o[0] for o in res[0][1]]                            # the same loss on every rank
    if single:          # the partitioned bf16 model is the single-GPU bf16 model
        _, (ip, ix, dv), X, Y = _data(n, F, C)
        G1 = pkg.gcn(pkg.csr_matrix(ip, ix, dv, n), sizes, agg_dtype="bf16")
        if S is not None:
            G1.set_splits(S)
        l1, _ = G1.train_forward(ctx, pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y))
        ctx.sync()
        print(f"[dist-bf16] single-GPU bf16 loss {l1!r}, partitioned {res[0][1][0][0]!r}")
        assert abs(res[0][1][0][0] - l1) <= TOL * abs(l1), (res[0][1][0][0], l1)


@pytest.mark.parametrize("mode,sets", [("allgather", False), ("halo", False), ("rounds", False), ("allgather", True)])
def test_dist_bf16_model_matches_the_bf16_oracle(pkg, ctx, oracle, mode, sets):
    _model_case(pkg, ctx, oracle, 2, mode, None, 1536, 20, 5, [16, 16], sets=sets)


def test_dist_bf16_model_on_an_odd_shape(pkg, ctx, oracle):
    _model_case(pkg, ctx, oracle, 3, "allgather", None, 1002, 13, 5, [20, 12])


@pytest.mark.parametrize("mode", ["allgather", "halo", "rounds"])
def test_dist_bf16_over_rccl_single_rank(pkg, ctx, oracle, mode):
    """the RCCL transport carries torch.bfloat16 (all_gather_into_tensor / all_to_all_single / broadcast on the comm
    stream) with the one rank a one-GPU box allows and the self-gather switched on"""
    _model_case(pkg, ctx, oracle, 1, mode, 2, 1536, 20, 5, [16, 16], backend="nccl", epochs=1, single=False)
