"""The edge sample with values and the SpMM on a device-built plan (include/mggcn.h: mggcn_edge_sample_rowscale_f32 /
_compact_val_f32, mggcn_spmm_dev_plan_*, mggcn_spmm_csr_dev_*; csrc/edge_sample.hip, csrc/spmm_dev.hip) on the device against
tests/edge_sample_val_ref.py: counts, indices and the plan's tables exactly, the row factors at their derived bound, the values
as fp32(v) * fp32(the device's own factor) bit for bit, and the product bit for bit against the host row-split plan of the same
split on the downloaded sample.  Graphs, thresholds, guards and the sentinel are those of test_gpu_edge_sample.py."""
from importlib import import_module

import numpy as np
import pytest

import edge_sample_ref as ref
import edge_sample_val_ref as vref
import gat_ref

pytestmark = pytest.mark.gpu

SENTINEL = 0x5EA1DEAD
GUARD = 64
FULL = 0xFFFFFFFF
SEED, EPOCH = 0x1234567887654321, 5
TOL = 1e-4                                                  # test_gpu_kernels.py's SpMM bar


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


def _torch():
    import torch
    return torch


def _u32(a):
    return _torch().from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def _f32(a):
    return _torch().from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


class _out:
    """n output words between two guards of GUARD words, everything pre-filled with SENTINEL; ``f``: the words as fp32"""

    def __init__(self, n, f=False):
        self.n = n
        self.flat = _torch().full((n + 2 * GUARD,), int(np.uint32(SENTINEL).view(np.int32)), dtype=_torch().int32, device="cuda")
        if f:
            self.flat = self.flat.view(_torch().float32)
        self.t = self.flat[GUARD:GUARD + n]

    def words(self):
        return self.flat.cpu().numpy().view(np.uint32)

    def check(self, what, want, written=None):
        w = self.words()
        written = self.n if written is None else written
        np.testing.assert_array_equal(w[GUARD:GUARD + written], np.asarray(want).view(np.uint32), err_msg=what)
        rest = np.concatenate([w[:GUARD], w[GUARD + written:]])
        assert (rest == SENTINEL).all(), (what, "a word outside the output was written", np.flatnonzero(rest != SENTINEL)[:4])


def _graphs():
    """name -> (indptr, indices, values, transposed, row0, col0, the destinations' indptr): test_gpu_edge_sample.py's six, the
    values uniform in (0.5, 1.5) on F and carried through the transpose"""
    out = {}
    ip, ix = gat_ref.kernel_graph_long()
    looped = ix.copy()
    for r in range(0, 320, 3):
        if ip[r + 1] > ip[r]:
            looped[ip[r + 1] - 1] = r
    v = np.random.default_rng(11).uniform(0.5, 1.5, size=ix.size).astype(np.float32)
    for name, idx in (("long", ix), ("loops", looped)):
        out[name] = (ip, idx, v, 0, 0, 0, ip)
        out[name + "T"] = (*vref.transpose_values(ip, idx, v, 320), 1, 0, 0, ip)
    rp, rx = gat_ref.kernel_graph(200, 320)
    rv = np.random.default_rng(12).uniform(0.5, 1.5, size=rx.size).astype(np.float32)
    out["rect"] = (rp, rx, rv, 0, 1000, 40, rp)
    out["rectT"] = (*vref.transpose_values(rp, rx, rv, 320), 1, 40, 1000, rp)
    return out


GRAPHS = _graphs()
FORWARD = ("long", "loops", "rect")
THRESHOLDS = ("zero", "full", "keep", "fanout", "mixed")


def _thr(kind, dst_indptr):
    n = dst_indptr.size - 1
    if kind == "zero":
        return np.zeros(n, dtype=np.uint32)
    if kind == "full":
        return np.full(n, FULL, dtype=np.uint32)
    if kind == "keep":
        return ref.thresholds(dst_indptr, None, 0.5)
    if kind == "fanout":
        return ref.thresholds(dst_indptr, 16, 1.0)
    return np.array([0, FULL, 0x80000000], dtype=np.uint32)[np.arange(n) % 3]


_scales = {}


def _device_scale(pkg, ctx, name, kind):
    """(counts guard, scale guard, scale as host fp32) of rowscale over the forward graph ``name``; made once"""
    key = (name, kind)
    if key not in _scales:
        ip, ix, v, _, row0, col0, _ = GRAPHS[name]
        n = ip.size - 1
        counts, scale = _out(n), _out(n, f=True)
        pkg.ops.edge_sample_rowscale(ctx, n, _u32(ip), _u32(ix), _f32(v), _u32(_thr(kind, ip)), counts.t, scale.t, row0=row0,
                                     col0=col0, seed=SEED, epoch=EPOCH)
        ctx.sync()
        _scales[key] = (counts, scale, scale.words()[GUARD:GUARD + n].view(np.float32).copy())
    return _scales[key]


# ---- rowscale ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", THRESHOLDS)
@pytest.mark.parametrize("name", FORWARD)
def test_rowscale(pkg, ctx, name, kind):
    ip, ix, v, _, row0, col0, _ = GRAPHS[name]
    n = ip.size - 1
    thr = _thr(kind, ip)
    counts, scale, got = _device_scale(pkg, ctx, name, kind)
    want_counts, _, _ = ref.sample(ip, ix, thr, 0, row0, col0, SEED, EPOCH)
    counts.check(f"{name} {kind} counts", want_counts)
    scale.check(f"{name} {kind} scale (guards)", got)
    r64, whole, nothing, length = vref.row_factors(ip, ix, v, thr, row0, col0, SEED, EPOCH)
    assert np.isfinite(got).all()
    assert (got[whole] == np.float32(1.0)).all() and (got[nothing] == 0.0).all()
    if kind == "full":
        assert whole[length > 0].all()
    # two fp32 sums of L positive terms (relative error <= (L - 1) u each, whatever the order) and one division (u): below 2 L u
    bound = 2.0 * length * 2.0 ** -24 * r64
    err = np.abs(got.astype(np.float64) - r64)
    print(f"[rowscale] {name} {kind}: worst |r - r64| / bound = {(err[bound > 0] / bound[bound > 0]).max() if (bound > 0).any() else 0:.3f}")
    assert (err <= bound).all()
    # the same bits for two calls over a split of the rows
    ip_d, ix_d, v_d, thr_d = _u32(ip), _u32(ix), _f32(v), _u32(thr)
    for r0, r1 in ((0, 7), (7, n)):
        k = r1 - r0
        c2, s2 = _out(k), _out(k, f=True)
        pkg.ops.edge_sample_rowscale(ctx, k, ip_d[r0:], ix_d, v_d, thr_d[r0:], c2.t, s2.t, row0=row0 + r0, col0=col0, seed=SEED,
                                     epoch=EPOCH)
        ctx.sync()
        c2.check(f"{name} {kind} rows {r0}:{r1} counts", want_counts[r0:r1])
        s2.check(f"{name} {kind} rows {r0}:{r1} scale", got[r0:r1])


# ---- compact with values -----------------------------------------------------------------------------------------------------------
def _compact_val(pkg, ctx, name, thr, scale, scale_self):
    ip, ix, v, transposed, row0, col0, _ = GRAPHS[name]
    n, nnz = ip.size - 1, int(ip[-1])
    ip_d, ix_d, thr_d = _u32(ip), _u32(ix), _u32(thr)
    counts, indptr, indices, values = _out(n), _out(n + 1), _out(nnz), _out(nnz, f=True)
    kw = dict(row0=row0, col0=col0, seed=SEED, epoch=EPOCH)
    pkg.ops.edge_sample_count(ctx, n, ip_d, ix_d, thr_d, transposed, counts.t, **kw)
    pkg.ops.edge_sample_scan(ctx, counts.t, n, indptr.t)
    pkg.ops.edge_sample_compact_val(ctx, n, ip_d, ix_d, _f32(v), thr_d, transposed, None if scale is None else _f32(scale),
                                    scale_self, indptr.t, indices.t, values.t, **kw)
    ctx.sync()
    return indptr, indices, values


@pytest.mark.parametrize("kind", THRESHOLDS)
@pytest.mark.parametrize("name", FORWARD)
def test_compact_val_on_both_sides(pkg, ctx, name, kind):
    """F and F^T of one graph: "row" (the device's own factors, self-loops scaled), "inverse" (the host's factors, self-loops
    left alone) and no factor at all"""
    dst_indptr = GRAPHS[name][6]
    thr = _thr(kind, dst_indptr)
    row_scale = _device_scale(pkg, ctx, name, kind)[2]
    for mode, scale, scale_self in (("row", row_scale, True), ("inverse", vref.inverse_factors(thr), False), ("none", None, True)):
        sides = []
        for side in (name, name + "T"):
            ip, ix, v, transposed, row0, col0, _ = GRAPHS[side]
            _, want_ip, want_ix, want_v = vref.sample_val(ip, ix, v, thr, transposed, scale, scale_self, row0, col0, SEED, EPOCH)
            indptr, indices, values = _compact_val(pkg, ctx, side, thr, scale, scale_self)
            what = f"{side} {kind} {mode}"
            indptr.check(what + " indptr", want_ip)
            indices.check(what + " indices", want_ix, want_ix.size)       # the sentinel still stands behind the sample
            values.check(what + " values", want_v, want_v.size)
            sides.append(vref.triples(want_ip, want_ix, want_v, transposed))
            if mode == "none":
                assert set(want_v.view(np.uint32).tolist()) <= set(v.view(np.uint32).tolist())
        np.testing.assert_array_equal(sides[0], sides[1])                 # the same (destination, source, value bits)
        if mode == "inverse" and name == "loops":                         # scale_self = 0: self-loops keep the parent's bits
            ip, ix, v, *_ = GRAPHS[name]
            parent = vref.triples(ip, ix, v, 0)
            have = {tuple(t) for t in parent[parent[:, 0] == parent[:, 1]]}
            loops = sides[0][sides[0][:, 0] == sides[0][:, 1]]
            assert loops.shape[0] >= 100 and all(tuple(t) in have for t in loops)


# ---- the sampler with values, the device plan, the product ------------------------------------------------------------------------
_samplers = {}


def _sampler(pkg, ctx, fanout, keep, rescale):
    """(edge_sampler, its drawn pair, per side the downloaded (indptr, indices, values)) on kernel_graph_long; made once"""
    key = (fanout, keep, rescale)
    if key not in _samplers:
        es = import_module(pkg.__name__ + ".edge_sample")
        ip, ix, v, *_ = GRAPHS["long"]
        F = pkg.csr_matrix(ip, ix, v, 320)
        F_T = F.transpose()
        np.testing.assert_array_equal(F_T.data, GRAPHS["longT"][2])
        sampler = es.edge_sampler(F, F_T, fanout, keep, rescale=rescale, max_d=132)
        pair = sampler.draw(ctx, SEED, EPOCH)
        host = [(*S.numpy(), S.values_numpy()) for S in pair]
        _samplers[key] = (sampler, pair, host)
    return _samplers[key]


@pytest.mark.parametrize("rescale", ["row", "inverse"])
def test_sampler_draws_the_restated_pair_with_values(pkg, ctx, rescale):
    sampler, pair, host = _sampler(pkg, ctx, 16, 0.75, rescale)
    thr = ref.thresholds(GRAPHS["long"][0], 16, 0.75)
    np.testing.assert_array_equal(sampler.thr_host, thr)
    scale = sampler._scale.cpu().numpy()
    if rescale == "inverse":
        np.testing.assert_array_equal(scale.view(np.uint32), vref.inverse_factors(thr).view(np.uint32))
    for side, S, (sp, sx, sv) in zip(("long", "longT"), pair, host):
        ip, ix, v, transposed, *_ = GRAPHS[side]
        _, want_ip, want_ix, want_v = vref.sample_val(ip, ix, v, thr, transposed, scale, rescale == "row", seed=SEED, epoch=EPOCH)
        np.testing.assert_array_equal(sp, want_ip)
        np.testing.assert_array_equal(sx, want_ix)
        np.testing.assert_array_equal(sv.view(np.uint32), want_v.view(np.uint32))
        assert S.device()[2] is not None and S.plan is not None and S.plan.built and 0 < S.nnz() < int(ip[-1])
    for name in ("sample-count", "sample-scan", "sample-compact", "sample-plan"):
        assert name in ctx.timers and ctx.measure(name) >= 0.0


@pytest.mark.parametrize("split", [64, 512])
def test_device_plan_tables(pkg, ctx, split):
    """capacity from the parent, the tables of a sample, then of a second, smaller sample in the same buffers: both tables and
    the three totals equal the restatement, and nothing beyond the totals is touched (the tables start as 0xFF bytes)"""
    _, big_pair, big = _sampler(pkg, ctx, None, 0.5, "row")
    _, small_pair, small = _sampler(pkg, ctx, 16, 0.75, "row")
    for side in (0, 1):
        parent_ip = GRAPHS[("long", "longT")[side]][0]
        plan = pkg.ops.spmm_dev_plan(ctx, parent_ip, 128, split)
        assert (plan.cap_items, plan.cap_slots, plan.cap_split) == vref.capacity(parent_ip, split) and plan.split == split
        items, rows, _ = plan.read()
        assert (items == FULL).all() and (rows == FULL).all()
        previous = None
        for pair, host in ((big_pair, big), (small_pair, small)):
            pkg.ops.spmm_dev_plan_build(ctx, plan, pair[side].device()[0])
            items, rows, totals = plan.read()
            want_items, want_rows, want_totals = vref.rowsplit_tables(host[side][0], split)
            assert tuple(int(t) for t in totals) == want_totals
            np.testing.assert_array_equal(items[:want_totals[0]], want_items)
            np.testing.assert_array_equal(rows[:want_totals[2]], want_rows)
            if previous is None:
                assert (items[want_totals[0]:] == FULL).all() and (rows[want_totals[2]:] == FULL).all()
                if side == 0:
                    assert want_totals[0] < plan.cap_items and (split != 64 or 0 < want_totals[2] <= plan.cap_split)
            else:                                                         # what the smaller build did not reach is the first's
                np.testing.assert_array_equal(items[want_totals[0]:], previous[0][want_totals[0]:])
                np.testing.assert_array_equal(rows[want_totals[2]:], previous[1][want_totals[2]:])
            previous = (items, rows)
        # the parent itself fills the capacity exactly
        ip, ix, v, *_ = GRAPHS[("long", "longT")[side]]
        pkg.ops.spmm_dev_plan_build(ctx, plan, _u32(parent_ip))
        assert tuple(int(t) for t in plan.read()[2]) == (plan.cap_items, plan.cap_slots, plan.cap_split)


def _host_rowsplit(pkg, ctx, csr, ld_b, B_t, C0, d, alpha, beta, flags):
    """mggcn_spmm_csr_f32 with the host row-split plan of ``csr`` (the environment picks form and split) on raw operands"""
    torch = _torch()
    C = torch.from_numpy(C0.copy()).cuda()
    buf = pkg.ops.spmm_plan_for(ctx, csr, 132, d)
    assert buf.num_sweep_tasks() == 0
    ipd, ixd, dvd = csr.device(ctx.device)
    ctx.lib.mggcn_spmm_csr_f32(ctx.stream(0), buf.handle, csr.n(), csr.m(), ipd.data_ptr(), ixd.data_ptr(), dvd.data_ptr(),
                               B_t.data_ptr(), ld_b, C.data_ptr(), d, d, alpha, beta, flags, 0.01)
    ctx.sync()
    return C.cpu().numpy(), buf


@pytest.mark.parametrize("split", [64, 512])
def test_spmm_dev_equals_the_host_row_split_plan_bit_for_bit(pkg, ctx, monkeypatch, split):
    torch = _torch()
    monkeypatch.setenv("MGGCN_SPMM_ALGO", "rowsplit")
    monkeypatch.setenv("MGGCN_SPMM_SPLIT", str(split))
    _, pair, host = _sampler(pkg, ctx, None, 0.5, "row")
    rng = np.random.default_rng(split)
    for side in (0, 1):
        S, (sp, sx, sv) = pair[side], host[side]
        csr = pkg.csr_matrix(sp.copy(), sx.copy(), sv.copy(), 320)
        plan = pkg.ops.spmm_dev_plan(ctx, GRAPHS[("long", "longT")[side]][0], 132, split)
        pkg.ops.spmm_dev_plan_build(ctx, plan, S.device()[0])
        # (width, leading dimension of B, alpha, beta, flags): every path of the dispatch, a pitch that breaks the vector path,
        # alpha / beta != (1, 0), the leaky-ReLU epilogue
        cases = [(1, 1, 1.0, 0.0, 0), (3, 3, 1.0, 0.0, 0), (41, 41, 0.5, 2.0, 0), (64, 64, 1.0, 0.0, 1), (128, 128, 1.0, 0.0, 0),
                 (132, 132, 0.5, 2.0, 1), (128, 130, 1.0, 0.0, 0), (128, 132, 0.5, 2.0, 1), (32, 32, 1.0, 0.0, 0)]
        for d, ldb, alpha, beta, flags in cases:
            Bfull = rng.standard_normal((320, ldb)).astype(np.float32)
            C0 = rng.standard_normal((320, d)).astype(np.float32)
            B_t = torch.from_numpy(Bfull).cuda()
            want, buf = _host_rowsplit(pkg, ctx, csr, ldb, B_t, C0, d, alpha, beta, flags)
            if split == 64 and side == 0:
                assert buf.num_split_rows() > 0
            C = pkg.dn_matrix.from_numpy(C0.copy())
            pkg.ops.spmm_dev(ctx, S, B_t[:, :d], C, plan, alpha, beta, flags)
            ctx.sync()
            got = C.numpy()
            np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=f"side {side} d {d} ldb {ldb}")
            again = pkg.dn_matrix.from_numpy(C0.copy())
            pkg.ops.spmm_dev(ctx, S, B_t[:, :d], again, plan, alpha, beta, flags)
            ctx.sync()
            np.testing.assert_array_equal(again.numpy().view(np.uint32), got.view(np.uint32))
            if ldb == d and d in (41, 128):
                # through ops.matmul as the models call it, and bf16: the fp32 product of the widened image, bit for bit
                Cm = pkg.dn_matrix.from_numpy(C0.copy())
                pkg.ops.matmul(ctx, csr, pkg.dn_matrix.from_numpy(Bfull), Cm, buf, alpha, beta, flags)
                ctx.sync()
                np.testing.assert_array_equal(Cm.numpy().view(np.uint32), got.view(np.uint32))
                B16 = B_t.to(torch.bfloat16)
                C16, Cw = pkg.dn_matrix.from_numpy(C0.copy()), pkg.dn_matrix.from_numpy(C0.copy())
                pkg.ops.spmm_dev(ctx, S, B16, C16, plan, alpha, beta, flags)
                pkg.ops.spmm_dev(ctx, S, pkg.dn_matrix.from_numpy(B16.float().cpu().numpy()), Cw, plan, alpha, beta, flags)
                ctx.sync()
                np.testing.assert_array_equal(C16.numpy().view(np.uint32), Cw.numpy().view(np.uint32))
            if (d, ldb, flags) == (128, 128, 0):
                dense = np.zeros((320, 320))
                rows = np.repeat(np.arange(320), np.diff(sp.astype(np.int64)))
                np.add.at(dense, (rows, sx.astype(np.int64)), sv.astype(np.float64))
                ref64 = alpha * (dense @ Bfull[:, :d].astype(np.float64)) + beta * C0
                den = np.maximum(np.abs(ref64).max(axis=1), 1e-2 * np.abs(ref64).max()) + 1e-30
                assert float((np.abs(got - ref64).max(axis=1) / den).max()) <= TOL


def test_wrappers_refuse_bad_arguments(pkg, ctx):
    _, pair, _ = _sampler(pkg, ctx, None, 0.5, "row")
    S = pair[0]
    B, C = pkg.dn_matrix(320, 16), pkg.dn_matrix(320, 16)
    fresh = pkg.ops.spmm_dev_plan(ctx, GRAPHS["long"][0], 16, 64)
    with pytest.raises(ValueError, match="built"):
        pkg.ops.spmm_dev(ctx, S, B, C, fresh)
    pkg.ops.spmm_dev_plan_build(ctx, fresh, S.device()[0])
    with pytest.raises(ValueError, match="max_d"):
        pkg.ops.spmm_dev(ctx, S, pkg.dn_matrix(320, 32), pkg.dn_matrix(320, 32), fresh)
    with pytest.raises(ValueError, match="shape"):
        pkg.ops.spmm_dev(ctx, S, pkg.dn_matrix(300, 16), C, fresh)
    with pytest.raises(ValueError, match="values"):
        pkg.ops.edge_sample_rowscale(ctx, 320, S.device()[0], S.device()[1], S.device()[1], S.device()[0], S.device()[0],
                                     S.device()[2])
    ctx.sync()
