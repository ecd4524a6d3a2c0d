"""The edge-sample kernels (include/mggcn.h: mggcn_edge_sample_*_u32; csrc/edge_sample.hip) on the device against
tests/edge_sample_ref.py, exactly: counts, the scanned indptr and the compacted indices, with guard words around every
output and a sentinel behind the sample; and the consumers -- the attention kernels of all three variants and the max
aggregator -- on the device-resident sampled_csr pair against the same call on a csr_matrix built from the restated sample,
bit for bit."""
from importlib import import_module

import numpy as np
import pytest

import edge_sample_ref as ref
import gat_ref

pytestmark = pytest.mark.gpu

SENTINEL = 0x5EA1DEAD
GUARD = 64
FULL = 0xFFFFFFFF
SEED, EPOCH = 0x1234567887654321, 5


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


def _torch():
    import torch
    return torch


def _u32(a):
    return _torch().from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


class _out:
    """n output words between two guards of GUARD words, everything pre-filled with SENTINEL"""

    def __init__(self, n):
        self.n = n
        self.flat = _torch().full((n + 2 * GUARD,), int(np.uint32(SENTINEL).view(np.int32)), dtype=_torch().int32, device="cuda")
        self.t = self.flat[GUARD:GUARD + n]

    def words(self):
        return self.flat.cpu().numpy().view(np.uint32)

    def check(self, what, want, written=None):
        """the first ``written`` (default: all n) words equal ``want``; every other word, guards included, is the sentinel"""
        w = self.words()
        written = self.n if written is None else written
        np.testing.assert_array_equal(w[GUARD:GUARD + written], want, err_msg=what)
        rest = np.concatenate([w[:GUARD], w[GUARD + written:]])
        assert (rest == SENTINEL).all(), (what, "a word outside the output was written", np.flatnonzero(rest != SENTINEL)[:4])


def _graphs():
    """name -> (indptr, indices, transposed, row0, col0, rows the thresholds belong to): kernel_graph_long as F and as F^T
    (rows of 0, 1, 63, 64, 65, 127-129, 191-193, 1000 and 4097 entries, a duplicated pair, an empty last row), the same with
    self-loops planted, and the 200 x 320 block at its origin (1000, 40), as F and as F^T"""
    out = {}
    ip, ix = gat_ref.kernel_graph_long()
    looped = ix.copy()
    for r in range(0, 320, 3):
        if ip[r + 1] > ip[r]:
            looped[ip[r + 1] - 1] = r
    for name, idx in (("long", ix), ("loops", looped)):
        out[name] = (ip, idx, 0, 0, 0, ip)
        out[name + "T"] = (*gat_ref.transpose_pattern(ip, idx, 320), 1, 0, 0, ip)
    rp, rx = gat_ref.kernel_graph(200, 320)
    out["rect"] = (rp, rx, 0, 1000, 40, rp)
    out["rectT"] = (*gat_ref.transpose_pattern(rp, rx, 320), 1, 40, 1000, rp)
    return out


GRAPHS = _graphs()
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
    return np.array([0, FULL, 0x80000000], dtype=np.uint32)[np.arange(n) % 3]       # the three classes row by row


def _run(pkg, ctx, ip_d, ix_d, thr_d, n, transposed, row0, col0, capacity):
    ops = pkg.ops
    counts, indptr, indices = _out(n), _out(n + 1), _out(capacity)
    kw = dict(row0=row0, col0=col0, seed=SEED, epoch=EPOCH)
    ops.edge_sample_count(ctx, n, ip_d, ix_d, thr_d, transposed, counts.t, **kw)
    ops.edge_sample_scan(ctx, counts.t, n, indptr.t)
    ops.edge_sample_compact(ctx, n, ip_d, ix_d, thr_d, transposed, indptr.t, indices.t, **kw)
    ctx.sync()
    return counts, indptr, indices


@pytest.mark.parametrize("kind", THRESHOLDS)
@pytest.mark.parametrize("name", list(GRAPHS))
def test_count_scan_compact_equal_the_restatement(pkg, ctx, name, kind):
    ip, ix, transposed, row0, col0, dst_indptr = GRAPHS[name]
    n, nnz = ip.size - 1, int(ip[-1])
    thr = _thr(kind, dst_indptr)
    want_counts, want_ip, want_ix = ref.sample(ip, ix, thr, transposed, row0, col0, SEED, EPOCH)
    if kind == "full":
        assert want_ix.size == nnz
    if kind == "zero":                                              # the self-loops and nothing else
        dst, src, _ = ref.pairs(ip, ix, transposed, row0, col0)
        assert want_ix.size == int((dst == src).sum())
        assert want_ix.size >= 100 if name.startswith("loops") else want_ix.size == 0 if name.startswith("rect") else True
    ip_d, ix_d, thr_d = _u32(ip), _u32(ix), _u32(thr)
    first = _run(pkg, ctx, ip_d, ix_d, thr_d, n, transposed, row0, col0, nnz)
    for what, buf, want, written in (("counts", first[0], want_counts, None), ("indptr", first[1], want_ip, None),
                                     ("indices", first[2], want_ix, want_ix.size)):
        buf.check(f"{name} {kind} {what}", want, written)             # indices: the sentinel still stands behind indptr[n]
    # two calls give the same bits
    again = _run(pkg, ctx, ip_d, ix_d, thr_d, n, transposed, row0, col0, nnz)
    for a, b in zip(first, again):
        np.testing.assert_array_equal(a.words(), b.words())
    # a row range passed as a call of its own gives the same rows
    for r0, r1 in ((0, 3), (2, 14), (n - 5, n), (11, 13)):
        k = r1 - r0
        t_d = thr_d if transposed else thr_d[r0:]
        counts, indptr = _out(k), _out(k + 1)
        size = int(want_ip[r1]) - int(want_ip[r0])
        indices = _out(max(size, 1))
        kw = dict(row0=row0 + r0, col0=col0, seed=SEED, epoch=EPOCH)
        pkg.ops.edge_sample_count(ctx, k, ip_d[r0:], ix_d, t_d, transposed, counts.t, **kw)
        pkg.ops.edge_sample_scan(ctx, counts.t, k, indptr.t)
        pkg.ops.edge_sample_compact(ctx, k, ip_d[r0:], ix_d, t_d, transposed, indptr.t, indices.t, **kw)
        ctx.sync()
        counts.check(f"{name} {kind} rows {r0}:{r1} counts", want_counts[r0:r1])
        indptr.check(f"{name} {kind} rows {r0}:{r1} indptr", want_ip[r0:r1 + 1] - want_ip[r0])
        indices.check(f"{name} {kind} rows {r0}:{r1} indices", want_ix[int(want_ip[r0]):int(want_ip[r1])], size)


def test_an_epoch_and_a_seed_change_the_sample(pkg, ctx):
    ip, ix, *_ = GRAPHS["long"]
    thr = _thr("keep", ip)
    ip_d, ix_d, thr_d = _u32(ip), _u32(ix), _u32(thr)
    got = {}
    for seed, epoch in ((SEED, 0), (SEED, 1), (SEED + (1 << 32), 0), (SEED + 1, 0), (SEED, 1 << 31)):
        counts = _out(320)
        pkg.ops.edge_sample_count(ctx, 320, ip_d, ix_d, thr_d, 0, counts.t, seed=seed, epoch=epoch)
        ctx.sync()
        counts.check(f"seed {seed:#x} epoch {epoch}", ref.sample(ip, ix, thr, 0, 0, 0, seed, epoch)[0])
        got[seed, epoch] = counts.words().tobytes()
    assert len(set(got.values())) == len(got)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 511, 512, 513, 65536 + 1, 257 * 256 + 1])
def test_scan_alone(pkg, ctx, n):
    """the scan's workgroup is 256 counts: lengths on either side of one and two of them, of 256 of them (one turn of the
    pass over the block sums) and beyond (two turns)"""
    rng = np.random.default_rng(n)
    counts = rng.integers(0, 1000, size=n).astype(np.uint32)
    if n > 300:
        counts[256:300] = 0
    want = np.zeros(n + 1, dtype=np.uint32)
    want[1:] = np.cumsum(counts.astype(np.uint64)).astype(np.uint32)
    src = _out(max(n, 1))
    src.t[:n].copy_(_u32(counts))
    out = _out(n + 1)
    pkg.ops.edge_sample_scan(ctx, src.t, n, out.t)
    ctx.sync()
    out.check(f"scan of {n}", want)
    assert (src.words()[GUARD:GUARD + n] == counts).all()                       # the input is read only


def test_scan_wraps_modulo_two_to_the_32(pkg, ctx):
    counts = np.full(600, 0x01000000, dtype=np.uint32)
    want = np.zeros(601, dtype=np.uint32)
    want[1:] = (np.cumsum(counts.astype(np.uint64)) & np.uint64(FULL)).astype(np.uint32)
    out = _out(601)
    pkg.ops.edge_sample_scan(ctx, _u32(counts), 600, out.t)
    ctx.sync()
    out.check("wrapping scan", want)


# ---- the sampler and the consumers ---------------------------------------------------------------------------------------------
_pairs = {}


def _sampled_pair(pkg, ctx, fanout, keep):
    """(device pair of edge_sampler.draw, csr_matrix pair of the restated sample) on kernel_graph_long; made once"""
    key = (fanout, keep)
    if key not in _pairs:
        es = import_module(pkg.__name__ + ".edge_sample")
        ip, ix = gat_ref.kernel_graph_long()
        F = pkg.csr_matrix(ip, ix, np.ones(ix.size, dtype=np.float32), 320)
        F_T = F.transpose()
        sampler = es.edge_sampler(F, F_T, fanout, keep)
        dev = sampler.draw(ctx, SEED, EPOCH)
        (sp, sx), (tp, tx) = ref.sample_pair(ip, ix, fanout, keep, SEED, EPOCH)
        host = (pkg.csr_matrix(sp, sx, np.ones(sx.size, dtype=np.float32), 320),
                pkg.csr_matrix(tp, tx, np.ones(tx.size, dtype=np.float32), 320))
        _pairs[key] = (sampler, dev, host)
    return _pairs[key]


@pytest.mark.parametrize("fanout,keep", [(None, 0.5), (16, 0.75)])
def test_sampler_draws_the_restated_pair(pkg, ctx, fanout, keep):
    sampler, dev, host = _sampled_pair(pkg, ctx, fanout, keep)
    for d, h in zip(dev, host):
        assert (d.n(), d.m()) == (320, 320) and d.device()[2] is None
        indptr, indices = d.numpy()
        np.testing.assert_array_equal(indptr, h.indptr)
        np.testing.assert_array_equal(indices, h.indices)
        assert d.nnz() == h.nnz() < sampler.F.nnz()
    for name in ("sample-count", "sample-scan", "sample-compact"):
        assert name in ctx.timers and ctx.measure(name) >= 0.0


def _bits(t):
    return t.numpy().view(np.uint32).copy()


def _attention_outputs(pkg, ctx, variant, K, dh, F, F_T):
    """forward and backward of one attention over (F, F_T): ops.gat_* / ops.gatv2_* / ops.gatdot_* as the layers call them"""
    d, n = K * dh, 320
    zw = {"v1": 1, "v2": 2, "dot": 3}[variant]
    Z, _, G, _ = gat_ref.tolerance_inputs(n, n, K, zw * dh)
    Zd, Gd = pkg.dn_matrix.from_numpy(Z), pkg.dn_matrix.from_numpy(np.ascontiguousarray(G[:, :d]))
    out, G_Z = pkg.dn_matrix(n, d), pkg.dn_matrix(n, zw * d)
    ctx.fill(out, 0.0)
    ctx.fill(G_Z, 0.0)
    if variant == "v1":
        attn = pkg.attention("t_", n, n, d, K)
    elif variant == "v2":
        attn = pkg.attention_v2("t_", n, d, K)
    else:
        attn = pkg.attention_dot("t_", n, d, K)
    attn(ctx, F, Zd, out)
    attn.backward(ctx, F, F_T, Zd, Gd, out, G_Z)
    ctx.sync()
    res = dict(out=_bits(out), lse=_bits(attn.lse), D=_bits(attn.D), G_Z=_bits(G_Z))
    if variant == "v1":
        res.update(ds_dst=_bits(attn.ds_dst), ds_src=_bits(attn.ds_src), G_att=_bits(attn.G_att))
    elif variant == "v2":
        res.update(G_att=_bits(attn.G_att))
    return res


@pytest.mark.parametrize("variant,K,dh", [("v1", 4, 32), ("v1", 3, 7), ("v2", 4, 32), ("dot", 4, 32)])
def test_attention_kernels_on_the_sampled_pair(pkg, ctx, variant, K, dh):
    _, dev, host = _sampled_pair(pkg, ctx, None, 0.5)
    got = _attention_outputs(pkg, ctx, variant, K, dh, *dev)
    want = _attention_outputs(pkg, ctx, variant, K, dh, *host)
    full = _attention_outputs(pkg, ctx, variant, K, dh, *_full_pair(pkg))
    for name in want:
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)
    assert (got["out"] != full["out"]).any()                                    # and the sample is not the full graph


def _full_pair(pkg):
    ip, ix = gat_ref.kernel_graph_long()
    F = pkg.csr_matrix(ip, ix, np.ones(ix.size, dtype=np.float32), 320)
    return F, F.transpose()


@pytest.mark.parametrize("d", [128, 41])
def test_max_aggregator_on_the_sampled_pair(pkg, ctx, d):
    _, dev, host = _sampled_pair(pkg, ctx, 16, 0.75)
    rng = np.random.default_rng(d)
    B = pkg.dn_matrix.from_numpy(rng.standard_normal((320, d)).astype(np.float32))
    G = pkg.dn_matrix.from_numpy(rng.standard_normal((320, d)).astype(np.float32))
    res = []
    for F, F_T in (dev, host):
        out, arg, G_B = pkg.dn_matrix(320, d), pkg.dn_matrix(320, d, dtype=np.int32), pkg.dn_matrix(320, d)
        pkg.ops.agg_max_forward(ctx, F, B, out, arg)
        pkg.ops.agg_max_backward(ctx, F_T, arg, G, G_B)
        ctx.sync()
        res.append((_bits(out), arg.numpy().view(np.uint32).copy(), _bits(G_B)))
    for a, b, name in zip(res[0], res[1], ("out", "arg", "G_B")):
        np.testing.assert_array_equal(a, b, err_msg=name)
