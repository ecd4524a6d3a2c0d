"""The row-partitioned GAT without a GPU: dist_row_csr_matrix.row_block_global(), the numpy restatement of the partitioned
algebra (dist_gat_ref.py) against the whole-graph restatement, the conditions that let the device tests see an offset bug,
the packed destination record's layout, and the constructor's refusals."""
from types import SimpleNamespace

import numpy as np
import pytest

import dist_gat_ref as dgr
import gat_ref as ref
from gat_ref import rowdist

EXACT = 1e-12


def _csr(pkg, indptr, indices, n):
    data = np.random.default_rng(7).standard_normal(indices.size).astype(np.float32)      # values travel with their entries
    return pkg.csr_matrix(indptr.copy(), indices.copy(), data, n)


@pytest.mark.parametrize("P", [1, 2, 4])
@pytest.mark.parametrize("transposed", [False, True])
def test_row_block_global_is_the_matrix_rows_entry_for_entry(pkg, P, transposed):
    """on kernel_graph_long (rows of up to 4097 entries in no column order) and on its transpose (ascending rows): indptr,
    indices and values of every rank's block equal the whole matrix's rows, from the whole matrix and from the rank's rows
    alone.  With keep_rows the rows are the source's own on both graphs; the default, the merge of the blocks, is that on
    the ascending graph, and on the unordered one every row sorted by block, entries of a block in their order"""
    indptr, indices = ref.kernel_graph_long()
    n = indptr.size - 1
    if transposed:
        indptr, indices = ref.transpose_pattern(indptr, indices, n)
    A = _csr(pkg, indptr, indices, n)
    p = pkg.dist.partition_bounds(n, P)
    for r in range(P):
        comm = SimpleNamespace(P=P, rank=r)
        lo, hi = int(indptr[p[r]]), int(indptr[p[r + 1]])
        ip = indptr[p[r]:p[r + 1] + 1] - indptr[p[r]]
        rows_only = pkg.csr_matrix(ip.copy(), indices[lo:hi].copy(), A.data[lo:hi].copy(), n)
        for keep in (True, False):
            for M in (pkg.dist.dist_row_csr_matrix(comm, A, p, p, keep_rows=keep),
                      pkg.dist.dist_row_csr_matrix(comm, rows_only, p, p, row_block=True, keep_rows=keep)):
                assert (M._rows is not None) == keep                  # nothing is held on to unless asked for
                B = M.row_block_global()
                assert B.shape() == (p[r + 1] - p[r], n) and M._rows is None and M.row_block_global() is B
                np.testing.assert_array_equal(B.indptr, ip)
                want_ix, want_dv = indices[lo:hi], A.data[lo:hi]
                if not keep and not transposed:                        # the merge: a stable sort of every row by block
                    rows = np.repeat(np.arange(ip.size - 1), np.diff(ip.astype(np.int64)))
                    block = np.searchsorted(np.asarray(p[1:]), want_ix, side="right")
                    order = np.lexsort((np.arange(want_ix.size), block, rows))
                    assert (order != np.arange(order.size)).any() or P == 1
                    want_ix, want_dv = want_ix[order], want_dv[order]
                np.testing.assert_array_equal(B.indices, want_ix)
                np.testing.assert_array_equal(B.data.view(np.uint32), want_dv.view(np.uint32))


def _close(got, want, what):
    want = np.asarray(want, dtype=np.float64)
    err = np.abs(np.asarray(got, dtype=np.float64).reshape(want.shape) - want).max() / max(1.0, np.abs(want).max())
    assert err <= EXACT, (what, err)


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("P", [2, 4])
@pytest.mark.parametrize("K,dh", dgr.OP_SHAPES)
def test_partitioned_restatement_is_the_whole_graph_restatement(K, dh, P, drop):
    """every output assembled from the ranks equals the exact whole-graph restatement at 1e-12 (plain: gat_ref.restate64;
    with attention dropout p = 0.5: gat_dropout_ref's, the mask drawn with the ranks' offsets), and G_att is the sum of the
    ranks' partials"""
    c, d = dgr.op_case(K, dh, drop)
    got = dgr.partitioned(c["indptr"], c["indices"], c["Z"], c["G"], c["att"], K, P, drop=d)
    for name in dgr.ROW_NAMES + ("G_att",):
        _close(got[name], c["want"][name], (name, K, dh, P, drop))
    assert len(got["G_att_partials"]) == P
    assert all(np.abs(x).max() > 0 for x in got["G_att_partials"])
    # the plain whole-graph G_att through the same path, for the dropout case too (its scale dict has no G_att entry)
    if not drop:
        assert rowdist(got["G_att"], c["want"]["G_att"], c["scale"]["G_att"]).max() <= EXACT


@pytest.mark.parametrize("P", [2, 4])
@pytest.mark.parametrize("K,dh", dgr.OP_SHAPES)
def test_an_offset_bug_on_one_rank_is_four_bars_away(K, dh, P):
    """the conditions: on a rank > 0, taking s_dst from rows [0, n/P), passing dst0 = 0 in the forward, and swapping dst0 /
    src0 in backward_src each move the restatement by at least four gat_ref.ROW_TOL in one of the row-local outputs, on the
    rows of that rank (the first needs no dropout and is checked without it too)"""
    plain, _ = dgr.op_case(K, dh, False)
    dropped, d = dgr.op_case(K, dh, True)
    n = plain["indptr"].size - 1
    for rank in sorted({1, P - 1}):
        lo, hi = rank * n // P, (rank + 1) * n // P
        for c, dd, mutations in ((plain, None, dgr.MUTATIONS[:1]), (dropped, d, dgr.MUTATIONS)):
            for mut in mutations:
                got = dgr.partitioned(c["indptr"], c["indices"], c["Z"], c["G"], c["att"], K, P, drop=dd, mutation=mut, rank=rank)
                worst = {nm: float(rowdist(got[nm], c["want"][nm], c["scale"][nm])[lo:hi].max()) for nm in dgr.ROW_NAMES}
                print(f"[dist-gat cpu] K={K} dh={dh} P={P} rank {rank} drop={dd is not None} {mut!r}: "
                      + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
                assert max(worst.values()) >= 4 * ref.ROW_TOL, (mut, rank, worst)
                if mut == dgr.MUTATIONS[2]:             # only backward_src is touched
                    assert max(worst[k] for k in ("out", "lse", "D", "ds_dst")) <= EXACT


def test_record_pack_then_unpack_is_exact():
    """the layout rec[(i K + k) 4 + {0, 1, 2, 3}] = s_dst, lse, D, 0 in numpy: bits in, bits out, NaN payloads, infinities
    and signed zeros included; the fourth float is +0.0"""
    rng = np.random.default_rng(1)
    n, K = 37, 3
    bits = rng.integers(0, 1 << 32, size=(3, n, K), dtype=np.uint64).astype(np.uint32)
    bits[0, 0, 0], bits[1, 0, 0], bits[2, 0, 0] = 0x7FC00001, 0xFF800000, 0x80000000
    s_dst, lse, D = (b.view(np.float32) for b in bits)
    rec = dgr.pack_dst(s_dst, lse, D)
    assert rec.shape == (n, K, 4) and rec.dtype == np.float32 and rec.flags["C_CONTIGUOUS"]
    flat = rec.reshape(-1).view(np.uint32)
    for i, k in ((0, 0), (5, 2), (n - 1, K - 1)):
        base = (i * K + k) * 4
        assert [int(x) for x in flat[base:base + 4]] == [int(bits[0, i, k]), int(bits[1, i, k]), int(bits[2, i, k]), 0]
    for got, want in zip(dgr.unpack_dst(rec), bits):
        np.testing.assert_array_equal(got.view(np.uint32), want)


def test_exchange_byte_count():
    """per rank and epoch: every layer's Z shard, G shard and records"""
    assert dgr.exchange_bytes(1024, 2, [48, 32, 32, 7], 4) == 512 * ((2 * 32 * 4 + 64) * 2 + (2 * 7 * 4 + 16))
    assert dgr.exchange_bytes(1024, 4, [16, 64, 8, 5], [2, 2, 1]) == 256 * ((512 + 32) + (64 + 32) + (40 + 16))


class _square:
    """a stand-in for a dist_row_csr_matrix with no data behind it: a refusal that needed the matrix or a device would fail
    on it with something other than ValueError"""

    def __init__(self, n, m=None):
        self._n, self._m = n, n if m is None else m

    def n(self): return self._n
    def m(self): return self._m


@pytest.mark.parametrize("kw,match", [
    (dict(heads=3), "not divisible"), (dict(heads=17), "heads"), (dict(heads=[4, 4]), "lists 2 layers"),
    (dict(sizes=[16, 2048, 5]), "1024"), (dict(dropout=1.0), "dropout"), (dict(attn_dropout=-0.1), "dropout"),
    (dict(attn_dropout=float("nan")), "dropout"), (dict(loss="hinge"), "loss"), (dict(sizes=[16]), "at least two sizes"),
])
def test_constructor_refuses_before_any_device_work(pkg, kw, match):
    kw = dict(dict(sizes=[16, 32, 32, 5]), **kw)
    sizes = kw.pop("sizes")
    dctx = SimpleNamespace(P=2, rank=1)                                         # no device, no process group
    with pytest.raises(ValueError, match=match):
        pkg.dist.dist_gat(dctx, _square(64), _square(64), sizes, **kw)


def test_constructor_refuses_a_bad_matrix_or_partition(pkg):
    dctx = SimpleNamespace(P=4, rank=0)
    with pytest.raises(ValueError, match="square"):
        pkg.dist.dist_gat(dctx, _square(64, 32), _square(32, 64), [16, 32, 5])
    with pytest.raises(ValueError, match="multiple"):
        pkg.dist.dist_gat(dctx, _square(66), _square(66), [16, 32, 5])
    with pytest.raises(ValueError, match="64 layers"):
        pkg.dist.dist_gat(dctx, _square(64), _square(64), [4] * 66 + [2], heads=1, attn_dropout=0.5)


def test_ops_refuse_a_bad_record_before_the_library(pkg):
    """ops.gat_pack_dst / gat_backward_src_rec need no context for their checks: a record of the wrong size or off 16-byte
    alignment raises ValueError (the library would print and exit)"""
    import torch

    class shape_only:
        def __init__(self, n, m):
            self._s = (n, m)

        def shape(self): return self._s
        def n(self): return self._s[0]
        def m(self): return self._s[1]

    s = shape_only(8, 4)
    with pytest.raises(ValueError, match="records"):
        pkg.ops.gat_pack_dst(None, s, s, s, torch.empty(8 * 4 * 4 - 4))
    with pytest.raises(ValueError, match="aligned"):
        pkg.ops.gat_pack_dst(None, s, s, s, torch.empty(8 * 4 * 4 + 1)[1:])
    F_T, Z = shape_only(8, 8), shape_only(8, 16)
    with pytest.raises(ValueError, match="records"):
        pkg.ops.gat_backward_src_rec(None, F_T, Z, torch.empty(8), s, Z, shape_only(2, 16), s, s, Z, 4)
