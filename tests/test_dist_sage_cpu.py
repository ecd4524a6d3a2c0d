"""The row-partitioned GraphSAGE without a GPU: the exports, the two new entries of the ABI, every refusal of dist_sage(...)
and of the two new ops calls (before any device work: a stand-in context with no device and no process group), the host
helper that sorts a row block, and the numpy restatement of the packed (arg, gradient) record."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import sage_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the package ------------------------------------------------------------------------------------------------------------------
def test_exports(pkg):
    from importlib import import_module
    mod = import_module(pkg.__name__ + ".dist_sage")
    for name in ("dist_sage", "dist_sage_layer", "dist_max_aggregate"):
        assert getattr(pkg.dist, name) is getattr(mod, name) and name in mod.__all__
    assert issubclass(pkg.dist.dist_sage, pkg.dist.dist_model_base) and issubclass(pkg.dist.dist_sage_layer, pkg.sage_layer)
    assert callable(pkg.ops.agg_max_pack) and callable(pkg.ops.agg_max_backward_rec)
    for name in ("sage", "sage_layer", "max_aggregate"):                     # the single-GPU names stay where they were
        assert name in pkg.__all__


def test_both_entries_are_declared_and_bound(pkg):
    text = open(os.path.join(ROOT, "include", "mggcn.h")).read()
    lib = pkg._lib.load()
    for name in ("mggcn_agg_max_pack_f32", "mggcn_agg_max_backward_rec_f32"):
        assert re.search(r"\bvoid %s\s*\(" % name, text), name
        assert name in pkg._lib.PROTOTYPES and hasattr(lib, name)
    assert len(pkg._lib.PROTOTYPES["mggcn_agg_max_pack_f32"][1]) == 9
    assert len(pkg._lib.PROTOTYPES["mggcn_agg_max_backward_rec_f32"][1]) == 12


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
class _square:
    """a stand-in for a dist_row_csr_matrix with no data behind it: a refusal that needed the matrix or a device would fail
    on it with something other than ValueError"""

    def __init__(self, n, m=None):
        self._n, self._m = n, n if m is None else m

    def n(self): return self._n
    def m(self): return self._m


@pytest.mark.parametrize("kw,word", [
    (dict(aggr="sum"), "aggr"), (dict(aggr=None), "aggr"), (dict(mode="ring"), "mode"),
    (dict(aggr="max", mode="halo"), "mode"), (dict(aggr="max", mode="rounds"), "mode"),
    (dict(norm="batch"), "norm"), (dict(loss="hinge"), "loss"), (dict(dropout=1.0), "dropout"), (dict(dropout=-0.1), "dropout"),
])
@pytest.mark.parametrize("rank", [0, 1])
def test_constructor_refuses_options_before_any_device_work(pkg, kw, word, rank):
    dctx = SimpleNamespace(P=2, rank=rank)                                   # no device, no process group, no self_gather
    with pytest.raises(ValueError, match=word):
        pkg.dist.dist_sage(dctx, _square(64), _square(64), [16, 32, 5], **kw)
    assert vars(dctx) == dict(P=2, rank=rank)


@pytest.mark.parametrize("aggr", ["mean", "max"])
def test_constructor_refuses_a_bad_pair_or_partition(pkg, aggr):
    dctx = SimpleNamespace(P=4, rank=3)
    for A, A_T in ((_square(64, 32), _square(32, 64)), (_square(64), _square(32)), (_square(64), _square(64, 32))):
        with pytest.raises(ValueError, match="square"):
            pkg.dist.dist_sage(dctx, A, A_T, [16, 32, 5], aggr=aggr)
    with pytest.raises(ValueError, match="multiple"):
        pkg.dist.dist_sage(dctx, _square(66), _square(66), [16, 32, 5], aggr=aggr)


def test_checkpoints_are_refused_and_nothing_is_created(pkg, tmp_path):
    model = object.__new__(pkg.dist.dist_sage)          # the members refuse before they look at the model or the context
    path = tmp_path / "model.ckpt"
    for call in (lambda: model.save(None, str(path)), lambda: model.load(None, str(path)),
                 lambda: model._write_checkpoint(None, str(path), {}, False, 0)):      # what model_selector.save_best calls
        with pytest.raises(ValueError, match="sage"):
            call()
    assert not path.exists() and list(tmp_path.iterdir()) == [] and vars(model) == {}


def _dn(pkg, n, m, dtype=np.float32):
    return pkg.dn_matrix(n, m, dtype=dtype, device="cpu")


def test_ops_wrappers_refuse_before_the_library(pkg):
    import torch
    ops = pkg.ops
    indptr = np.arange(0, 14, 2, dtype=np.uint32)
    F_T = pkg.csr_matrix(indptr, np.arange(12, dtype=np.uint32) % 6, np.ones(12, dtype=np.float32), 6)
    arg, G, G_B = _dn(pkg, 6, 8, np.int32), _dn(pkg, 6, 8), _dn(pkg, 6, 8)
    rec = torch.empty(6 * 8 * 2, dtype=torch.int32)
    off = torch.empty(6 * 8 * 2 + 1, dtype=torch.float32)[1:]
    assert rec.data_ptr() % 8 == 0 and off.data_ptr() % 8 == 4
    cases = [
        (ops.agg_max_pack, (arg, G, rec[:-2]), {}, "records"),
        (ops.agg_max_pack, (arg, G, off), {}, "aligned"),
        (ops.agg_max_pack, (arg, G, rec.view(6, 16)[:, :8]), {}, "records"),              # not contiguous
        (ops.agg_max_pack, (arg, G, torch.empty(6 * 8 * 2, dtype=torch.int16)), {}, "records"),
        (ops.agg_max_pack, (_dn(pkg, 6, 8), G, rec), {}, "arg"),                          # fp32
        (ops.agg_max_pack, (None, G, rec), {}, "arg"),
        (ops.agg_max_pack, (_dn(pkg, 5, 8, np.int32), G, rec), {}, "arg"),
        (ops.agg_max_pack, (_dn(pkg, 6, 1025, np.int32), _dn(pkg, 6, 1025), rec), {}, "width"),
        (ops.agg_max_backward_rec, (F_T, rec[:-2], 8, G_B), {}, "records"),
        (ops.agg_max_backward_rec, (F_T, off, 8, G_B), {}, "aligned"),
        (ops.agg_max_backward_rec, (F_T, rec, 8, _dn(pkg, 5, 8)), {}, "shape"),
        (ops.agg_max_backward_rec, (F_T, rec, 7, G_B), {}, "shape"),
        (ops.agg_max_backward_rec, (F_T, rec, 8.0, G_B), {}, "shape"),
        (ops.agg_max_backward_rec, (F_T, torch.empty(6 * 1025 * 2, dtype=torch.int32), 1025, _dn(pkg, 6, 1025)), {}, "width"),
        (ops.agg_max_backward_rec, (F_T, rec, 8, G_B), dict(src0=0xFFFFFFFF), "src0"),
        (ops.agg_max_backward_rec, (F_T, rec, 8, G_B), dict(src0=-1), "src0"),
    ]
    for fn, args, kw, word in cases:
        with pytest.raises(ValueError, match=word):
            fn(None, *args, **kw)
    assert F_T._dev is None


# ---- the sorted row block -----------------------------------------------------------------------------------------------------
def _blocks(pkg, P):
    """sage_ref.kernel_pattern as the square pattern of 50 vertices (rows beyond the 40 are empty), its transposed rows --
    unsorted on purpose -- cut into P row blocks (of 12 or 13 rows at P = 4) with global columns"""
    indptr, indices, n = ref.kernel_pattern()
    indptr = np.concatenate((indptr, np.full(n + 1 - indptr.size, indptr[-1], dtype=np.uint32)))
    # the backward matrix: rows are sources, entries destinations, in an order that keeps duplicates apart
    rows = np.repeat(np.arange(n), np.diff(indptr.astype(np.int64)))
    order = np.lexsort((np.random.default_rng(5).random(indices.size), indices))
    t_indptr = np.concatenate(([0], np.cumsum(np.bincount(indices, minlength=n)))).astype(np.uint32)
    t_indices = rows[order].astype(np.uint32)
    bounds = [r * n // P for r in range(P + 1)]
    out = []
    for r in range(P):
        lo, hi = int(t_indptr[bounds[r]]), int(t_indptr[bounds[r + 1]])
        out.append(pkg.csr_matrix((t_indptr[bounds[r]:bounds[r + 1] + 1] - t_indptr[bounds[r]]).astype(np.uint32),
                                  t_indices[lo:hi].copy(), np.arange(lo, hi, dtype=np.float32), n))
    return (indptr, indices, n), (t_indptr, t_indices), bounds, out


@pytest.mark.parametrize("P", [1, 2, 4])
def test_sorted_row_block_is_ascending_and_partitions_the_backward(pkg, P):
    from importlib import import_module
    sorted_row_block = import_module(pkg.__name__ + ".dist_sage").sorted_row_block
    (indptr, indices, n), (t_indptr, t_indices), bounds, blocks = _blocks(pkg, P)
    lens = np.diff(t_indptr.astype(np.int64))
    assert (lens == 0).any()                                                   # an unreferenced source: an empty row
    d = 5
    rng = np.random.default_rng(2)
    B = rng.choice(np.array([-2, -1, -0.0, 0.0, 1, 2], dtype=np.float32), size=(n, d))
    _, arg = ref.agg_max(indptr, indices, B)
    G = rng.standard_normal((n, d))
    # the whole pattern, sorted by the reference's own transpose
    want = ref.agg_max_backward(*ref.transpose_pattern(indptr, indices, n), arg, G, n)
    got, saw_duplicate, saw_unsorted = [], False, False
    for r, blk in enumerate(blocks):
        before = (blk.indptr.copy(), blk.indices.copy(), blk.data.copy())
        S = sorted_row_block(blk)
        assert S.shape() == blk.shape() and (S.indptr == blk.indptr).all() and S.indices.dtype == np.uint32
        assert all((a == b).all() for a, b in zip(before, (blk.indptr, blk.indices, blk.data)))      # the block is left alone
        for j in range(S.n()):
            lo, hi = int(S.indptr[j]), int(S.indptr[j + 1])
            row, src = S.indices[lo:hi].astype(np.int64), blk.indices[lo:hi].astype(np.int64)
            assert (np.diff(row) >= 0).all() and (row == np.sort(src)).all()                   # ascending, duplicates kept
            saw_duplicate |= bool((np.diff(row) == 0).any())
            saw_unsorted |= bool((np.diff(src) < 0).any())
        got.append(ref.agg_max_backward(S.indptr, S.indices, arg, G, S.n(), src0=bounds[r]))
    assert saw_duplicate and saw_unsorted
    np.testing.assert_array_equal(np.concatenate(got), want)
    assert np.abs(want).max() > 0


# ---- the record ---------------------------------------------------------------------------------------------------------------
def pack(arg, G):
    """the record of mggcn_agg_max_pack_f32 in numpy: words 2c and 2c + 1 of row i are arg[i, c] and the bits of G[i, c]"""
    rec = np.empty((arg.shape[0], 2 * arg.shape[1]), dtype=np.uint32)
    rec[:, 0::2] = np.asarray(arg).view(np.uint32)
    rec[:, 1::2] = np.ascontiguousarray(G, dtype=np.float32).view(np.uint32)
    return rec.view(np.float32)


def test_record_pack_then_unpack_is_exact():
    rng = np.random.default_rng(1)
    n, d = 37, 5
    arg = rng.integers(0, 1 << 32, size=(n, d), dtype=np.uint64).astype(np.uint32)
    gbits = rng.integers(0, 1 << 32, size=(n, d), dtype=np.uint64).astype(np.uint32)
    arg[0, 0], gbits[0, 0], gbits[1, 0], gbits[2, 0], gbits[3, 0] = ref.NONE, 0x7FC00001, 0xFF800000, 0x80000000, 0xFFC12345
    rec = pack(arg, gbits.view(np.float32))
    assert rec.shape == (n, 2 * d) and rec.dtype == np.float32 and rec.flags["C_CONTIGUOUS"]
    assert (rec.view(np.uint32)[:, 0::2] == arg).all() and (rec.view(np.uint32)[:, 1::2] == gbits).all()
    flat = rec.reshape(-1).view(np.uint32)
    for i, c in ((0, 0), (5, 2), (n - 1, d - 1)):
        assert [int(x) for x in flat[(i * d + c) * 2:(i * d + c) * 2 + 2]] == [int(arg[i, c]), int(gbits[i, c])]
