"""The row-partitioned GATv2 without a GPU: the numpy restatement of the partitioned algebra (dist_gatv2_ref.py) against the
whole-graph restatement of gatv2_ref.py, the conditions that let the device tests see a partition bug, the fp32 twin of the
rank-summed G_att against the bar the device is held to, the packed (lse, D) record's layout, the bytes of the exchange, and
the refusals of dist_gat(variant=...) and of the two new ops calls."""
from types import SimpleNamespace

import numpy as np
import pytest

import dist_gatv2_ref as dgr
import gat_ref as ref
import gatv2_ref as v2
from gat_ref import rowdist

EXACT = 1e-12


@pytest.fixture(autouse=True)
def _the_model_this_file_restates(pkg):
    """dist_gatv2_ref.py speaks for dist_gat(variant="v2") and the packed record: without them there is nothing to hold to it"""
    assert hasattr(pkg.dist, "dist_attention_v2") and hasattr(pkg.dist, "dist_gatv2_layer")
    assert {"mggcn_gatv2_pack_dst_f32", "mggcn_gatv2_backward_src_rec_f32"} <= set(pkg._lib.PROTOTYPES)


def _close(got, want, what):
    want = np.asarray(want, dtype=np.float64)
    err = np.abs(np.asarray(got, dtype=np.float64).reshape(want.shape) - want).max() / max(1.0, np.abs(want).max())
    assert err <= EXACT, (what, err)


def _partitioned(c, K, P, **kw):
    return dgr.partitioned(c["indptr"], c["indices"], c["Zs"], c["Zd"], c["G"], c["att"], K, P, **kw)


@pytest.mark.parametrize("P", [1, 2, 4])
@pytest.mark.parametrize("K,dh", dgr.OP_SHAPES)
def test_partitioned_restatement_is_the_whole_graph_restatement(K, dh, P):
    """fp64, kernel_graph_long as F: every row-local output assembled from the ranks equals the exact whole-graph
    restatement at 1e-12, and G_att is the sum of the ranks' partials"""
    c = dgr.op_case(K, dh)
    got = _partitioned(c, K, P)
    for name in dgr.ROW_NAMES + ("G_att",):
        _close(got[name], c["want"][name], (name, K, dh, P))
    assert len(got["G_att_partials"]) == P
    assert all(np.abs(x).max() > 0 for x in got["G_att_partials"])
    _close(sum(got["G_att_partials"]), c["want"]["G_att"], ("partials", K, dh, P))
    assert rowdist(got["G_att"], c["want"]["G_att"], c["scale"]["G_att"]).max() <= EXACT


@pytest.mark.parametrize("P", [2, 4])
@pytest.mark.parametrize("K,dh", dgr.OP_SHAPES)
def test_a_partition_bug_on_one_rank_is_a_hundred_bars_away(K, dh, P):
    """the conditions: on a rank > 0 each mutation of dist_gatv2_ref.MUTATIONS moves one of the outputs by at least 100 bars
    (gatv2_ref.BAR) on the row-scaled measure -- a row-local output on the rows of that rank, or the total G_att.  "local
    lse/D" touches backward_src alone and "att_grad whole" G_att alone.
    The weakest margin found over the three shapes, P = 2 and 4 and ranks 1 and P - 1, per mutation: "att_grad whole" 421
    bars (G_att at (4, 32), P = 2, rank 1: the other rank's partial is 3.4e-2 of the column's scale), "Zd rows" 38635 bars
    (P at (4, 32), P = 4, rank 3), "halves swapped" 764502 bars (out at (3, 7), P = 4, rank 3), "local lse/D" 1790546 bars
    (G_Zs at (3, 7), P = 2, rank 1)."""
    c = dgr.op_case(K, dh)
    n = c["n"]
    for rank in sorted({1, P - 1}):
        lo, hi = rank * n // P, (rank + 1) * n // P
        for mut in dgr.MUTATIONS:
            got = _partitioned(c, K, P, mutation=mut, rank=rank)
            worst = {nm: float(rowdist(got[nm], c["want"][nm], c["scale"][nm])[lo:hi].max()) for nm in dgr.ROW_NAMES}
            worst["G_att"] = float(rowdist(got["G_att"], c["want"]["G_att"], c["scale"]["G_att"]).max())
            margin = max(worst[nm] / v2.BAR[nm] for nm in worst)
            print(f"[dist-gatv2 cpu] K={K} dh={dh} P={P} rank {rank} {mut!r}: {margin:.1f} bars; "
                  + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
            assert margin >= 100, (mut, rank, worst)
            if mut == "local lse/D":                 # only backward_src is touched
                assert max(worst[k] for k in ("out", "lse", "D", "G_Zd", "P", "G_att")) <= EXACT
            if mut == "att_grad whole":              # only the sum over the ranks
                assert max(worst[k] for k in dgr.ROW_NAMES) <= EXACT


@pytest.mark.parametrize("P", [1, 2, 4])
@pytest.mark.parametrize("K,dh", dgr.OP_SHAPES)
def test_the_fp32_twin_of_the_rank_summed_G_att_earns_ROW_TOL(K, dh, P):
    """the partitioned algebra in fp32, the partials added in fp32 in rank order: G_att stays within ROW_TOL / 8 of the exact
    restatement on its scale, so gatv2_ref.bar_rule gives ROW_TOL = gatv2_ref.BAR["G_att"] for the device's all-reduced G_att
    too -- fixed here, before any device run"""
    c = dgr.op_case(K, dh)
    with np.errstate(over="ignore"):
        got = _partitioned(c, K, P, T=np.float32)
    assert got["G_att"].dtype == np.float32
    worst = float(rowdist(got["G_att"], c["want"]["G_att"], c["scale"]["G_att"]).max())
    print(f"[dist-gatv2 cpu] K={K} dh={dh} P={P} fp32 twin of the rank-summed G_att: {worst:.3e} (ROW_TOL / 8 = {ref.ROW_TOL / 8:.1e})")
    assert worst <= ref.ROW_TOL / 8
    assert v2.bar_rule(worst) == ref.ROW_TOL == v2.BAR["G_att"]


def test_record_pack_then_unpack_is_exact():
    """the layout rec[(i K + k) 2 + {0, 1}] = lse, D in numpy: bits in, bits out, NaN payloads, infinities and signed zeros
    included"""
    rng = np.random.default_rng(1)
    n, K = 37, 3
    bits = rng.integers(0, 1 << 32, size=(2, n, K), dtype=np.uint64).astype(np.uint32)
    bits[0, 0, 0], bits[1, 0, 0] = 0x7FC00001, 0x80000000             # a NaN with a payload, -0.0
    bits[0, 1, 0], bits[1, 1, 0] = 0x00000000, 0xFF800000             # +0.0, -inf
    bits[0, 2, 0], bits[1, 2, 0] = 0xFFC12345, 0x7F800000             # a negative NaN, +inf
    lse, D = (b.view(np.float32) for b in bits)
    rec = dgr.pack_dst(lse, D)
    assert rec.shape == (n, K, 2) and rec.dtype == np.float32 and rec.flags["C_CONTIGUOUS"]
    flat = rec.reshape(-1).view(np.uint32)
    for i, k in ((0, 0), (1, 0), (2, 0), (5, 2), (n - 1, K - 1)):
        base = (i * K + k) * 2
        assert [int(x) for x in flat[base:base + 2]] == [int(bits[0, i, k]), int(bits[1, i, k])]
    for got, want in zip(dgr.unpack_dst(rec), bits):
        np.testing.assert_array_equal(got.view(np.uint32), want)


def test_exchange_byte_count():
    """per rank and epoch: every layer's Z2 shard (2 out columns), G shard and 8-byte records"""
    assert dgr.exchange_bytes_v2(1024, 2, [48, 32, 32, 7], 4) == 512 * ((3 * 32 * 4 + 32) * 2 + (3 * 7 * 4 + 8))
    assert dgr.exchange_bytes_v2(1024, 4, [16, 64, 8, 5], [2, 2, 1]) == 256 * ((768 + 16) + (96 + 16) + (60 + 8))


class _square:
    """a stand-in for a dist_row_csr_matrix with no data behind it: a refusal that needed the matrix or a device would fail
    on it with something other than ValueError"""

    def __init__(self, n, m=None):
        self._n, self._m = n, n if m is None else m

    def n(self): return self._n
    def m(self): return self._m


@pytest.mark.parametrize("kw,match", [
    (dict(variant="v3"), "variant"), (dict(variant=None), "variant"), (dict(variant="v2", attn_dropout=0.1), "attention dropout"),
    (dict(variant="v2", heads=3), "not divisible"), (dict(variant="v2", attn_dropout=-0.1), "dropout"),
])
def test_constructor_refuses_before_any_device_work(pkg, kw, match):
    dctx = SimpleNamespace(P=2, rank=1)                                         # no device, no process group
    with pytest.raises(ValueError, match=match):
        pkg.dist.dist_gat(dctx, _square(64), _square(64), [16, 32, 32, 5], **kw)


def test_constructor_refuses_a_partition_that_does_not_divide(pkg):
    dctx = SimpleNamespace(P=4, rank=0)
    with pytest.raises(ValueError, match="multiple"):
        pkg.dist.dist_gat(dctx, _square(66), _square(66), [16, 32, 5], variant="v2")
    with pytest.raises(ValueError, match="square"):
        pkg.dist.dist_gat(dctx, _square(64, 32), _square(32, 64), [16, 32, 5], variant="v2")


def test_set_dropout_refuses_attention_dropout_for_v2_and_stores_nothing(pkg):
    """dist_gat borrows gat.set_dropout, which reads ``variant``: on a v2 model attn > 0 is a ValueError before anything is
    stored, feature dropout alone is taken; a v1 model takes both.  The stand-in holds what the constructor sets before any
    device work"""
    import sys
    cls = pkg.dist.dist_gat
    check_dropout = sys.modules[cls.__module__].check_dropout

    def stand_in(variant):
        G = cls.__new__(cls)
        G.variant = variant
        G._init_dropout(0.5, 3)
        G._attn_dropout_params, G.attn_dropout_p = check_dropout(0.0, 3), 0.0
        return G
    G = stand_in("v2")
    before = (G._dropout_params, G.dropout_p, G.dropout_seed, G.dropout_epoch, G._attn_dropout_params, G.attn_dropout_p)
    with pytest.raises(ValueError, match="attention dropout"):
        G.set_dropout(0.25, seed=5, epoch=9, attn=0.1)
    assert (G._dropout_params, G.dropout_p, G.dropout_seed, G.dropout_epoch, G._attn_dropout_params, G.attn_dropout_p) == before
    G.set_dropout(0.25, seed=5, epoch=9)
    assert (G.dropout_p, G.dropout_seed, G.dropout_epoch, G.attn_dropout_p) == (0.25, 5, 9, 0.0)
    G1 = stand_in("v1")
    G1.set_dropout(0.25, seed=5, epoch=9, attn=0.1)
    assert (G1.dropout_p, G1.attn_dropout_p) == (0.25, 0.1)


def test_ops_refuse_a_bad_record_before_the_library(pkg):
    """ops.gatv2_pack_dst / gatv2_backward_src_rec need no context for their checks: a record of the wrong size or off 8-byte
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
        pkg.ops.gatv2_pack_dst(None, s, s, torch.empty(8 * 4 * 2 - 2))
    with pytest.raises(ValueError, match="aligned"):
        pkg.ops.gatv2_pack_dst(None, s, s, torch.empty(8 * 4 * 2 + 1)[1:])
    with pytest.raises(ValueError, match="one shape"):
        pkg.ops.gatv2_pack_dst(None, s, shape_only(8, 2), torch.empty(8 * 4 * 2))
    F_T, Z, att = shape_only(8, 8), shape_only(8, 16), shape_only(1, 16)
    with pytest.raises(ValueError, match="records"):
        pkg.ops.gatv2_backward_src_rec(None, F_T, Z, Z, att, torch.empty(8), Z, Z, 4)
    with pytest.raises(ValueError, match="aligned"):
        pkg.ops.gatv2_backward_src_rec(None, F_T, Z, Z, att, torch.empty(8 * 4 * 2 + 1)[1:], Z, Z, 4)
