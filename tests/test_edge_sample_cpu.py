"""Per-epoch edge sampling without a GPU: the host thresholds of mg-gcn_amd/edge_sample.py against the restatement, the
properties of the rule itself on tests/edge_sample_ref.py (the two sides of a pair are transposes, duplicates share a bit,
self-loops stay, no counter is shared with the other masks, the rate), every refusal on a model object built without a
device, and the ABI."""
import os
import re
from importlib import import_module

import numpy as np
import pytest

import dropout_ref
import edge_sample_ref as ref
import gat_dropout_ref
import gat_ref
import label_input_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("mggcn_edge_sample_count_u32", "mggcn_edge_sample_scan_u32", "mggcn_edge_sample_compact_u32")


@pytest.fixture(scope="module")
def es(pkg):
    return import_module(pkg.__name__ + ".edge_sample")


# ---- thresholds ------------------------------------------------------------------------------------------------------------
def test_thresholds(es):
    indptr = np.array([0, 0, 1, 17, 33, 1033, 1033], dtype=np.uint32)           # degrees 0, 1, 16, 16, 1000, 0
    full = np.uint32(0xFFFFFFFF)
    t = es.thresholds(indptr, 16, 1.0)                                          # keep = 1, fanout >= deg: no draw at all
    assert (t[:4] == full).all() and t[5] == full
    assert t[4] == int(np.floor(16 / 1000 * 2.0 ** 32))
    assert (es.thresholds(indptr, None, 1.0) == full).all()                     # and so is "everything"
    assert (es.thresholds(indptr, None, 0.5) == np.uint32(0x80000000)).all()    # deg = 0 rows are harmless: q = keep
    below = np.nextafter(1.0, 0.0)                                              # q just below 1 does not wrap to 0
    assert (es.thresholds(indptr, None, below) == np.uint32(0xFFFFFFFF)).all()
    assert es.thresholds(indptr, None, below)[0] == int(np.floor(below * 2.0 ** 32)) == 0xFFFFFFFF
    assert es.thresholds(indptr, None, 1.0 - 2.0 ** -30)[0] == 0xFFFFFFFC
    tiny = es.thresholds(indptr, 1, 1e-12)
    assert (tiny == 0).all()                                                    # q 2^32 < 1: only self-loops survive
    for fanout, keep in ((None, 0.5), (16, 0.75), (1, 1.0), (10 ** 6, 1.0), (3, 0.3)):
        got = es.thresholds(indptr, fanout, keep)
        assert got.dtype == np.uint32
        np.testing.assert_array_equal(got, ref.thresholds(indptr, fanout, keep))
    g = gat_ref.kernel_graph_long()
    np.testing.assert_array_equal(es.thresholds(g[0], 16, 0.75), ref.thresholds(g[0], 16, 0.75))


# ---- the pair --------------------------------------------------------------------------------------------------------------
def _pair_case(name):
    if name == "long":
        indptr, indices = gat_ref.kernel_graph_long()
        return indptr, indices, 320, 0, 0
    indptr, indices, n_src = gat_ref.edge_graphs()["rect"]                      # 200 destinations x 320 sources
    return indptr, indices, n_src, 1000, 40                                     # the block's origin


@pytest.mark.parametrize("name", ["long", "rect"])
@pytest.mark.parametrize("fanout,keep", [(None, 0.5), (16, 0.75), (4, 1.0)])
def test_the_two_sides_are_transposes_entry_for_entry(name, fanout, keep):
    """the sample of F and the sample of transpose_pattern(F) are transposes, with the entry order the host transpose gives"""
    indptr, indices, n_src, dst0, src0 = _pair_case(name)
    thr = ref.thresholds(indptr, fanout, keep)
    t_indptr, t_indices = gat_ref.transpose_pattern(indptr, indices, n_src)
    for epoch in (0, 3):
        counts, ip, ix = ref.sample(indptr, indices, thr, 0, dst0, src0, seed=7, epoch=epoch)
        t_counts, tip, tix = ref.sample(t_indptr, t_indices, thr, 1, src0, dst0, seed=7, epoch=epoch)
        assert 0 < ix.size < indices.size
        want_ip, want_ix = gat_ref.transpose_pattern(ip, ix, n_src)
        np.testing.assert_array_equal(tip, want_ip)
        np.testing.assert_array_equal(tix, want_ix)
        np.testing.assert_array_equal(counts, np.diff(ip.astype(np.int64)))
        np.testing.assert_array_equal(t_counts, np.diff(tip.astype(np.int64)))


def test_duplicates_share_their_bit_and_self_loops_stay():
    indptr, indices = gat_ref.kernel_graph_long()
    indices = indices.copy()
    for r in range(20, 60):                                                     # plant self-loops
        if indptr[r + 1] > indptr[r]:
            indices[indptr[r]] = r
    b = int(indptr[gat_ref.LONG_DUPLICATE_ROW])
    assert indices[b] == indices[b + 1]
    rows = np.repeat(np.arange(320), np.diff(indptr.astype(np.int64)))
    loops = rows == indices
    assert loops.sum() >= 30
    flips = 0
    for epoch in range(40):
        kept = ref.keep_mask(indptr, indices, ref.thresholds(indptr, None, 0.5), seed=3, epoch=epoch)
        assert kept[b] == kept[b + 1]
        flips += int(kept[b])
        assert kept[loops].all()
        assert not kept[~loops].all()
    assert 5 <= flips <= 35                                                     # a fair bit, not a constant
    kept = ref.keep_mask(indptr, indices, np.zeros(320, dtype=np.uint32), seed=3, epoch=0)
    np.testing.assert_array_equal(kept, loops)                                  # threshold 0: the self-loops and nothing else
    assert ref.keep_mask(indptr, indices, np.full(320, 0xFFFFFFFF, dtype=np.uint32), seed=3).all()


def test_no_counter_is_shared_with_the_other_masks():
    """under one seed: the counter tuples of the sample, of feature dropout (dropout_ref.words), of attention dropout
    (gat_dropout_ref.words) and of the label mask (label_input_ref.words), each collected by recording what the restatement
    hands to Philox"""
    indptr, indices = gat_ref.kernel_graph_long()
    seen = {}

    def recording(name, fn, *a, **kw):
        got = []
        real = dropout_ref.philox4x32_10

        def spy(ctr, key):
            c = np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) for x in ctr])
            got.append(np.stack([x.reshape(-1) for x in c], axis=1))
            return real(ctr, key)
        mods = (dropout_ref, ref, gat_dropout_ref.dropout_ref, label_input_ref.dropout_ref)
        old = [m.philox4x32_10 for m in mods]
        for m in mods:
            m.philox4x32_10 = spy
        try:
            fn(*a, **kw)
        finally:
            for m, o in zip(mods, old):
                m.philox4x32_10 = o
        seen[name] = {tuple(int(x) for x in row) for row in np.concatenate(got)}

    dst, src, _ = ref.pairs(indptr, indices, 0)
    for epoch in (0, 1, 64, 65):                    # the epochs and the streams epoch * 64 + layer that could collide
        recording(("sample", epoch), ref.words, dst, src, 7, epoch)
        recording(("dropout", epoch), dropout_ref.words, 320, 130, 0, 7, epoch)
        recording(("attention", epoch), gat_dropout_ref.entry_words, indptr, indices, 16, 7, epoch)
        recording(("label", epoch), label_input_ref.words, np.arange(320), 7, epoch)
    sample = set().union(*(v for k, v in seen.items() if k[0] == "sample"))
    assert len(sample) == 4 * len({(int(a), int(b)) for a, b in zip(dst, src)})
    assert {c[2] for c in sample} == {ref.DOMAIN}
    for k, v in seen.items():
        if k[0] != "sample":
            assert v and not (v & sample), k
            assert ref.DOMAIN not in {c[2] for c in v}, k


# ---- the rate --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fanout,keep", [(None, 0.5), (16, 0.75)])
@pytest.mark.parametrize("epoch", [0, 1])
def test_the_rate_is_within_five_binomial_standard_deviations(fanout, keep, epoch):
    """over the distinct off-diagonal pairs with q < 1 of kernel_graph_long, seed 7: kept within 5 sigma of sum q.  Measured
    with this rule: z = 1.21, -1.69 (keep 0.5, epochs 0, 1) and 2.32, -2.32 (keep 0.75, fanout 16)."""
    indptr, indices = gat_ref.kernel_graph_long()
    thr = ref.thresholds(indptr, fanout, keep)
    dst, src, _ = ref.pairs(indptr, indices, 0)
    t = thr[dst.astype(np.int64)]
    _, first = np.unique(dst * np.uint64(1 << 32) + src, return_index=True)
    pick = np.zeros(dst.size, dtype=bool)
    pick[first] = True
    pick &= (dst != src) & (t != 0xFFFFFFFF)
    q = t[pick].astype(np.float64) / 2.0 ** 32
    assert q.size > 1000
    kept = ref.keep_mask(indptr, indices, thr, seed=7, epoch=epoch)[pick]
    z = (kept.sum() - q.sum()) / np.sqrt((q * (1 - q)).sum())
    print(f"[edge-sample] rate fanout={fanout} keep={keep} epoch={epoch}: {int(kept.sum())} of {q.size} kept, "
          f"expected {q.sum():.1f}, z = {z:.2f}")
    assert abs(z) <= 5.0


# ---- refusals on objects built without a device -------------------------------------------------------------------------------
def _tiny(pkg, n=8):
    return pkg.csr_matrix(np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32), np.ones(n, dtype=np.float32), n)


def _stand_in(pkg, cls="gat", **attrs):
    """a model object without a device, as test_gatdot_cpu.py builds its own"""
    mod = import_module(pkg.__name__ + "." + {"gat": "gat", "sage": "sage", "gcn": "gcn"}[cls])
    G = getattr(mod, cls).__new__(getattr(mod, cls))
    A = _tiny(pkg)
    G._sample_matrices = (A, A)
    for k, v in attrs.items():
        setattr(G, k, v)
    return mod, G


BAD = [dict(keep=0.0), dict(keep=-0.5), dict(keep=1.5), dict(keep=float("nan")), dict(keep="0.5"), dict(keep=True),
       dict(fanout=0), dict(fanout=-3), dict(fanout=2.5), dict(fanout="4"), dict(fanout=True)]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "-".join(f"{k}={v!r}" for k, v in b.items()))
def test_bad_arguments_are_refused_by_name_before_any_device_work(pkg, bad):
    name = next(iter(bad))
    A = _tiny(pkg)
    ctor = {("edge_keep" if k == "keep" else k): v for k, v in bad.items()}
    with pytest.raises(ValueError, match=name):
        pkg.gat(A, [4, 8, 3], heads=2, **ctor)
    with pytest.raises(ValueError, match=name):
        pkg.sage(A, [4, 8, 3], aggr="max", **ctor)
    for cls, attrs in (("gat", dict(variant="v1")), ("sage", dict(aggr="max"))):
        _, G = _stand_in(pkg, cls, **attrs)
        with pytest.raises(ValueError, match=name):
            G.set_sampling(seed=5, epoch=2, **bad)
        assert (G.sample_fanout, G.sample_keep, G.sample_seed, G.sample_epoch, G.sampler) == (None, 1.0, 0, 0, None)


def test_set_sampling_state_without_a_device(pkg, es):
    _, G = _stand_in(pkg, "gat", variant="v1")
    G.set_sampling(fanout=10, keep=0.5, seed=(1 << 64) + 5, epoch=3)
    assert (G.sample_fanout, G.sample_keep, G.sample_seed, G.sample_epoch) == (10, 0.5, 5, 3)
    assert isinstance(G.sampler, es.edge_sampler) and G.sampler.thr_host.dtype == np.uint32
    G.set_sampling(fanout=10 ** 6)                                              # every q is 1: still on (the identity case)
    assert G.sampler is not None and (G.sampler.thr_host == 0xFFFFFFFF).all()
    G.set_sampling()                                                            # off: no sampler
    assert G.sampler is None and (G.sample_fanout, G.sample_keep, G.sample_epoch) == (None, 1.0, 0)
    assert not es.sampling_on(None, 1.0) and es.sampling_on(None, 0.999) and es.sampling_on(10 ** 6, 1.0)


def test_edge_attr_refuses_sampling(pkg):
    A = _tiny(pkg)
    E = np.ones((A.nnz(), 2), dtype=np.float32)
    for kw in (dict(fanout=4), dict(edge_keep=0.5)):
        with pytest.raises(ValueError, match="edge_attr"):
            pkg.gat(A, [4, 8, 3], heads=2, edge_attr=E, **kw)
    _, G = _stand_in(pkg, "gat", variant="v1", edge_dim=2)
    with pytest.raises(ValueError, match="edge_attr"):
        G.set_sampling(keep=0.5)
    assert G.sampler is None and G.sample_keep == 1.0
    G.set_sampling()                                                            # off is not refused


def test_models_without_row_walk_kernels_refuse_sampling(pkg):
    A = _tiny(pkg)
    for make in (lambda **kw: pkg.gcn(A, [4, 8, 3], **kw), lambda **kw: pkg.sage(A, [4, 8, 3], aggr="mean", **kw)):
        with pytest.raises(ValueError, match="fanout"):
            make(fanout=4)
        with pytest.raises(ValueError, match="keep"):
            make(edge_keep=0.5)
        with pytest.raises(ValueError, match="keep"):
            make(edge_keep=0.0)
    for cls, attrs in (("gcn", {}), ("sage", dict(aggr="mean"))):
        _, G = _stand_in(pkg, cls, **attrs)
        with pytest.raises(ValueError, match="fanout"):
            G.set_sampling(fanout=4)
        with pytest.raises(ValueError, match="keep"):
            G.set_sampling(keep=0.5)
        G.set_sampling()                                                        # off is accepted
        assert getattr(G, "sampler", None) is None


def test_the_row_partition_does_not_take_the_arguments(pkg):
    dist = import_module(pkg.__name__ + ".dist")
    for cls in (dist.dist_gat, dist.dist_sage):
        for kw in (dict(fanout=4), dict(edge_keep=0.5)):
            with pytest.raises(TypeError):
                cls(None, None, None, [16, 32, 5], **kw)
        assert not hasattr(cls, "set_sampling")


def test_export_after_a_sampled_forward_is_refused(pkg):
    """attention_weights(ctx) and gat_layer.alpha without X, with None in the place of the context"""
    gat, G = _stand_in(pkg, "gat", variant="v1", heads=[2, 1])
    layers = []
    for cls, attn in ((gat.gat_layer, gat.attention), (gat.gatv2_layer, gat.attention_v2)):
        layer = cls.__new__(cls)
        layer.name, layer.H, layer.sample, layer.attn = "0_", object(), (object(), object()), attn.__new__(attn)
        layers.append(layer)
        with pytest.raises(ValueError, match="sampl"):
            layer.alpha(None)
    G.layers_ = layers
    with pytest.raises(ValueError, match="sampl"):
        G.attention_weights(None)
    with pytest.raises(ValueError, match="sampl"):
        G.attention_weights(None, layers=[1])


# ---- the ABI -----------------------------------------------------------------------------------------------------------------
def test_the_three_exports_are_declared_and_bound(pkg):
    text = open(os.path.join(ROOT, "include", "mggcn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in EXPORTS:
        assert re.search(r"\bvoid\s+%s\s*\(" % name, text), name
        assert name in pkg._lib.PROTOTYPES
    proto = pkg._lib.PROTOTYPES
    assert len(proto[EXPORTS[0]][1]) == 11 and len(proto[EXPORTS[1]][1]) == 4 and len(proto[EXPORTS[2]][1]) == 12
    for fn in ("edge_sample_count", "edge_sample_scan", "edge_sample_compact"):
        assert callable(getattr(pkg.ops, fn))
