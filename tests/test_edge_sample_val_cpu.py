"""Edge sampling with values (gcn / sage(aggr="mean") with edge_rescale=) without a GPU: the restatement
tests/edge_sample_val_ref.py against the package's host side (inverse factors, plan capacity) and against the host plan builder
itself (csrc/plan_host.cpp: rowsplit_build, compiled here), the properties of the rescaled sample, the option state on model
objects built without a device, every refusal by name, and the ABI."""
import os
import re
import subprocess
from importlib import import_module

import numpy as np
import pytest

import edge_sample_ref as ref
import edge_sample_val_ref as vref
import gat_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("mggcn_edge_sample_rowscale_f32", "mggcn_edge_sample_compact_val_f32", "mggcn_spmm_dev_plan_capacity",
           "mggcn_spmm_dev_plan_create", "mggcn_spmm_dev_plan_destroy", "mggcn_spmm_dev_plan_bytes", "mggcn_spmm_dev_plan_describe",
           "mggcn_spmm_dev_plan_build", "mggcn_spmm_dev_plan_read", "mggcn_spmm_csr_dev_f32", "mggcn_spmm_csr_dev_bf16")
SEED, EPOCH = 0x1234567887654321, 5


@pytest.fixture(scope="module")
def es(pkg):
    return import_module(pkg.__name__ + ".edge_sample")


def _values(nnz, seed=1):
    return np.random.default_rng(seed).uniform(0.5, 1.5, size=nnz).astype(np.float32)


# ---- the factors -------------------------------------------------------------------------------------------------------------
def test_inverse_factors_bit_for_bit(es):
    ip, _ = gat_ref.kernel_graph_long()
    edge = np.array([0, 1, 2, 3, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint32)
    assert es.inverse_factors(edge)[0] == 0.0 and es.inverse_factors(edge)[-1] == 1.0
    assert es.inverse_factors(edge)[5] == 2.0 and es.inverse_factors(edge)[1] == np.float32(2.0 ** 32)
    for thr in (edge, ref.thresholds(ip, 16, 0.75), ref.thresholds(ip, None, 0.5), ref.thresholds(ip, 3, 0.3)):
        got = es.inverse_factors(thr)
        assert got.dtype == np.float32 and np.isfinite(got).all()
        np.testing.assert_array_equal(got.view(np.uint32), vref.inverse_factors(thr).view(np.uint32))


@pytest.mark.parametrize("fanout,keep", [(None, 0.5), (16, 1.0), (4, 0.75)])
def test_row_rescale_preserves_row_sums_and_never_divides_by_zero(fanout, keep):
    ip, ix = gat_ref.kernel_graph_long()
    v = _values(ix.size)
    thr = ref.thresholds(ip, fanout, keep)
    r, whole, nothing, length = vref.row_factors(ip, ix, v, thr, seed=SEED, epoch=EPOCH)
    assert np.isfinite(r).all() and (r[nothing] == 0).all() and (r[whole] == 1).all() and (r[~nothing] >= 1).all()
    assert nothing[length == 0].all() and whole.any() and (~whole & ~nothing).any()
    _, sp, sx, sv = vref.sample_val(ip, ix, v, thr, 0, r.astype(np.float32), True, seed=SEED, epoch=EPOCH)
    rows = np.repeat(np.arange(320), np.diff(ip.astype(np.int64)))
    S = np.bincount(rows, weights=v.astype(np.float64), minlength=320)
    srows = np.repeat(np.arange(320), np.diff(sp.astype(np.int64)))
    Sk = np.bincount(srows, weights=sv.astype(np.float64), minlength=320)
    np.testing.assert_allclose(Sk[~nothing], S[~nothing], rtol=1e-5)
    assert (Sk[nothing] == 0).all()


@pytest.mark.parametrize("mode", ["row", "inverse"])
def test_the_two_sides_hold_the_same_value_bits(mode):
    """the factor is one array per destination: the rescaled samples of F and of transpose(F) are the same multiset of
    (destination, source, value bits), and self-loops are scaled only by "row" """
    ip, ix = gat_ref.kernel_graph_long()
    ix = ix.copy()
    for r in range(0, 320, 3):
        if ip[r + 1] > ip[r]:
            ix[ip[r + 1] - 1] = r
    v = _values(ix.size)
    thr = ref.thresholds(ip, 16, 0.75)
    if mode == "row":
        scale = vref.row_factors(ip, ix, v, thr, seed=SEED, epoch=EPOCH)[0].astype(np.float32)
    else:
        scale = vref.inverse_factors(thr)
    order = np.argsort(ix[: int(ip[-1])].astype(np.int64) * 320 + np.repeat(np.arange(320), np.diff(ip.astype(np.int64))), kind="stable")
    tp, tx = gat_ref.transpose_pattern(ip, ix, 320)
    rows = np.repeat(np.arange(320, dtype=np.uint32), np.diff(ip.astype(np.int64)))
    np.testing.assert_array_equal(tx, rows[order])
    tv = v[order]
    _, sp, sx, sv = vref.sample_val(ip, ix, v, thr, 0, scale, mode == "row", seed=SEED, epoch=EPOCH)
    _, stp, stx, stv = vref.sample_val(tp, tx, tv, thr, 1, scale, mode == "row", seed=SEED, epoch=EPOCH)
    a, b = vref.triples(sp, sx, sv, 0), vref.triples(stp, stx, stv, 1)
    assert 0 < a.shape[0] < ix.size
    np.testing.assert_array_equal(a, b)
    loops = a[:, 0] == a[:, 1]
    assert loops.sum() >= 50
    if mode == "inverse":                                   # the self-loops carry their parent's value bits
        parent = vref.triples(ip, ix, v, 0)
        have = {tuple(t) for t in parent[parent[:, 0] == parent[:, 1]]}
        assert all(tuple(t) in have for t in a[loops])


# ---- the plan rule -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [64, 512])
def test_capacity_is_the_worst_case_over_every_sample(pkg, split):
    """the rule is monotone in the row length, so the worst case over all subsets of a row's entries is the row itself: brute
    force over every shorter length, then the library's sum against the restatement's"""
    lib = pkg._lib.load()
    worst = [0, 0, 0]
    for length in range(0, 4200):
        cost = vref.row_cost(length, split)
        worst = [max(w, c) for w, c in zip(worst, cost)]
        assert list(cost) == worst, length                  # no shorter row costs more in any of the three
    assert vref.row_cost(split + split // 2, split) == (1, 0, 0) and vref.row_cost(split + split // 2 + 1, split)[2] == 1
    ip, ix = gat_ref.kernel_graph_long()
    tp, _ = gat_ref.transpose_pattern(ip, ix, 320)
    for indptr in (ip, tp, np.zeros(1, dtype=np.uint32), np.array([0, 0, 5000], dtype=np.uint32)):
        assert pkg.ops.spmm_dev_capacity(lib, indptr, split) == vref.capacity(indptr, split)
    cap = vref.capacity(ip, split)
    for fanout, keep in ((None, 0.5), (16, 1.0), (10 ** 6, 1.0)):
        _, sp, _ = ref.sample(ip, ix, ref.thresholds(ip, fanout, keep), 0, seed=SEED, epoch=EPOCH)
        assert all(s <= c for s, c in zip(vref.capacity(sp, split), cap))
    assert vref.capacity(ip, split) == vref.rowsplit_tables(ip, split)[2]
    assert pkg.ops.spmm_dev_capacity(lib, ip, 0) == vref.capacity(ip, 512)          # split 0: the default
    assert pkg.ops.spmm_dev_capacity(lib, ip, 7) == vref.capacity(ip, 64)           # the floor


def test_tables_in_row_order_are_the_host_builders_before_its_sort(tmp_path):
    """rowsplit_build (csrc/plan_host.cpp) compiled on the host: its items, stably sorted back by (row, beg), its split rows
    and its slot count equal the restatement's row-order tables -- the slice boundaries and the slot numbering of the device
    builder's contract are the host builder's"""
    src = tmp_path / "rs.cpp"
    src.write_text(
        '#include <cstdio>\n#include <cstdlib>\n#include <vector>\n#include "plan_host.h"\n'
        'int main(int argc, char **argv) { unsigned split = std::strtoul(argv[1], nullptr, 10); std::vector<uint32_t> ip;\n'
        '  for (int i = 2; i < argc; i++) ip.push_back((uint32_t)std::strtoul(argv[i], nullptr, 10));\n'
        '  auto rs = mggcn_plan::rowsplit_build((uint32_t)ip.size() - 1, ip.data(), split);\n'
        '  std::printf("%zu %zu %u\\n", rs.items.size(), rs.split_rows.size(), rs.n_slots);\n'
        '  for (auto &it : rs.items) std::printf("%u %u %u %u\\n", it.row, it.beg, it.end, it.slot);\n'
        '  for (auto &r : rs.split_rows) std::printf("%u %u %u %u\\n", r.row, r.first_slot, r.n_slots, r.pad); }\n')
    exe = tmp_path / "rs"
    csrc = os.path.join(ROOT, "mg-gcn_amd", "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-I", csrc, str(src), os.path.join(csrc, "plan_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    ip, ix = gat_ref.kernel_graph_long()
    tp, _ = gat_ref.transpose_pattern(ip, ix, 320)
    for indptr in (ip, tp):
        for split in (64, 512):
            out = subprocess.run([str(exe), str(split)] + [str(int(x)) for x in indptr], capture_output=True, text=True)
            assert out.returncode == 0, out.stderr
            lines = out.stdout.strip().splitlines()
            n_items, n_rows, n_slots = (int(x) for x in lines[0].split())
            body = np.array([ln.split() for ln in lines[1:]], dtype=np.uint64).astype(np.uint32).reshape(-1, 4)
            items, rows = body[:n_items], body[n_items:]
            items = items[np.lexsort((items[:, 1], items[:, 0]))]
            want_items, want_rows, totals = vref.rowsplit_tables(indptr, split)
            assert totals == (n_items, n_slots, n_rows)
            np.testing.assert_array_equal(items, want_items)
            np.testing.assert_array_equal(rows, want_rows)
            if split == 64 and indptr is ip:
                assert n_rows >= 2 and n_slots > 64                 # the 1000- and 4097-entry rows are sliced


# ---- option state on objects built without a device ------------------------------------------------------------------------------
def _tiny(pkg, n=8):
    return pkg.csr_matrix(np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32), np.ones(n, dtype=np.float32), n)


def _stand_in(pkg, cls, **attrs):
    mod = import_module(pkg.__name__ + "." + cls)
    G = getattr(mod, cls).__new__(getattr(mod, cls))
    A = _tiny(pkg)
    G._sample_matrices = (A, A)
    for k, v in attrs.items():
        setattr(G, k, v)
    return G


MODELS = [("gcn", {}), ("sage", dict(aggr="mean"))]


@pytest.mark.parametrize("cls,attrs", MODELS, ids=["gcn", "sage-mean"])
@pytest.mark.parametrize("mode", ["row", "inverse"])
def test_a_rescale_switches_sampling_on(pkg, es, cls, attrs, mode):
    G = _stand_in(pkg, cls, edge_rescale=mode, **attrs)
    G.set_sampling(fanout=4, seed=(1 << 64) + 5, epoch=3)
    assert (G.sample_fanout, G.sample_keep, G.sample_seed, G.sample_epoch, G.edge_rescale) == (4, 1.0, 5, 3, mode)
    assert isinstance(G.sampler, es.edge_sampler) and G.sampler.rescale == mode and G.sampler.thr_host.dtype == np.uint32
    assert (G.sampler.inv_host is not None) == (mode == "inverse")
    other = "inverse" if mode == "row" else "row"
    G.set_sampling(keep=0.5, rescale=other)                                     # rescale= replaces the model's ...
    assert G.edge_rescale == other and G.sampler.rescale == other and G.sample_keep == 0.5 and G.sample_fanout is None
    G.set_sampling(keep=0.5)                                                    # ... and None keeps it
    assert G.edge_rescale == other and G.sampler.rescale == other
    G.set_sampling()                                                            # off whatever edge_rescale says
    assert G.sampler is None and G.edge_rescale == other
    H = _stand_in(pkg, cls, **attrs)                                            # the class-level default is None ...
    assert H.edge_rescale is None
    H.set_sampling(fanout=4, rescale=mode)                                      # ... and set_sampling alone can switch it on
    assert H.sampler is not None and H.edge_rescale == mode


@pytest.mark.parametrize("cls,attrs", MODELS, ids=["gcn", "sage-mean"])
def test_refusals_by_name(pkg, cls, attrs):
    A = _tiny(pkg)
    make = (lambda **kw: pkg.gcn(A, [4, 8, 3], **kw)) if cls == "gcn" else (lambda **kw: pkg.sage(A, [4, 8, 3], aggr="mean", **kw))
    for bad in ("mean", "Row", 1, True, ""):
        with pytest.raises(ValueError, match="edge_rescale"):
            make(edge_rescale=bad)
        with pytest.raises(ValueError, match="edge_rescale"):
            make(edge_rescale=bad, fanout=4)
        G = _stand_in(pkg, cls, **attrs)
        with pytest.raises(ValueError, match="rescale"):
            G.set_sampling(fanout=4, rescale=bad)
        assert G.sampler is None and G.edge_rescale is None and G.sample_fanout is None
    # without a rescale: refused as before, and the text points at the argument that would allow it
    for kw, name in ((dict(fanout=4), "fanout"), (dict(edge_keep=0.5), "keep")):
        with pytest.raises(ValueError, match=name) as e:
            make(**kw)
        assert "edge_rescale=" in str(e.value)
    # range errors come first and still name their argument
    with pytest.raises(ValueError, match="keep"):
        make(edge_keep=0.0, edge_rescale="row")
    with pytest.raises(ValueError, match="fanout"):
        make(fanout=0, edge_rescale="row")
    G = _stand_in(pkg, cls, edge_rescale="row", **attrs)
    with pytest.raises(ValueError, match="fanout"):
        G.set_sampling(fanout=2.5)
    assert G.sampler is None and G.sample_fanout is None


def test_max_aggregation_refuses_a_rescale(pkg):
    A = _tiny(pkg)
    for kw in (dict(edge_rescale="row"), dict(edge_rescale="inverse", fanout=4)):
        with pytest.raises(ValueError, match="edge_rescale"):
            pkg.sage(A, [4, 8, 3], aggr="max", **kw)
    G = _stand_in(pkg, "sage", aggr="max")
    with pytest.raises(ValueError, match="rescale"):
        G.set_sampling(fanout=4, rescale="row")
    assert G.sampler is None and G.edge_rescale is None
    G.set_sampling(fanout=4)                                                    # and samples without one, as before
    assert G.sampler is not None and G.sampler.rescale is None


def test_hoisting_refuses_sampling_both_ways(pkg):
    A = _tiny(pkg)
    for kw in (dict(fanout=4), dict(edge_keep=0.5)):
        with pytest.raises(ValueError, match="hoist_first_aggregation"):
            pkg.gcn(A, [4, 8, 3], hoist_first_aggregation=True, edge_rescale="row", **kw)
    G = _stand_in(pkg, "gcn", edge_rescale="row", hoist_first_aggregation=True)
    with pytest.raises(ValueError, match="hoist_first_aggregation"):
        G.set_sampling(fanout=4)
    assert G.sampler is None
    G = _stand_in(pkg, "gcn", edge_rescale="row", agg_dtype="f32")
    G.set_sampling(fanout=4)
    with pytest.raises(ValueError, match="hoist_first_aggregation"):
        G.set_hoist_first_aggregation(True)
    assert G.hoist_first_aggregation is False


def test_models_that_do_not_take_the_argument(pkg):
    dist = import_module(pkg.__name__ + ".dist")
    for cls in (dist.dist_gcn, dist.dist_sage, dist.dist_gat):
        with pytest.raises(TypeError):
            cls(None, None, None, [16, 32, 5], edge_rescale="row")
    with pytest.raises(TypeError):
        pkg.gat(_tiny(pkg), [4, 8, 3], heads=2, edge_rescale="row")
    gat = import_module(pkg.__name__ + ".gat")
    G = gat.gat.__new__(gat.gat)
    with pytest.raises(TypeError):
        G.set_sampling(fanout=4, rescale="row")


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
def test_the_exports_are_declared_and_bound(pkg):
    text = open(os.path.join(ROOT, "include", "mggcn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in pkg._lib.PROTOTYPES
    proto = pkg._lib.PROTOTYPES
    assert len(proto["mggcn_edge_sample_rowscale_f32"][1]) == 12 and len(proto["mggcn_edge_sample_compact_val_f32"][1]) == 16
    assert proto["mggcn_spmm_csr_dev_f32"][1] == proto["mggcn_spmm_csr_f32"][1]
    assert proto["mggcn_spmm_csr_dev_bf16"][1] == proto["mggcn_spmm_csr_bf16"][1]
    for fn in ("edge_sample_rowscale", "edge_sample_compact_val", "spmm_dev_plan", "spmm_dev_plan_build", "spmm_dev", "spmm_dev_capacity"):
        assert callable(getattr(pkg.ops, fn))
