"""ROC-AUC without a GPU: the numpy restatement (tests/auc_ref.py) against the O(P N) pair count on the floats, the known
answer, every refusal of ops.radix_sort_pairs / ops.roc_auc_keys / ops.roc_auc_stats / metrics.roc_auc_evaluator /
model.roc_auc / model_selector(metric="roc_auc") with None standing in for contexts and buffers, and the ABI."""
import math
import os
import re
import types
from importlib import import_module

import numpy as np
import pytest

import auc_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECIAL = np.array([-np.inf, -1.5, -0.0, 0.0, 1e-30, 2.0, np.inf], dtype=np.float32)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def test_restatement_against_the_pair_count():
    """a few hundred random cases up to 300 rows, half of them drawn from SPECIAL (ties, signed zeros, infinities)"""
    rng = np.random.default_rng(11)
    for case in range(300):
        n = int(rng.integers(1, 301))
        s = (rng.choice(SPECIAL, size=n) if case % 2 else rng.standard_normal(n).astype(np.float32))
        y = (rng.random(n) < rng.choice([0.0, 0.1, 0.5, 1.0], p=[0.05, 0.3, 0.6, 0.05])).astype(np.int32)
        got = ref.stats(s.reshape(n, 1), y.reshape(n, 1))[0][4]
        assert got == (ref.pair_count(s, y), int(y.sum()), int(n - y.sum())), case
        assert got == ref.stats(s.reshape(n, 1), y.reshape(n, 1))[0][0]         # without sets every row is slot 0


def test_restatement_by_slot_against_the_pair_count():
    rng = np.random.default_rng(12)
    for case in range(40):
        n = int(rng.integers(1, 301))
        s = rng.choice(SPECIAL, size=(n, 2)) if case % 2 else rng.standard_normal((n, 2)).astype(np.float32)
        y = (rng.random((n, 2)) < 0.3).astype(np.int32)
        sets = rng.choice([0, 1, 2, 7, -1], size=n)
        st = ref.stats(s, y, sets)
        slot = ref.slots_of(sets, n)
        for c in range(2):
            for k in range(5):
                m = np.ones(n, dtype=bool) if k == 4 else slot == k
                assert st[c][k] == (ref.pair_count(s[m, c], y[m, c]), int(y[m, c].sum()), int(m.sum() - y[m, c].sum()))


def test_the_key_map_is_monotone_and_ties_the_zeros():
    x = np.array([-np.inf, -3.0e38, -1.5, -1e-45, -0.0, 0.0, 1e-45, 1e-30, 2.0, 3.0e38, np.inf], dtype=np.float32)
    k = ref.keys_of(x).astype(np.int64)
    assert k[4] == k[5] == 0x80000000
    assert (np.diff(np.delete(k, 4)) > 0).all()
    rng = np.random.default_rng(3)
    a = rng.standard_normal(2000).astype(np.float32)
    np.testing.assert_array_equal(np.argsort(a, kind="stable"), np.argsort(ref.keys_of(a), kind="stable"))
    assert ref.vals_of(np.array([[0, 5], [1, 0]]), np.array([2, 9])).tolist() == [[4, 5], [7, 6]]


def test_known_answer():
    st = ref.stats(np.array([[0.1], [0.4], [0.35], [0.8]], dtype=np.float32), np.array([[0], [0], [1], [1]]))
    assert st[0][4] == (6, 2, 2)
    assert ref.summary(st)["all"] == 0.75 and ref.auc_of(*st[0][4]) == 0.75
    assert math.isnan(ref.summary(st)["val"])


def test_summarize_matches_the_restatement(pkg):
    rng = np.random.default_rng(5)
    y = (rng.random((200, 6)) < 0.3).astype(np.int32)
    y[:, 1], y[:, 4] = 1, 0
    st = ref.stats(rng.choice(SPECIAL, size=(200, 6)), y, rng.choice([0, 1, 2, 7], size=200))
    got, want = pkg.metrics.summarize(st), ref.summary(st)
    np.testing.assert_array_equal(got["per_class"], want["per_class"])
    assert np.isnan(got["per_class"][:, [1, 4]]).all() and not np.isnan(got["per_class"][4, [0, 2, 3, 5]]).any()
    for name in ref.VIEWS:
        assert got[name] == want[name] or (math.isnan(got[name]) and math.isnan(want[name]))
    assert got["stats"] is st and pkg.metrics.VIEWS == ref.VIEWS == pkg.ops.SPLIT_NAMES + ("all",)
    assert got["all"] == math.fsum(want["per_class"][4, [0, 2, 3, 5]]) / 4     # the single-label classes are skipped


# ---- refusals: the sort --------------------------------------------------------------------------------------------------------
class fake_tensor:
    """quacks like a contiguous device tensor of `numel` elements at `ptr`: nothing is ever dereferenced"""

    def __init__(self, ptr, numel, size=4, floating=False):
        self.ptr, self.n, self.size = ptr, numel, size
        self.is_cuda, self.dtype = True, types.SimpleNamespace(is_floating_point=floating)

    def data_ptr(self): return self.ptr
    def numel(self): return self.n
    def element_size(self): return self.size
    def is_contiguous(self): return True


def _four(total, base=1 << 20):
    return [fake_tensor(base + 16 * total * i, total) for i in range(4)]       # apart, with room between them


@pytest.mark.parametrize("bits", [(-1, 8), (0, 33), (8, 8), (9, 8), (32, 32), (0.0, 8), (0, True)])
def test_sort_refuses_a_bad_bit_range(pkg, bits):
    with pytest.raises(ValueError, match="begin_bit|end_bit"):
        pkg.ops.radix_sort_pairs(None, 1, 8, None, None, None, None, None, *bits)


def test_sort_refuses_two_to_the_31_pairs(pkg):
    for n_seg, seg_len in ((1, 1 << 31), (1 << 16, 1 << 15), (3, 715827883)):
        with pytest.raises(ValueError, match="2\\^31"):
            pkg.ops.radix_sort_pairs(None, n_seg, seg_len, None, None, None, None, None)
    with pytest.raises(ValueError, match="n_seg"):
        pkg.ops.radix_sort_pairs(None, -1, 8, None, None, None, None, None)
    with pytest.raises(ValueError, match="seg_len"):
        pkg.ops.radix_sort_pairs(None, 1, 2.5, None, None, None, None, None)


def test_sort_refuses_a_small_work_and_short_arrays(pkg):
    total = 3 * 5000
    need = pkg.ops.radix_sort_work_bytes(3, 5000)
    assert need == 4 * (2 * 3 * 256 * 2 + 1) and pkg.ops.radix_sort_work_bytes(0, 5) == 0 == pkg.ops.radix_sort_work_bytes(5, 0)
    arrays = _four(total)
    for work in (None, fake_tensor(1 << 30, need - 1, size=1), fake_tensor(1 << 30, need // 8 - 1, size=8)):
        with pytest.raises(ValueError, match="work"):
            pkg.ops.radix_sort_pairs(None, 3, 5000, *arrays, work)
    for i, name in enumerate(("keys", "vals", "keys_alt", "vals_alt")):
        short = list(arrays)
        short[i] = fake_tensor(arrays[i].ptr, total - 1)
        with pytest.raises(ValueError, match=name):
            pkg.ops.radix_sort_pairs(None, 3, 5000, *short, fake_tensor(1 << 30, need, size=1))
        with pytest.raises(ValueError, match=name):
            pkg.ops.radix_sort_pairs(None, 3, 5000, *[None if j == i else a for j, a in enumerate(arrays)], None)


def test_sort_refuses_any_aliasing(pkg):
    total = 1000
    work = fake_tensor(1 << 30, pkg.ops.radix_sort_work_bytes(1, total), size=1)
    names = ("keys", "vals", "keys_alt", "vals_alt")
    for i in range(4):
        for j in range(i + 1, 4):
            for shift in (0, 4, 4 * total - 4, -4 * total + 4):                 # the same array, and partial overlaps
                arrays = _four(total)
                arrays[j] = fake_tensor(arrays[i].ptr + shift, total)
                with pytest.raises(ValueError, match=f"{names[i]} and {names[j]}"):
                    pkg.ops.radix_sort_pairs(None, 1, total, *arrays, work)
    # and an empty sort is a no-op that needs nothing
    pkg.ops.radix_sort_pairs(None, 0, 10, None, None, None, None, None)
    pkg.ops.radix_sort_pairs(None, 10, 0, None, None, None, None, None)


# ---- refusals: keys and stats ----------------------------------------------------------------------------------------------------
def test_keys_and_stats_refuse_bad_operands(pkg):
    torch = import_module("torch")
    L, T = torch.zeros(6, 4), torch.zeros(6, 4, dtype=torch.int32)
    with pytest.raises(ValueError, match="logits"):
        pkg.ops.roc_auc_keys(None, None, T, None, 0, 4, None, None)
    with pytest.raises(ValueError, match="logits"):
        pkg.ops.roc_auc_keys(None, T, T, None, 0, 4, None, None)                # int32 logits
    with pytest.raises(ValueError, match="device"):
        pkg.ops.roc_auc_keys(None, L, T, None, 0, 4, None, None)                # host tensors
    with pytest.raises(ValueError, match="contiguous"):
        pkg.ops.roc_auc_keys(None, L.t(), T, None, 0, 4, None, None)
    with pytest.raises(ValueError, match="stats: n"):
        pkg.ops.roc_auc_stats(None, None, None, -1, 2, None, None)
    with pytest.raises(ValueError, match="2\\^31"):
        pkg.ops.roc_auc_stats(None, None, None, 1 << 31, 1, None, None)
    with pytest.raises(ValueError, match="2\\^31"):
        pkg.ops.roc_auc_stats(None, None, None, 1 << 20, 1 << 11, None, None)
    keys = fake_tensor(1 << 20, 2000)
    with pytest.raises(ValueError, match="stats: keys"):
        pkg.ops.roc_auc_stats(None, fake_tensor(1 << 20, 1999), keys, 1000, 2, None, None)
    with pytest.raises(ValueError, match="stats: stats"):
        pkg.ops.roc_auc_stats(None, keys, keys, 1000, 2, fake_tensor(1 << 24, 29, size=8), None)
    with pytest.raises(ValueError, match="work"):
        pkg.ops.roc_auc_stats(None, keys, keys, 1000, 2, fake_tensor(1 << 24, 30, size=8), None)
    assert pkg.ops.roc_auc_stats_work_bytes(0, 3) == 0 and pkg.ops.roc_auc_stats_work_bytes(1025, 3) == 3 * 256


# ---- refusals: the evaluator, the model member, the selector -----------------------------------------------------------------------
def test_evaluator_checks_its_options_and_groups_the_classes(pkg):
    ev = pkg.roc_auc_evaluator
    for bad in (dict(n=1 << 31, n_classes=2), dict(n=-1, n_classes=2), dict(n=2.0, n_classes=2)):
        with pytest.raises(ValueError, match="n must"):
            ev(**bad)
    with pytest.raises(ValueError, match="n_classes"):
        ev(10, 0)
    with pytest.raises(ValueError, match="max_workspace_bytes"):
        ev(10, 2, max_workspace_bytes=0)
    assert ev(132_534, 112).group == 112 and ev(232_968, 41).group == 41        # the default cap holds both shapes whole
    assert ev(1000, 41, max_workspace_bytes=16_000).group == 1
    assert ev(1000, 41, max_workspace_bytes=15_999).group == 1                  # below one class: g = 1 exceeds the cap
    assert ev(1000, 41, max_workspace_bytes=32_000).group == 2 and ev(1000, 41, max_workspace_bytes=47_999).group == 2
    assert ev(1000, 41, max_workspace_bytes=1 << 40).group == 41
    assert ev((1 << 31) - 1, 5, max_workspace_bytes=1 << 60).group == 1         # a sort call stays below 2^31 pairs
    e = ev(6, 4)
    assert e._arrays is None                                                    # nothing is allocated before the first call
    torch = import_module("torch")
    with pytest.raises(ValueError, match="logits"):
        e(None, torch.zeros(6, 3), torch.zeros(6, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="Y must"):
        e(None, torch.zeros(6, 4), torch.zeros(5, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="S must"):
        e(None, torch.zeros(6, 4), torch.zeros(6, 4, dtype=torch.int32), S=np.zeros(6, dtype=np.int32))
    assert e._arrays is None


def _stand_in(pkg, cls="gcn", loss="bce", n=8, width=3, S=None):
    mod = import_module(pkg.__name__ + "." + cls)
    G = getattr(mod, cls).__new__(getattr(mod, cls))
    G.loss, G._out_width, G.dropout_p = loss, width, 0.0
    G.A = types.SimpleNamespace(n=lambda: n)
    G.loss_layer = types.SimpleNamespace(S=S, counts=[4, 2, 2, 0])
    return G


@pytest.mark.parametrize("cls", ["gcn", "gat", "sage"])
def test_model_member_refuses_before_any_device_work(pkg, cls):
    with pytest.raises(ValueError, match="loss"):
        _stand_in(pkg, cls, loss="softmax").roc_auc(None, None, None)
    G = _stand_in(pkg, cls)
    with pytest.raises(ValueError, match="targets"):
        G.roc_auc(None, None, None)                                             # what check_targets says
    with pytest.raises(ValueError, match="targets"):
        G.roc_auc(None, None, np.zeros((8, 3), dtype=np.int32))
    with pytest.raises(ValueError, match="2\\^31"):
        _stand_in(pkg, cls, n=1 << 31).roc_auc(None, None, None)
    assert G._roc_auc_evaluator is None


def test_model_member_refuses_sets_of_the_wrong_shape(pkg):
    G = _stand_in(pkg)
    checks = pkg.metrics.model_roc_auc_checks
    for bad in (np.zeros(7, dtype=np.int32), np.zeros((8, 2), dtype=np.int32), np.zeros(8, dtype=np.float32)):
        with pytest.raises(ValueError, match="^S: "):
            checks(G, None, bad, targets=False)
    marker = object()
    assert checks(_stand_in(pkg, S=marker), None, None, targets=False) is marker    # S=None: the sets of set_splits
    assert checks(G, None, None, targets=False) is None


def test_selector_takes_roc_auc_and_still_refuses_auc(pkg):
    S = object()
    with pytest.raises(ValueError, match="metric"):
        pkg.model_selector(_stand_in(pkg, S=S), metric="auc")
    sel = pkg.model_selector(_stand_in(pkg, S=S), metric="roc_auc", patience=2)
    assert (sel.metric, sel.clean, sel.split, sel.history, sel.best_epoch) == ("roc_auc", True, "val", [], None)
    assert pkg.model_selector(_stand_in(pkg, S=S), metric="roc_auc", clean=True).clean
    with pytest.raises(ValueError, match="clean"):
        pkg.model_selector(_stand_in(pkg, S=S), metric="roc_auc", clean=False)
    with pytest.raises(ValueError, match="loss"):
        pkg.model_selector(_stand_in(pkg, loss="softmax", S=S), metric="roc_auc")
    with pytest.raises(ValueError, match="2\\^31"):
        pkg.model_selector(_stand_in(pkg, n=1 << 31, S=S), metric="roc_auc")
    with pytest.raises(ValueError, match="roc_auc"):
        pkg.model_selector(types.SimpleNamespace(loss_layer=types.SimpleNamespace(S=S, counts=[4, 2, 2, 0]), dropout_p=0.0),
                           metric="roc_auc")
    # higher is better, a NaN never improves
    sel.best_value = 0.5
    assert sel._improved(0.6) and not sel._improved(0.5) and not sel._improved(0.4) and not sel._improved(float("nan"))


def test_the_row_partition_has_neither_member(pkg):
    dist = import_module(pkg.__name__ + ".dist")
    for cls in (dist.dist_gcn, dist.dist_gat, dist.dist_sage):
        assert not hasattr(cls, "roc_auc") and not hasattr(cls, "_roc_auc_evaluator")
    for cls in (pkg.gcn, pkg.gat, pkg.sage):
        assert callable(cls.roc_auc)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_the_exports_are_declared_and_bound_with_their_arity(pkg):
    text = open(os.path.join(ROOT, "include", "mggcn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    arity = {"mggcn_radix_sort_work_bytes": ("size_t", 2), "mggcn_radix_sort_pairs_u32": ("void", 11),
             "mggcn_roc_auc_keys_f32": ("void", 11), "mggcn_roc_auc_stats_work_bytes": ("size_t", 2),
             "mggcn_roc_auc_stats_u64": ("void", 8)}
    for name, (res, k) in arity.items():
        m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)" % (res, name), text)
        assert m, name
        assert len(m.group(1).split(",")) == k, name
        assert len(pkg._lib.PROTOTYPES[name][1]) == k, name
    assert re.search(r"#define\s+MGGCN_RADIX_SORT_TILE\s+%d\b" % pkg.ops.RADIX_SORT_TILE, text)
    assert re.search(r"#define\s+MGGCN_ROC_AUC_CHUNK\s+%d\b" % pkg.ops.ROC_AUC_CHUNK, text)
    lib = pkg._lib.load()
    for n_seg, seg_len in ((1, 1), (3, 4095), (3, 4096), (41, 4097), (2, 70_001), (0, 9), (9, 0)):
        assert lib.mggcn_radix_sort_work_bytes(n_seg, seg_len) == pkg.ops.radix_sort_work_bytes(n_seg, seg_len)
    for n, nc in ((1, 1), (1024, 3), (1025, 3), (70_001, 2), (3001, 112), (0, 4), (4, 0)):
        assert lib.mggcn_roc_auc_stats_work_bytes(n, nc) == pkg.ops.roc_auc_stats_work_bytes(n, nc)
