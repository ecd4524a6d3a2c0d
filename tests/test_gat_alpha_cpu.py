"""The host side of the attention-coefficient export, checked without a GPU: the reference stays within its own rules (the
fp32 twin inside the bar, no tolerance case near expf's underflow, rows that sum to one), the bar tells every mutation of
gat_alpha_ref apart by two orders of magnitude, and the wrappers and attention_weights refuse bad arguments on stand-ins
that own no device memory, before the library is touched."""
from importlib import import_module

import numpy as np
import pytest

import gat_alpha_ref as ar
import gat_ref as ref

VARIANTS = {"v1": (ar.case_v1, ar.mutations_v1), "v2": (ar.case_v2, ar.mutations_v2)}


# ---- the reference alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_twin_is_inside_the_bar_and_the_bar_follows_the_rule(variant):
    """the fp32 twin (its own scores and lse in fp32) against the fp64 restatement on every case: the worst distance is what
    gat_alpha_ref.TWIN_MEASURED records, and the bar is 8 x the larger of the two, rounded up, below gat_ref.ROW_TOL"""
    top = (0.0, None)
    for name, K, dh in ar.cases():
        c = VARIANTS[variant][0](name, K, dh)
        d, p = ar.worst(c["twin_alpha"], c["alpha"], c["cp"])
        print(f"[gat-alpha] {variant} twin {name} K={K} dh={dh}: {d:.3e} at entry {p[0]} head {p[1]}")
        assert d <= ar.BAR, (variant, name, K, dh, p, d)
        top = max(top, (d, (name, K, dh) + p))
    print(f"[gat-alpha] {variant} twin worst: {top[0]:.3e} at {top[1]} (recorded {ar.TWIN_MEASURED[variant]:.3e}, bar {ar.BAR:.1e})")
    assert 0.9 * ar.TWIN_MEASURED[variant] <= top[0] <= 1.02 * ar.TWIN_MEASURED[variant], top
    rule = 8 * max(ar.TWIN_MEASURED.values())
    assert rule <= ar.BAR <= 1.1 * rule and ar.BAR <= ref.ROW_TOL


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_no_tolerance_case_is_near_underflow_and_rows_sum_to_one(variant):
    """every exact alpha of every tolerance case is >= 2^-100 (the absolute rule is for the stress cases alone), the injected
    form (fp32 scalars on both sides) too, and every non-empty row sums to 1 in fp64; an empty row has no entry"""
    for name, K, dh in ar.cases():
        c = VARIANTS[variant][0](name, K, dh)
        assert c["alpha"].shape == (c["indices"].size, K) and c["cp"].shape == c["alpha"].shape
        assert c["alpha"].min() >= ar.TINY and c["alpha_inj"].min() >= ar.TINY, (name, K, dh)
        full = np.diff(c["indptr"].astype(np.int64)) > 0
        sums = ar.row_sums(c["indptr"], c["alpha"])
        assert np.abs(sums[full] - 1).max() <= 1e-13 and not sums[~full].any(), (name, K, dh)
        # the injected scalars are the exact ones rounded once: the two restatements differ by a rounding of the exponent
        assert ar.worst(c["alpha_inj"], c["alpha"], c["cp"])[0] <= ar.BAR / 8


def test_v2_restatement_is_gatv2_refs():
    """gat_alpha_ref.alpha_v2 without its two switches gives gatv2_ref.attention_v2's alpha, to the last bit of fp64"""
    for name, K, dh in ar.cases():
        c = ar.case_v2(name, K, dh)
        np.testing.assert_array_equal(c["restated"], c["alpha"])


def test_stress_cases_do_reach_the_absolute_rule():
    """the stress cases hold what the tolerance cases must not: entries below 2^-100 (v1 "ascending" and "late peak", v2), next
    to entries of order one"""
    for c in (ar.stress_v1("ascending", 4, 32), ar.stress_v1("late peak", 3, 7), ar.stress_v2(4, 32), ar.stress_v2(3, 7)):
        assert (c["alpha"] < ar.TINY).any() and (c["alpha"] > 0.1).any()
    assert ar.stress_v1("constant", 4, 32)["alpha"].min() >= ar.TINY


# ---- what the bar tells apart ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name,K,dh", [("long", 4, 32), ("longT", 3, 7), ("rect", 1, 260)])
def test_every_mutation_moves_some_entry_by_a_hundred_bars(variant, name, K, dh):
    """lse of the next row, no leaky slope, the score of the previous entry's source and -- v2 -- lrelu outside the dot
    product: each moves some entry by at least 100 bars on the measure"""
    case, mutations = VARIANTS[variant]
    c = case(name, K, dh)
    muts = mutations(c, K)
    assert len(muts) == (4 if variant == "v2" else 3)
    for what, alpha in muts.items():
        d, p = ar.worst(alpha, c["alpha"], c["cp"])
        print(f"[gat-alpha] {variant} {name} K={K} dh={dh} mutation '{what}': {d / ar.BAR:.3g} bars at entry {p[0]} head {p[1]}")
        assert d >= 100 * ar.BAR, (what, d)


# ---- refusals before the library ---------------------------------------------------------------------------------------------------------
class M:
    """a matrix that owns no device memory"""
    def __init__(self, n, m): self.N, self.Mm = n, m
    def n(self): return self.N
    def m(self): return self.Mm
    def shape(self): return (self.N, self.Mm)
    def buffer(self): raise AssertionError("the library must not be reached")


def _tiny(pkg):
    """8 x 8, 11 entries; its device() must not be reached either"""
    indptr = np.array([0, 2, 3, 3, 5, 6, 8, 10, 11], dtype=np.uint32)
    indices = np.array([1, 2, 0, 3, 4, 5, 6, 7, 0, 1, 2], dtype=np.uint32)
    F = pkg.csr_matrix(indptr, indices, np.ones(11, dtype=np.float32), 8)
    F.device = lambda *a: (_ for _ in ()).throw(AssertionError("the library must not be reached"))
    return F


def test_ops_refuse_bad_shapes_before_the_library(pkg):
    ops, F = pkg.ops, _tiny(pkg)
    for shape in ((10, 4), (11, 3), (8, 4)):                        # entries x heads is 11 x 4
        with pytest.raises(ValueError, match="alpha must be 11 x 4"):
            ops.gat_alpha(None, F, M(8, 4), M(8, 4), M(8, 4), M(*shape), 4)
        with pytest.raises(ValueError, match="alpha must be 11 x 4"):
            ops.gatv2_alpha(None, F, M(8, 64), M(8, 64), M(1, 32), M(8, 4), M(*shape), 4)
    with pytest.raises(ValueError, match="scores must be rows x heads"):
        ops.gat_alpha(None, F, M(8, 4), M(7, 4), M(8, 4), M(11, 4), 4)
    with pytest.raises(ValueError, match="lse must be rows x heads"):
        ops.gat_alpha(None, F, M(8, 4), M(8, 4), M(8, 3), M(11, 4), 4)
    with pytest.raises(ValueError, match="heads"):
        ops.gat_alpha(None, F, M(8, 17), M(8, 17), M(8, 17), M(11, 17), 17)
    with pytest.raises(ValueError, match="att must be 1 x"):
        ops.gatv2_alpha(None, F, M(8, 32), M(8, 32), M(2, 32), M(8, 4), M(11, 4), 4)
    with pytest.raises(ValueError, match="not divisible"):
        ops.gatv2_alpha(None, F, M(8, 30), M(8, 30), M(1, 30), M(8, 4), M(11, 4), 4)
    with pytest.raises(ValueError, match="shape mismatch"):
        ops.gatv2_alpha(None, F, M(9, 32), M(8, 32), M(1, 32), M(8, 4), M(11, 4), 4)
    with pytest.raises(ValueError, match="lse must be rows x heads"):
        ops.gatv2_alpha(None, F, M(8, 32), M(8, 32), M(1, 32), M(7, 4), M(11, 4), 4)
    with pytest.raises(ValueError, match="neither"):
        ops.gatv2_alpha(None, F, M(8, 48), M(8, 32), M(1, 32), M(8, 4), M(11, 4), 4)


class _layer:
    def __init__(self, F, H=None): self.F, self.H = F, H
    def alpha(self, ctx, out=None): raise AssertionError("the library must not be reached")


@pytest.mark.parametrize("module,cls", [("gat", "gat"), ("dist_gat", "dist_gat")])
def test_attention_weights_refuses_before_any_device_work(pkg, module, cls):
    """on a stand-in model without a device: a layer index out of range, an ``out`` of the wrong length or shape, and an
    export before any forward raise ValueError; no layer is asked for anything"""
    klass = getattr(import_module(pkg.__name__ + "." + module), cls)
    G = klass.__new__(klass)
    F = _tiny(pkg)
    G.layers_, G.heads = [_layer(F), _layer(F), _layer(F)], [4, 2, 1]
    for layers in ([3], [0, -1], [1, 7]):
        with pytest.raises(ValueError, match="out of range"):
            G.attention_weights(None, layers=layers)
    with pytest.raises(ValueError, match="out lists 2 matrices for 3 layers"):
        G.attention_weights(None, out=[M(11, 4), M(11, 2)])
    with pytest.raises(ValueError, match="out lists 1 matrices for 2 layers"):
        G.attention_weights(None, layers=[2, 0], out=[M(11, 1)])
    with pytest.raises(ValueError, match="out of layer 0 must be 11 x 4"):
        G.attention_weights(None, layers=[2, 0], out=[M(11, 1), M(11, 1)])
    with pytest.raises(ValueError, match="no forward has run"):
        G.attention_weights(None)
    with pytest.raises(ValueError, match="no forward has run"):
        G.attention_weights(None, layers=[1], out=[M(11, 2)])


def test_layer_alpha_refuses_before_any_forward(pkg):
    gat = import_module(pkg.__name__ + ".gat")
    L = gat.gat_layer.__new__(gat.gat_layer)
    L.name, L.H = "0_", None
    with pytest.raises(ValueError, match="no forward has run"):
        L.alpha(None)


def test_abi_lists_the_two_entry_points(pkg):
    protos = pkg._lib.PROTOTYPES
    assert len(protos["mggcn_gat_alpha_f32"][1]) == 12 and len(protos["mggcn_gatv2_alpha_f32"][1]) == 16
