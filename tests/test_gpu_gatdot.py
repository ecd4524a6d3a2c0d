"""The dot-product attention kernels (include/mggcn.h: mggcn_gatdot_*) and gat(variant="dot") on the device, against the fp64
restatement and the reference model of gatdot_ref.py.  Kernel level: the row-scaled measure of gat_ref.rowdist at the bars
gatdot_ref.BAR, fixed on the CPU (test_gatdot_cpu.py), on independently padded operands with guard words around every one of
them (guarded.py); model level: the sizes, heads, rules and bars of test_gpu_gatv2.py's model tests.  Everything that is
claimed bitwise is compared as bits."""
import numpy as np
import pytest

import bce_ref
import gat_ref as ref
import gatdot_ref as dot
from gat_ref import relerr, rowerr
from guarded import Guarded
from test_gpu_gat import N, TOL, _model_data, _u32
from test_gpu_gatv2 import MODELS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class _third:
    """one third of a guarded [rows x 3 d] device buffer"""

    def __init__(self, whole, d, third):
        self.whole, self.d, self.ld, self.third = whole, d, whole.ld, third

    @property
    def ptr(self):
        return self.whole.ptr + 4 * self.d * self.third

    def values(self):
        return self.whole.values()[:, self.third * self.d:(self.third + 1) * self.d].copy()


INPUTS = ("Zq", "Zk", "Zv", "G", "out_in", "lse_in", "D_in")
OUTPUTS = ("out", "lse", "D", "G_Zq", "G_Zk", "G_Zv")
OPERANDS = ("Zq", "Zk", "Zv", "G", "out", "G_Zq", "G_Zk", "G_Zv")      # the dense operands with a leading dimension


def _outputs(c, K, d, thirds, lay):
    n, n_src = c["n"], c["n_src"]
    m = dict(out=Guarded(n, d, d + lay("out")[1], lay("out")[0], output=True), lse=Guarded(n, K, K, output=True),
             D=Guarded(n, K, K, output=True))
    if thirds:
        m["G_Z3"] = Guarded(n, 3 * d, 3 * d, output=True)
        m.update(G_Zq=_third(m["G_Z3"], d, 0), G_Zk=_third(m["G_Z3"], d, 1), G_Zv=_third(m["G_Z3"], d, 2))
    else:
        m.update(G_Zq=Guarded(n, d, d + lay("G_Zq")[1], lay("G_Zq")[0], output=True),
                 G_Zk=Guarded(n_src, d, d + lay("G_Zk")[1], lay("G_Zk")[0], output=True),
                 G_Zv=Guarded(n_src, d, d + lay("G_Zv")[1], lay("G_Zv")[0], output=True))
    return m


def build(c, K, thirds=False, odd=()):
    """the operands of one case on the device, every one in a guarded buffer of its own (``thirds``: Zq | Zk | Zv and
    G_Zq | G_Zk | G_Zv as the thirds of one [n x 3 d] buffer each, square cases).  ``odd``: the operands of OPERANDS that
    sit one float off their 16-byte alignment with a leading dimension of d + 3.  backward_dst and backward_src read the
    restatement's out, lse and D (rounded to fp32) from buffers of their own, not what the forward wrote."""
    n, n_src, d = c["n"], c["n_src"], c["Zq"].shape[1]

    def lay(name):
        return (1, 3) if name in odd else (0, 0)
    m = dict(n=n, n_src=n_src, d=d, K=K, dh=d // K, thirds=thirds, lay=lay, ip=_u32(c["indptr"]), ix=_u32(c["indices"]))
    t_indptr, t_indices = ref.transpose_pattern(c["indptr"], c["indices"], n_src)
    m.update(tip=_u32(t_indptr), tix=_u32(t_indices))
    if thirds:
        assert n == n_src and not odd
        m["Z3"] = Guarded(n, 3 * d, 3 * d, logical=np.concatenate([c["Zq"], c["Zk"], c["Zv"]], axis=1))
        m.update(Zq=_third(m["Z3"], d, 0), Zk=_third(m["Z3"], d, 1), Zv=_third(m["Z3"], d, 2))
    else:
        m.update(Zq=Guarded(n, d, d + lay("Zq")[1], lay("Zq")[0], logical=c["Zq"]),
                 Zk=Guarded(n_src, d, d + lay("Zk")[1], lay("Zk")[0], logical=c["Zk"]),
                 Zv=Guarded(n_src, d, d + lay("Zv")[1], lay("Zv")[0], logical=c["Zv"]))
    m["backward"] = "G" in c
    if m["backward"]:
        w = c["want"]
        m.update(G=Guarded(n, d, d + lay("G")[1], lay("G")[0], logical=c["G"]),
                 out_in=Guarded(n, d, d + lay("out")[1], lay("out")[0], logical=w["out"].astype(np.float32)),
                 lse_in=Guarded(n, K, K, logical=w["lse"].astype(np.float32)),
                 D_in=Guarded(n, K, K, logical=w["D"].astype(np.float32)))
    m.update(_outputs(c, K, d, thirds, lay))
    return m


def fresh_outputs(c, m):
    """new NaN-filled output buffers in the layout of ``m``"""
    m.update(_outputs(c, m["K"], m["d"], m["thirds"], m["lay"]))


def launch(ctx, m, scale=None, rows=None, t_rows=None):
    """the three entry points once, through the C ABI with raw pointers; ``rows`` / ``t_rows`` = (r0, r1): the calls over
    F's rows / over F^T's rows take that row range only, as a call of its own (indptr + r0, the row operands moved by r0)"""
    import torch
    lib, st, K, dh = ctx.lib, ctx.stream(0), m["K"], m["dh"]
    scale = float(dot.default_scale(dh)) if scale is None else float(scale)
    torch.cuda.synchronize()                        # the operands are filled on torch's stream, the library runs on the context's
    r0, r1 = rows if rows is not None else (0, m["n"])
    t0, t1 = t_rows if t_rows is not None else (0, m["n_src"])

    def at(x, r):                                   # the address of row r
        return x.ptr + 4 * r * x.ld
    Zq, Zk, Zv = m["Zq"], m["Zk"], m["Zv"]
    lib.mggcn_gatdot_forward_f32(st, r1 - r0, m["n_src"], m["ip"].data_ptr() + 4 * r0, m["ix"].data_ptr(), at(Zq, r0), Zq.ld,
                                 Zk.ptr, Zk.ld, Zv.ptr, Zv.ld, K, dh, scale, at(m["out"], r0), m["out"].ld, at(m["lse"], r0))
    if m["backward"]:
        G, out_in, lse_in, D_in = m["G"], m["out_in"], m["lse_in"], m["D_in"]
        lib.mggcn_gatdot_backward_dst_f32(st, r1 - r0, m["n_src"], m["ip"].data_ptr() + 4 * r0, m["ix"].data_ptr(), at(Zq, r0),
                                          Zq.ld, Zk.ptr, Zk.ld, Zv.ptr, Zv.ld, at(lse_in, r0), at(G, r0), G.ld, at(out_in, r0),
                                          out_in.ld, K, dh, scale, at(m["D"], r0), at(m["G_Zq"], r0), m["G_Zq"].ld)
        lib.mggcn_gatdot_backward_src_f32(st, t1 - t0, m["n"], m["tip"].data_ptr() + 4 * t0, m["tix"].data_ptr(), Zq.ptr, Zq.ld,
                                          at(Zk, t0), Zk.ld, at(Zv, t0), Zv.ld, lse_in.ptr, D_in.ptr, G.ptr, G.ld, K, dh, scale,
                                          at(m["G_Zk"], t0), m["G_Zk"].ld, at(m["G_Zv"], t0), m["G_Zv"].ld)
    ctx.sync()


def results(m, what):
    """the outputs as numpy arrays, after the guard words around every output and every input were found intact"""
    names = OUTPUTS if m["backward"] else ("out", "lse")
    for k in (("out", "lse", "D", "G_Z3") if m["thirds"] else OUTPUTS):
        m[k].check_guards(f"{what} {k}")
    for k in ((("Z3",) if m["thirds"] else ("Zq", "Zk", "Zv")) + (("G", "out_in", "lse_in", "D_in") if m["backward"] else ())):
        m[k].check_unchanged(f"{what} {k}")
    return {k: m[k].values() for k in names}


def run_device(ctx, c, K, what="", scale=None, **kw):
    m = build(c, K, **kw)
    launch(ctx, m, scale)
    return results(m, what)


def _assert_case(what, c, got, names=dot.NAMES):
    for name in names:
        rt, dt = rowerr(c["twin"][name], c["want"][name], c["scale"][name]) if "twin" in c else (-1, 0.0)
        rg, dg = rowerr(got[name], c["want"][name], c["scale"][name])
        print(f"[gatdot] {what} {name}: twin {dt:.3e} (row {rt}) device {dg:.3e} (row {rg}) (bar {dot.BAR[name]:.0e})")
        assert dg <= dot.BAR[name], (what, name, rg, dg, "twin:", dt)


# ---- (1) every entry point against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K,dh", dot.cases())
def test_every_entry_point_against_the_restatement(ctx, name, K, dh):
    """out, lse, D, G_Zq, G_Zk and G_Zv within the bar on the long graph as F and transposed (so each kernel walks the long
    rows) at one (K, dh) per compiled variant plus the masked-tile cases, and on the 200 x 320 block; backward_dst and
    backward_src read the restatement's lse, D and out"""
    c = dot.case(name, K, dh)
    what = f"{name} K={K} dh={dh}"
    _assert_case(what, c, run_device(ctx, c, K, what))


# ---- (2) the model's layout -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,dh", [(4, 32), (3, 7), (1, 260)])
def test_thirds_of_one_buffer_give_the_bits_of_separate_buffers(ctx, K, dh):
    """Zq | Zk | Zv as the thirds of one [n x 3 out] buffer with ld = 3 out, and G_Zq | G_Zk | G_Zv as thirds of one buffer"""
    c = dot.case("long", K, dh)
    a, b = run_device(ctx, c, K, "separate"), run_device(ctx, c, K, "thirds", thirds=True)
    for name in dot.NAMES:
        np.testing.assert_array_equal(_bits(a[name]), _bits(b[name]), err_msg=name)
    _assert_case(f"thirds K={K} dh={dh}", c, b)


# ---- (3) misalignment ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", OPERANDS)
def test_misaligned_operands_take_the_element_path(ctx, which):
    """(4, 32) with one operand alone one float off 16-byte alignment at a leading dimension of d + 3: every kernel that
    touches it leaves the float4 path, stays within the bar of the restatement and leaves every guard word intact"""
    c = dot.case("long", 4, 32)
    _assert_case(f"misaligned {which}", c, run_device(ctx, c, 4, f"misaligned {which}", odd=(which,)))


def test_all_operands_misaligned_on_the_wide_shapes(ctx):
    """(1, 260) and (1, 1024) with every operand off alignment: the element path at 5 and 16 column tiles, (1,16,1)"""
    for K, dh in ((1, 260), (1, 1024)):
        c = dot.case("longT", K, dh)
        _assert_case(f"all misaligned K={K} dh={dh}", c, run_device(ctx, c, K, "all misaligned", odd=OPERANDS))


# ---- (4) empty and one-entry rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,dh", [(4, 32), (3, 7)])
def test_empty_rows_one_entry_rows_and_unreferenced_sources(ctx, K, dh):
    """rows without entries write lse = 0, out = +0.0 and G_Zq = +0.0 over the NaNs the buffers held, bit for bit; the
    one-entry row's out is its source's Zv row bit for bit; an unreferenced source gets G_Zk = G_Zv = +0.0"""
    c = dot.case("long", K, dh)
    indptr, indices = c["indptr"], c["indices"]
    got = run_device(ctx, c, K, "edge rows")
    for r in (0, 319):
        assert indptr[r] == indptr[r + 1]
        for name in ("out", "lse", "G_Zq"):
            np.testing.assert_array_equal(_bits(got[name][r]), np.zeros(got[name].shape[1], dtype=np.uint32), err_msg=name)
    assert indptr[2] - indptr[1] == 1
    np.testing.assert_array_equal(_bits(got["out"][1]), _bits(c["Zv"][indices[indptr[1]]]))
    for name in ("G_Zk", "G_Zv"):
        np.testing.assert_array_equal(_bits(got[name][ref.UNREFERENCED]), np.zeros(K * dh, dtype=np.uint32), err_msg=name)


# ---- (5) crafted probes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,dh", [(4, 32), (3, 7)])
def test_the_source_that_wins_by_40_at_every_chunk_edge(ctx, K, dh):
    """gatdot_ref.forward_probe_case: the source at position 0, 63, 64, 127, 128, L - 2 or L - 1 of each row scores 40, every
    other 0, all exactly.  out[row] is that source's Zv row and lse = 40, both within the bar"""
    for t in range(ref.PROBE_SLOTS):
        c = dot.forward_probe_case(t, K, dh)
        got = run_device(ctx, c, K, f"probe slot {t}", scale=dot.PROBE_SCALE)
        w = c["want"]
        hot = c["Zv"][c["hot"]]
        ro, do = rowerr(got["out"], w["out"], w["scale"]["out"])
        rh, dh_ = rowerr(got["out"], hot.astype(np.float64), w["scale"]["out"])
        rl, dl = rowerr(got["lse"], np.full((c["n"], K), 40.0), w["scale"]["lse"])
        print(f"[gatdot] probe K={K} dh={dh} slot {t} positions {c['pos']}: out {do:.3e}, from the hot row {dh_:.3e}, lse {dl:.3e}")
        assert do <= dot.BAR["out"] and dh_ <= dot.BAR["out"] and dl <= dot.BAR["lse"], (t, c["pos"], ro, rh, rl)


@pytest.mark.parametrize("K,dh", dot.STRESS_SHAPES)
def test_scores_in_the_hundreds_stay_finite(ctx, K, dh):
    """gatdot_ref.stress_case: integer queries and keys, c a power of two, every score exact and the largest |e| in
    [100, 256).  Every output is finite, lse is within the bar of the exact scores' lse, and the weights add up to one:
    |sum_j exp(e_ijk - lse[i, k]) - 1| <= the bar with the exact scores and the DEVICE's lse"""
    c = dot.stress_case(K, dh)
    e = c["want"]["e"]
    assert 100 <= np.abs(e).max() < 256, (c["a"], np.abs(e).max())
    got = run_device(ctx, c, K, "stress")
    for name in dot.NAMES:
        assert np.isfinite(got[name]).all(), name
    rl, dl = rowerr(got["lse"], c["want"]["lse"], c["scale"]["lse"])
    sums = dot.alpha_row_sums(c["indptr"], e, got["lse"])
    print(f"[gatdot] stress K={K} dh={dh} a={c['a']}: max |e| {np.abs(e).max():.2f}, lse {dl:.3e} (row {rl}), "
          f"|sum alpha - 1| <= {np.abs(sums - 1).max():.2e}")
    assert dl <= dot.BAR["lse"]
    assert np.abs(sums - 1).max() <= dot.BAR["lse"]
    # out and D too, as test_gpu_gatv2.py's stress test holds them; not the three gradients: every source of the probe block
    # has one entry, and where its weight is below fp32's smallest normal (e^-200 here) the format, not the kernel, decides
    # what is left of that single term (gat_ref.stress_case has the same remark)
    _assert_case(f"stress K={K} dh={dh}", c, got, names=("out", "lse", "D"))


def test_two_destinations_prefer_different_sources(ctx):
    """gatdot_ref.dynamic_probe() on the device: out[i, :2] are destination i's two coefficients"""
    indptr, indices, Zq, Zk, Zv = dot.dynamic_probe()
    c = dict(indptr=indptr, indices=indices, n=2, n_src=2, Zq=Zq, Zk=Zk, Zv=Zv)
    got = run_device(ctx, c, 1, "dynamic probe")
    want = dot.restate64(indptr, indices, Zq, Zk, Zv, 1, exact=True, scales=True)
    assert rowerr(got["out"], want["out"], want["scale"]["out"])[1] <= dot.BAR["out"]
    assert rowerr(got["lse"], want["lse"], want["scale"]["lse"])[1] <= dot.BAR["lse"]
    assert got["out"][0, 0] > 0.5 > got["out"][1, 0] and got["out"][1, 1] > 0.5 > got["out"][0, 1], got["out"]


# ---- (6) reproducibility and row splits ----------------------------------------------------------------------------------------------------
BITS_CASES = [("long", 4, 32, ()), ("longT", 4, 32, ()), ("long", 3, 7, ()), ("longT", 1, 260, ()), ("long", 1, 257, ()),
              ("rect", 2, 65, ()), ("long", 4, 32, OPERANDS)]


@pytest.mark.parametrize("name,K,dh,odd", BITS_CASES)
def test_two_calls_and_every_row_split_give_the_same_bits(ctx, name, K, dh, odd):
    """a second call gives the first call's bits, and so do a call over rows [0, r) and one over [r, n) (offset pointers)
    for r = 1, 4, 7 and n - 1, for all three kernels (backward_src splits the rows of F^T)"""
    c = dot.case(name, K, dh)
    m = build(c, K, odd=odd)
    launch(ctx, m)
    whole = results(m, "whole")
    launch(ctx, m)
    again = results(m, "again")
    for nm in dot.NAMES:
        np.testing.assert_array_equal(_bits(whole[nm]), _bits(again[nm]), err_msg=nm)
    n, n_src = c["n"], c["n_src"]
    for r, rt in ((1, 1), (4, 4), (7, 7), (n - 1, n_src - 1)):
        fresh_outputs(c, m)
        launch(ctx, m, rows=(0, r), t_rows=(0, rt))
        launch(ctx, m, rows=(r, n), t_rows=(rt, n_src))
        split = results(m, f"split at {r}")
        for nm in dot.NAMES:
            np.testing.assert_array_equal(_bits(whole[nm]), _bits(split[nm]), err_msg=f"{nm} split at {r} / {rt}")


def test_no_rows_launches_nothing_and_writes_nothing(ctx):
    c = dot.case("long", 4, 32)
    m = build(c, 4)
    launch(ctx, m, rows=(0, 0), t_rows=(0, 0))
    for k in OUTPUTS:
        m[k].check_guards(f"no rows {k}")
        np.testing.assert_array_equal(m[k].bits(), m[k].init, err_msg=k)          # the logical elements too


# ---- (7) the model -----------------------------------------------------------------------------------------------------------------------------
def _gat(pkg, csr, sizes, heads, **kw):
    ip, ix, dv = csr
    return pkg.gat(pkg.csr_matrix(ip.copy(), ix.copy(), dv.copy(), N), sizes, heads=heads, variant="dot", **kw)


def _oracle(oracle, csr, sizes, heads, **kw):
    ip, ix, dv = csr
    per_layer = [heads] * (len(sizes) - 2) + [1]
    return dot.oracle_gatdot(oracle, oracle.Csr(ip.copy(), ix.copy(), dv.copy(), N), sizes, per_layer, **kw)


def _sync_oracle_state(G, O):
    """identical inputs for the next epoch: the reference takes over the device's parameters and Adam moments"""
    for layer, ol in zip(G.layers(), O.layers):
        ol.lin.W, ol.lin.b = layer.W().numpy().copy(), layer.b().numpy().copy()
        if layer.lin.mW is not None:
            ol.lin.mW, ol.lin.vW = layer.lin.mW.numpy().copy(), layer.lin.vW.numpy().copy()
            ol.lin.mb, ol.lin.vb = layer.lin.mb.numpy().copy(), layer.lin.vb.numpy().copy()
            ol.lin.step = layer.lin.step


def _grads(G):
    return [(l.GW().numpy().copy(), l.Gb().numpy().copy()) for l in G.layers()]


def _assert_grads(what, mine, theirs):
    for li, (g, o) in enumerate(zip(mine, theirs)):
        for name, a, b in zip(("G_W", "G_b"), g, o):
            d = relerr(a, b)
            print(f"[gatdot] {what} layer {li} {name}: {d:.3e}")
            assert d <= TOL, (what, li, name, d)


def _state_bits(G):
    out = []
    for l in G.layers():
        assert l.params() == [l.lin] and l.attn.adam_tensors(5e-4) == []
        for t in (l.W(), l.b(), l.GW(), l.Gb(), l.lin.mW, l.lin.vW, l.lin.mb, l.lin.vb):
            out.append(t.numpy().view(np.uint32).copy())
    return out


def _epochs_against_the_reference(pkg, oracle, ctx, G, O, sizes, X, Y, what):
    for layer, ol in zip(G.layers(), O.layers):                     # same seed-99 init, bit for bit
        np.testing.assert_array_equal(layer.W().numpy(), ol.lin.W)
        np.testing.assert_array_equal(layer.b().numpy(), ol.lin.b)
        assert layer.W().shape() == (ol.lin.W.shape[0], 3 * ol.out_width) and layer.att() is None
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    lr = 1e-2
    for epoch in range(3):
        _sync_oracle_state(G, O)
        loss, acc = G.train_forward(ctx, Xd, Yd)
        G.backward(ctx)
        ctx.sync()
        grads = _grads(G)
        G.adam_update(ctx, lr, 0.9, 0.999, 5e-4, 1e-8)
        ctx.sync()
        ol, oa = O.train_forward(X, Y)
        O.backward()
        ograds = [(l.lin.G_W.copy(), l.lin.G_b.copy()) for l in O.layers]
        O.adam_update()
        print(f"[gatdot] {what} epoch {epoch}: loss {loss!r} (reference {ol!r}), acc {acc!r} ({oa!r})")
        assert np.isfinite(ol), "the reference overflowed: the input is outside its range"
        assert abs(loss - ol) <= TOL * abs(ol), (epoch, loss, ol)
        assert abs(acc - oa) <= 3.0 / N, (epoch, acc, oa)
        _assert_grads(f"{what} epoch {epoch}", grads, ograds)
        for li, (layer, olayer) in enumerate(zip(G.layers(), O.layers)):
            P, Po, g = layer.W().numpy(), olayer.lin.W, ograds[li][0]
            assert np.abs(P - Po).max() <= 2.05 * lr, (epoch, li)                   # never more than a sign flip
            solid = np.abs(g) > 1e-2 * np.abs(g).max()                              # well-conditioned entries
            assert np.abs(P - Po)[solid].max() <= TOL * np.abs(Po).max(), (epoch, li)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("sizes,heads", MODELS)
def test_gatdot_epochs_match_the_reference(pkg, oracle, ctx, fused, sizes, heads):
    """three full epochs (forward, loss, backward, Adam) against the reference model on identical inputs, by the rules of
    test_gpu_gatv2.test_gatv2_epochs_match_the_reference"""
    csr, X, Y = _model_data(pkg, sizes)
    G = _gat(pkg, csr, sizes, heads, fused=fused)
    O = _oracle(oracle, csr, sizes, heads)
    _epochs_against_the_reference(pkg, oracle, ctx, G, O, sizes, X, Y, f"sizes={sizes} fused={fused}")


def test_gatdot_dropout_epochs_match_the_reference(pkg, oracle, ctx):
    """dropout=0.5 against the reference model with the numpy mask, from epoch 4 of seed 0xC0FFEE123"""
    sizes, heads = MODELS[0]
    csr, X, Y = _model_data(pkg, sizes)
    G = _gat(pkg, csr, sizes, heads, dropout=0.5)
    G.set_dropout(0.5, seed=0xC0FFEE123, epoch=4)
    O = _oracle(oracle, csr, sizes, heads, p=0.5, seed=0xC0FFEE123, epoch=4)
    _epochs_against_the_reference(pkg, oracle, ctx, G, O, sizes, X, Y, f"sizes={sizes} dropout=0.5")
    assert G.dropout_epoch == 7 and G.attn_dropout_p == 0.0


def _run_epochs(pkg, ctx, sizes, heads, fused, step, epochs=3, **kw):
    csr, X, Y = _model_data(pkg, sizes)
    G = _gat(pkg, csr, sizes, heads, fused=fused, **kw)
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    res = []
    for _ in range(epochs):
        if step:
            res.append(G.train_step(ctx, Xd, Yd, 1e-2, 0.9, 0.999, 5e-4, 1e-8))
        else:
            res.append(G.train_forward(ctx, Xd, Yd))
            G.backward(ctx)
            G.adam_update(ctx, 1e-2, 0.9, 0.999, 5e-4, 1e-8)
            ctx.sync()
    return res, _state_bits(G)


@pytest.mark.parametrize("sizes,heads", MODELS)
def test_fused_adam_per_tensor_adam_and_train_step_give_the_same_bits(pkg, ctx, sizes, heads):
    base = _run_epochs(pkg, ctx, sizes, heads, fused=False, step=False)
    for fused, step in ((True, False), (True, True), (False, True)):
        res, bits = _run_epochs(pkg, ctx, sizes, heads, fused=fused, step=step)
        assert res == base[0], (fused, step)
        for a, b in zip(bits, base[1]):
            np.testing.assert_array_equal(a, b)
    assert base[0][-1][0] < base[0][0][0], base[0]                 # and it trains


def test_bce_with_splits_matches_the_reference(pkg, oracle, ctx):
    """loss="bce" with set_splits: one epoch against the reference model with the fp32 restatement of the multi-label loss
    over the training rows"""
    sizes, heads = MODELS[1]
    csr, X, _ = _model_data(pkg, sizes)
    T = (np.random.default_rng(3).random((N, sizes[-1])) < 0.2).astype(np.int32)
    S = np.random.default_rng(4).choice(4, size=N, p=(0.5, 0.2, 0.25, 0.05)).astype(np.int32)
    train = S == 0
    n_train = int(train.sum())
    G = _gat(pkg, csr, sizes, heads, loss="bce")
    G.set_splits(S)

    def loss(H):
        Gr = np.ascontiguousarray(bce_ref.grad32(H, T, 1.0 / (float(n_train) * H.shape[1])))
        Gr[~train] = 0
        return Gr, (float(bce_ref.loss32(H, T).astype(np.float64)[train].sum() / (n_train * H.shape[1])),
                    bce_ref.micro_f1(*bce_ref.counts(H[train], T[train])[0]))
    O = _oracle(oracle, csr, sizes, heads, loss=loss)
    got = G.train_forward(ctx, pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(T))
    assert got == G.split_metrics()["train"] and G.split_metrics()["counts"]["train"] == n_train
    G.backward(ctx)
    ctx.sync()
    want = O.train_forward(X, None)
    O.backward()
    print(f"[gatdot] bce with splits: (loss, micro-F1) {got!r} (reference {want!r})")
    assert abs(got[0] - want[0]) <= TOL * abs(want[0])
    assert got[1] == want[1] or abs(got[1] - want[1]) <= 3.0 / n_train
    _assert_grads("bce with splits", _grads(G), [(l.lin.G_W, l.lin.G_b) for l in O.layers])


def test_evaluate_and_predict_agree_with_a_plain_forward(pkg, ctx):
    sizes, heads = MODELS[1]
    csr, X, Y = _model_data(pkg, sizes)
    S = np.random.default_rng(4).choice(3, size=N).astype(np.int32)
    G = _gat(pkg, csr, sizes, heads, dropout=0.5)
    Xd, Yd, Sd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y), pkg.dn_matrix.from_numpy(S.reshape(-1, 1))
    res = G.evaluate(ctx, Xd, Yd, Sd)
    out = G(ctx, Xd)
    ctx.sync()
    best = out.numpy().argmax(axis=1)
    hit = best == Y.reshape(-1)
    assert res["all"] == float(hit.mean()) and G.dropout_epoch == 0       # neither drops
    for k, name in enumerate(("train", "val", "test")):
        assert res[name] == float(hit[S == k].mean())
    np.testing.assert_array_equal(G.predict(ctx, Xd).reshape(-1), best)


def test_set_dropout_replays_an_epoch(pkg, ctx):
    sizes, heads = MODELS[0]
    csr, X, Y = _model_data(pkg, sizes)
    G = _gat(pkg, csr, sizes, heads, dropout=0.5)
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)

    def epoch():
        res = G.train_forward(ctx, Xd, Yd)
        G.backward(ctx)
        ctx.sync()
        return res, [_bits(t) for g in _grads(G) for t in g]
    G.set_dropout(0.5, seed=11, epoch=2)
    first = epoch()
    assert G.dropout_epoch == 3
    second = epoch()
    assert second[0] != first[0] and any((a != b).any() for a, b in zip(first[1], second[1]))
    G.set_dropout(0.5, seed=11, epoch=2)
    again = epoch()
    assert again[0] == first[0]
    for a, b in zip(first[1], again[1]):
        np.testing.assert_array_equal(a, b)
    with pytest.raises(ValueError, match="attention dropout"):
        G.set_dropout(0.5, seed=11, epoch=9, attn=0.1)
    assert G.attn_dropout_p == 0.0 and G.dropout_epoch == 3             # a refused call stores nothing


def test_selector_restores_the_best_epoch(pkg, ctx, tmp_path):
    """model_selector on a dot model: restore() brings back the parameters the best epoch ended with, bit for bit, and resets
    Adam; save_best, save and load are refused and create nothing"""
    sizes, heads = MODELS[0]
    csr, X, Y = _model_data(pkg, sizes)
    S = np.random.default_rng(5).choice(3, size=N, p=(0.6, 0.2, 0.2)).astype(np.int32)
    G = _gat(pkg, csr, sizes, heads)
    G.set_splits(S)
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    sel = pkg.model_selector(G, metric="loss", clean=True)
    ended = []
    for _ in range(6):
        sel.step(ctx, Xd, Yd, 5e-2, 0.9, 0.999, 5e-4, 1e-8)
        ctx.sync()
        ended.append([t.numpy().view(np.uint32).copy() for l in G.layers() for t in (l.W(), l.b())])
    assert sel.best_epoch == int(np.argmin(sel.history)) and len(sel.history) == 6
    sel.restore(ctx)
    for a, b in zip([t.numpy().view(np.uint32) for l in G.layers() for t in (l.W(), l.b())], ended[sel.best_epoch]):
        np.testing.assert_array_equal(a, b)
    for l in G.layers():
        assert l.lin.step == 0 and not l.lin.mW.numpy().any() and not l.lin.vb.numpy().any()
    for refused in (lambda: sel.save_best(ctx, str(tmp_path / "best")), lambda: G.save(ctx, str(tmp_path / "model")),
                    lambda: G.load(ctx, str(tmp_path / "model")), lambda: G.attention_weights(ctx, Xd),
                    lambda: G.layers()[0].alpha(ctx)):
        with pytest.raises(ValueError, match="dot"):
            refused()
    assert not list(tmp_path.iterdir())


def test_the_other_variants_keep_their_bits_next_to_a_dot_model(pkg):
    """a "v1" and a "v2" model built next to a "dot" model in the same process give the bits of a second build of each, and
    a dot model registers its two sparse timers per layer and none of the others' attention timers"""
    from test_gpu_gatv2 import _run_epochs as run_other
    sizes, heads = MODELS[0]
    ctx = pkg.context(0)
    before = {v: run_other(pkg, ctx, sizes, heads, fused=True, step=True, variant=v) for v in ("v1", "v2")}
    ctx2 = pkg.context(0)
    d = _run_epochs(pkg, ctx2, sizes, heads, fused=True, step=True)
    mine = sorted(t for t in ctx2.timers if "gat" in t)
    assert mine == sorted(f"{li}_{s}" for li in range(3) for s in ("0_gatdot-forward", "1_gatdot-backward-dst",
                                                                  "1_gatdot-backward-src")), mine
    for v in ("v1", "v2"):
        after = run_other(pkg, ctx, sizes, heads, fused=True, step=True, variant=v)
        assert after[0] == before[v][0] and after[0] != d[0], v
        for x, y in zip(after[1], before[v][1]):
            np.testing.assert_array_equal(x, y)
    assert not [t for t in ctx.timers if "gatdot" in t], sorted(ctx.timers)
