"""Every attention entry point (include/mggcn.h: mggcn_gat_*, the _drop twins, mggcn_gatv2_*, the packed-record forms and the
two alpha exports) on independently padded, guarded operands: gat_layout_ref.py has the 37 x 53 graph, the layout table and
the guard-sizing rule, guarded.py the buffers.  Per (family, shape, layout) the whole chain runs once on ctx.stream(0);
inputs carry IN_NAN32 outside the logical matrix, outputs start as OUT_NAN32 everywhere.  After one synchronisation:
(a) nothing outside an output's logical window changed, (b) every input buffer is as uploaded, (c) every logical output
element was written, (d) and is finite, (e) every output meets the fp64 restatement of its family row by row at that
family's bar, (f) a call that takes the variant it takes on contiguous operands -- and reads from such calls only -- gives
the contiguous run's bits, and the record forms give the plain forms' bits in every layout.  A kernel that mixes up two
leading dimensions reads guard NaNs or overwrites guard words; the guards are sized so that it cannot leave the allocation."""
import time

import numpy as np
import pytest

import gat_alpha_ref as ar
import gat_layout_ref as lr
import gat_ref as ref
from gat_ref import rowerr
from guarded import OUT_NAN32, Guarded

pytestmark = pytest.mark.gpu

EMPTY_ROW = 34
RANGE = (5, 34)
_t0 = time.perf_counter()


@pytest.fixture(scope="module")
def ctx(pkg):
    yield pkg.context(0)
    print(f"[gat-layouts] wall time of this file: {time.perf_counter() - _t0:.1f} s")


def _torch():
    import torch
    return torch


_graph = {}


def _device_graph(c):
    """device addresses of indptr, indices and the transposed pattern, uploaded once"""
    if not _graph:
        torch = _torch()
        for k in ("indptr", "indices", "t_indptr", "t_indices"):
            _graph[k] = torch.from_numpy(np.ascontiguousarray(c[k], dtype=np.uint32).view(np.int32)).cuda()
    return tuple(_graph[k].data_ptr() for k in ("indptr", "indices", "t_indptr", "t_indices"))


class _Half:
    """one half of a wider guarded buffer as an operand: its address, the buffer's leading dimension, its logical bits"""

    def __init__(self, whole, col0, rows, cols):
        self.whole, self.col0, self.rows, self.cols, self.ld, self.ptr = whole, col0, rows, cols, whole.ld, whole.ptr + 4 * col0

    def logical_bits(self):
        return self.whole.logical_bits()[:self.rows, self.col0:self.col0 + self.cols].copy()


def _operands(b, p):
    return {name: (b[name] if q.view is None else _Half(b[q.view[0]], q.view[1], q.rows, q.cols)) for name, q in p.items()}


def _launch(ctx, family, c, o, K, dh, rows=None, t_rows=None, only=None):
    """the chain of one family in the order of the existing run_device helpers, the pack_dst + _rec form of backward_src next
    to the plain one and the alpha export last; ``rows`` / ``t_rows`` = (r0, r1): the calls over F's / F^T's rows take that
    range as a call of their own (indptr + r0, the row operands moved by r0 rows); ``only``: these calls alone"""
    L, st, slope = ctx.lib, ctx.stream(0), ref.SLOPE
    n, n_src, d = c["n"], c["n_src"], K * dh
    ip, ix, tip, tix = _device_graph(c)
    r0, r1 = rows or (0, n)
    t0, t1 = t_rows or (0, n_src)

    def at(name, r=0):
        return o[name].ptr + 4 * r * o[name].ld

    def ld(name):
        return o[name].ld

    def on(call):
        return only is None or call in only
    if family == "gatv2":
        if on("forward"):
            L.mggcn_gatv2_forward_f32(st, r1 - r0, n_src, ip + 4 * r0, ix, at("Zs"), ld("Zs"), at("Zd", r0), ld("Zd"), at("att"), K,
                                      dh, slope, at("out", r0), ld("out"), at("lse", r0))
        if on("backward_dst"):
            L.mggcn_gatv2_backward_dst_f32(st, r1 - r0, n_src, ip + 4 * r0, ix, at("Zs"), ld("Zs"), at("Zd", r0), ld("Zd"), at("att"),
                                           at("lse", r0), at("G", r0), ld("G"), at("out", r0), ld("out"), K, dh, slope, at("D", r0),
                                           at("G_Zd", r0), ld("G_Zd"), at("P", r0), ld("P"))
        if on("att_grad"):
            L.mggcn_gatv2_att_grad_f32(st, at("P"), ld("P"), n, d, at("G_att"))
        if on("backward_src"):
            L.mggcn_gatv2_backward_src_f32(st, t1 - t0, n, tip + 4 * t0, tix, at("Zs", t0), ld("Zs"), at("Zd"), ld("Zd"), at("att"),
                                           at("lse"), at("D"), at("G"), ld("G"), K, dh, slope, at("G_Zs", t0), ld("G_Zs"))
        if on("pack_dst"):
            L.mggcn_gatv2_pack_dst_f32(st, at("lse"), at("D"), n, K, at("rec"))
        if on("backward_src_rec"):
            L.mggcn_gatv2_backward_src_rec_f32(st, t1 - t0, n, tip + 4 * t0, tix, at("Zs", t0), ld("Zs"), at("Zd"), ld("Zd"),
                                               at("att"), at("rec"), at("G"), ld("G"), K, dh, slope, at("G_Zs_r", t0), ld("G_Zs_r"))
        if on("alpha"):
            L.mggcn_gatv2_alpha_f32(st, n, n_src, ip, ix, at("Zs"), ld("Zs"), at("Zd"), ld("Zd"), at("att"), at("lse"), K, dh, slope,
                                    at("alpha"), ld("alpha"))
        return
    drop = family == "gat-drop"
    sfx = "_drop_f32" if drop else "_f32"
    th, scale, seed, stream = c["drop"][:4] if drop else (0, 1.0, 0, 0)
    fwd_drop = (th, scale, seed, stream, r0, 0) if drop else ()            # the rows of F are destinations: dst0 = r0
    src_drop = (th, scale, seed, stream, 0, t0) if drop else ()            # the rows of F^T are sources: src0 = t0
    if on("scores"):
        L.mggcn_gat_scores_f32(st, at("Zd"), ld("Zd"), at("att"), at("s_dst"), None, n, K, dh)
        L.mggcn_gat_scores_f32(st, at("Zs"), ld("Zs"), at("att"), None, at("s_src"), n_src, K, dh)
    if on("forward"):
        getattr(L, "mggcn_gat_forward" + sfx)(st, r1 - r0, n_src, ip + 4 * r0, ix, at("Zs"), ld("Zs"), at("s_dst", r0), at("s_src"),
                                              K, dh, slope, at("out", r0), ld("out"), at("lse", r0), *fwd_drop)
    if on("backward_dst"):
        getattr(L, "mggcn_gat_backward_dst" + sfx)(st, r1 - r0, n_src, ip + 4 * r0, ix, at("Zs"), ld("Zs"), at("s_dst", r0),
                                                   at("s_src"), at("lse", r0), at("G", r0), ld("G"), at("out", r0), ld("out"), K, dh,
                                                   slope, at("D", r0), at("ds_dst", r0), *fwd_drop)
    # a rectangular block: the destinations live elsewhere, so backward_src gets no ds_dst
    if on("backward_src"):
        getattr(L, "mggcn_gat_backward_src" + sfx)(st, t1 - t0, n, tip + 4 * t0, tix, at("Zs", t0), ld("Zs"), at("s_dst"),
                                                   at("s_src", t0), at("lse"), at("D"), at("G"), ld("G"), at("att"), None, K, dh,
                                                   slope, at("ds_src", t0), at("G_Zs", t0), ld("G_Zs"), *src_drop)
    if on("pack_dst"):
        L.mggcn_gat_pack_dst_f32(st, at("s_dst"), at("lse"), at("D"), n, K, at("rec"))
    if on("backward_src_rec"):
        getattr(L, "mggcn_gat_backward_src_rec" + sfx)(st, t1 - t0, n, tip + 4 * t0, tix, at("Zs", t0), ld("Zs"), at("rec"),
                                                       at("s_src", t0), at("G"), ld("G"), at("att"), None, K, dh, slope,
                                                       at("ds_src_r", t0), at("G_Zs_r", t0), ld("G_Zs_r"), *src_drop)
    if on("scores_backward"):
        L.mggcn_gat_scores_backward_f32(st, at("ds_dst"), at("Zd"), ld("Zd"), n, at("ds_src"), at("Zs"), ld("Zs"), n_src, K, dh,
                                        at("G_att"))
    if on("alpha"):
        L.mggcn_gat_alpha_f32(st, n, n_src, ip, ix, at("s_dst"), at("s_src"), at("lse"), K, slope, at("alpha"), ld("alpha"))


def _buffers(family, K, dh, layout):
    c = lr.case(family, K, dh)
    p = lr.plan(family, K, dh, layout, c["nnz"])
    values = lr.input_values(family, c)
    if layout == "halves":
        values["Z2"] = lr.halves_values(c, K, dh)
    b = lr.make_buffers(p, values)
    if layout == "halves":                  # the G_Zd half has no rows beyond the destinations: nobody writes there
        g = b["G_Z2"]
        g._window(g.mask)[c["n"]:, K * dh:] = False
    return c, p, b


def run_chain(ctx, family, K, dh, layout):
    """(case, plan, buffers, operand -> logical bits) after the whole chain and one synchronisation"""
    c, p, b = _buffers(family, K, dh, layout)
    o = _operands(b, p)
    _torch().cuda.synchronize()             # the buffers are filled on torch's stream, the library runs on the context's
    _launch(ctx, family, c, o, K, dh)
    ctx.sync()
    bits = {name: o[name].logical_bits() for name, q in p.items() if q.output and name != "G_Z2"}
    return c, p, b, bits


_contiguous = {}


def _baseline(ctx, family, K, dh):
    if (family, K, dh) not in _contiguous:
        _contiguous[(family, K, dh)] = run_chain(ctx, family, K, dh, "contiguous")[3]
    return _contiguous[(family, K, dh)]


def _f32(bits):
    return bits.view(np.float32)


def _check(ctx, family, K, dh, layout):
    c, p, b, bits = run_chain(ctx, family, K, dh, layout)
    what = f"{family} K={K} dh={dh} {layout}"
    # (a)-(d)
    found = lr.violations(b, p)
    assert not found, (what, [v[2] for v in found])
    # rows without entries: +0.0 in out (and G_Zd, P), lse = 0; alpha has a position for every entry and for nothing else
    assert c["indptr"][EMPTY_ROW] == c["indptr"][EMPTY_ROW + 1]
    for name in ("out", "lse") + (("G_Zd", "P") if family == "gatv2" else ()):
        assert not bits[name][EMPTY_ROW].any(), (what, name)
    assert bits["alpha"].shape == (c["nnz"], K)
    # (e) against the restatement, row by row
    for name in lr.compared(family):
        rn = lr.result_name(family, name)
        row, dist = rowerr(_f32(bits[name]), c["want"][rn], c["scale"][rn])
        print(f"[gat-layouts] {what} {name}: {dist:.3e} at row {row} (bar {c['bar'][rn]:.1e})")
        assert dist <= c["bar"][rn], (what, name, row, dist)
    dist, where, _ = ar.check(_f32(bits["alpha"]), c["alpha"], c["cp"])
    print(f"[gat-layouts] {what} alpha: {dist:.3e} at entry {where[0]} head {where[1]} (bar {ar.BAR:.1e})")
    assert c["alpha"].min() >= ar.TINY and dist <= ar.BAR, (what, where, dist)
    # the record and its forms: the plain forms' bits in every layout
    n = c["n"]
    if family == "gatv2":
        rec = np.stack([bits["lse"], bits["D"]], axis=2).reshape(n, 2 * K)
    else:
        rec = np.stack([bits["s_dst"], bits["lse"], bits["D"], np.zeros_like(bits["D"])], axis=2).reshape(n, 4 * K)
        np.testing.assert_array_equal(bits["ds_src_r"], bits["ds_src"], err_msg=what)
    np.testing.assert_array_equal(bits["rec"], rec, err_msg=what)
    np.testing.assert_array_equal(bits["G_Zs_r"], bits["G_Zs"], err_msg=what)
    # (f) bits against the contiguous run
    base = _baseline(ctx, family, K, dh)
    same = lr.same_bits_as_contiguous(family, K, dh, p, lr.plan(family, K, dh, "contiguous", c["nnz"]))
    for call, (_, _, _, outputs, _) in lr.CALLS[family].items():
        if same[call]:
            for name in outputs:
                np.testing.assert_array_equal(bits[name], base[name], err_msg=f"{what}: {call} -> {name}")
    return same


CASES = [(f, K, dh, layout) for f in lr.FAMILIES for K, dh in lr.SHAPES[f] for layout in lr.layouts_for(f, K, dh)]


@pytest.mark.parametrize("family,K,dh,layout", CASES)
def test_chain_on_independently_padded_guarded_operands(ctx, family, K, dh, layout):
    """checks (a)-(f) of the module's docstring for one (family, shape, layout)"""
    same = _check(ctx, family, K, dh, layout)
    if dh % 4 != 0 or layout not in ("odd-ld", "off-base"):
        assert all(same.values()), same                 # float4 stays float4, and an element shape is one in every layout


@pytest.mark.parametrize("K,dh", [(4, 32), (3, 7)])
def test_halves_of_one_buffer_with_unequal_partners(ctx, K, dh):
    """GATv2's model layout: Zs | Zd and G_Zs | G_Zd are the halves of [rows x 2 K dh] buffers, and G, out and P each have
    another padded leading dimension; (a)-(f), the bits of the contiguous run included"""
    same = _check(ctx, "gatv2", K, dh, "halves")
    assert all(same.values()), same


# one float4 and one element shape per family
@pytest.mark.parametrize("family,K,dh", [(f, K, dh) for f in lr.FAMILIES for K, dh in ((4, 32), (3, 7))])
def test_a_row_range_leaves_the_rows_around_it_alone(ctx, family, K, dh):
    """forward, backward_dst and backward_src on rows [5, 34) of F (of F^T for backward_src) as calls of their own on padded
    guarded buffers that start as OUT_NAN32: the rows before and behind the range -- those the last, partly filled workgroup
    could reach included -- still hold OUT_NAN32, and the rows inside carry the whole call's bits"""
    r0, r1 = RANGE
    c, p, b, whole = run_chain(ctx, family, K, dh, "vec-padded")
    v2 = family == "gatv2"
    ranged = ("out", "lse", "D") + (("G_Zd", "P") if v2 else ("ds_dst",)) + ("G_Zs",) + (() if v2 else ("ds_src",))
    fresh = {}
    for name in ranged:
        q = p[name]
        fresh[name] = Guarded(q.rows, q.cols, q.ld, q.off, output=True, tail_rows=q.tail_rows)
        g = fresh[name]
        g._window(g.mask)[:r0] = False                  # the logical window is the range alone
        g._window(g.mask)[r1:] = False
    o = _operands(b, p)
    _torch().cuda.synchronize()
    # F's rows: forward and backward_dst write the range of the fresh out, lse, D, ...; backward_src reads lse and D of
    # EVERY destination (its entries), so it runs on the whole call's and writes the range of the fresh G_Zs (and ds_src)
    first = dict(o, **{k: v for k, v in fresh.items() if k not in ("G_Zs", "ds_src")})
    _launch(ctx, family, c, first, K, dh, rows=RANGE, only=("forward", "backward_dst"))
    second = dict(o, **{k: fresh[k] for k in ("G_Zs", "ds_src") if k in fresh})
    _launch(ctx, family, c, second, K, dh, t_rows=RANGE, only=("backward_src",))
    ctx.sync()
    found = lr.violations(fresh, p) + lr.violations({k: v for k, v in b.items() if not p[k].output}, p)
    assert not found, [v[2] for v in found]
    for name, g in fresh.items():
        got = g.logical_bits()
        assert (got[:r0] == OUT_NAN32).all() and (got[r1:] == OUT_NAN32).all(), name
        np.testing.assert_array_equal(got[r0:r1], whole[name][r0:r1], err_msg=name)
