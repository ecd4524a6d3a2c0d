"""The export of the attention coefficients on the device: mggcn_gat_alpha_f32 / mggcn_gatv2_alpha_f32 through the C ABI with
raw pointers, gat.attention_weights / attention_pattern, and dist_gat's on two ranks.  The measure, its bar (fixed on the CPU,
test_gat_alpha_cpu.py) and the cases are gat_alpha_ref's; everything that is claimed bitwise is compared as bits."""
import multiprocessing as mp
import os
import queue
import signal
import sys
import time
import traceback

import numpy as np
import pytest

import gat_alpha_ref as ar
import gat_ref as ref
import gatv2_ref as v2
from gat_ref import ROW_TOL, rowerr
from test_gpu_dist_bf16 import _free_port, _init
from test_gpu_gat import _dense, _u32

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 123.0


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _sync():
    import torch
    torch.cuda.synchronize()            # the operands are filled on torch's stream, the library runs on the context's


class _alpha(_dense):
    """the [nnz x K] output at leading dimension K + pad, ``offset`` floats off a 16-byte aligned allocation, pre-filled with
    123.0; whole() is every float of the allocation's [nnz x ld] block, guards() the floats around it"""

    def whole(self):
        o = int((self.ptr - self.flat.data_ptr()) // 4)
        return self.flat[o:o + self.rows * self.ld].view(self.rows, self.ld).cpu().numpy()

    def guards(self):
        o = int((self.ptr - self.flat.data_ptr()) // 4)
        return np.concatenate([self.flat[:o].cpu().numpy(), self.flat[o + self.rows * self.ld:].cpu().numpy()])


# ---- the two variants behind one interface: operands(ctx, c, K, dh, inject) and export(ctx, m, alpha, rows) -------------------------
class V1:
    name, case, stress_slope = "v1", staticmethod(ar.case_v1), ref.SLOPE

    @staticmethod
    def operands(ctx, c, K, dh, inject):
        """the device state an export reads: the reference's fp32 s_dst, s_src, lse (``inject``), or what the device's own
        gat_scores + gat_forward leave behind (then m["out"] and m["Z"] are there too)"""
        lib, st = ctx.lib, ctx.stream(0)
        n, n_src = c["indptr"].size - 1, c["n_src"]
        m = dict(n=n, n_src=n_src, K=K, dh=dh, ip=_u32(c["indptr"]), ix=_u32(c["indices"]))
        if inject:
            m.update(s_dst=_dense(n, K, host=c["s_dst32"]), s_src=_dense(n_src, K, host=c["s_src32"]), lse=_dense(n, K, host=c["lse32"]))
            _sync()
            return m
        d = K * dh
        Zs, at = _dense(n_src, d, host=c["Z"]), _dense(2, d, host=c["att"])
        m.update(Z=Zs, s_dst=_dense(n, K), s_src=_dense(n_src, K), lse=_dense(n, K), out=_dense(n, d))
        _sync()
        if c.get("Z_dst") is None:
            lib.mggcn_gat_scores_f32(st, Zs.ptr, Zs.ld, at.ptr, m["s_dst"].ptr, m["s_src"].ptr, n_src, K, dh)
        else:
            Zd = _dense(n, d, host=c["Z_dst"])
            _sync()
            lib.mggcn_gat_scores_f32(st, Zd.ptr, Zd.ld, at.ptr, m["s_dst"].ptr, None, n, K, dh)
            lib.mggcn_gat_scores_f32(st, Zs.ptr, Zs.ld, at.ptr, None, m["s_src"].ptr, n_src, K, dh)
        lib.mggcn_gat_forward_f32(st, n, n_src, m["ip"].data_ptr(), m["ix"].data_ptr(), Zs.ptr, Zs.ld, m["s_dst"].ptr,
                                  m["s_src"].ptr, K, dh, ref.SLOPE, m["out"].ptr, m["out"].ld, m["lse"].ptr)
        ctx.sync()
        return m

    @staticmethod
    def export(ctx, m, alpha, rows=None, slope=ref.SLOPE):
        r0, r1 = rows if rows is not None else (0, m["n"])
        K = m["K"]
        ctx.lib.mggcn_gat_alpha_f32(ctx.stream(0), r1 - r0, m["n_src"], m["ip"].data_ptr() + 4 * r0, m["ix"].data_ptr(),
                                    m["s_dst"].ptr + 4 * r0 * K, m["s_src"].ptr, m["lse"].ptr + 4 * r0 * K, K, slope,
                                    alpha.ptr, alpha.ld)
        ctx.sync()


class V2:
    name, case, stress_slope = "v2", staticmethod(ar.case_v2), v2.STRESS_SLOPE

    @staticmethod
    def operands(ctx, c, K, dh, inject, slope=ref.SLOPE):
        lib, st = ctx.lib, ctx.stream(0)
        n, n_src, d = c["indptr"].size - 1, c["n_src"], K * dh
        Zs, Zd, at = _dense(n_src, d, host=c["Zs"]), _dense(n, d, host=c["Zd"]), _dense(1, d, host=c["att"])
        m = dict(n=n, n_src=n_src, K=K, dh=dh, ip=_u32(c["indptr"]), ix=_u32(c["indices"]), Zs=Zs, Z=Zs, Zd=Zd, att=at)
        if inject:
            m["lse"] = _dense(n, K, host=c["lse32"])
            _sync()
            return m
        m.update(lse=_dense(n, K), out=_dense(n, d))
        _sync()
        lib.mggcn_gatv2_forward_f32(st, n, n_src, m["ip"].data_ptr(), m["ix"].data_ptr(), Zs.ptr, Zs.ld, Zd.ptr, Zd.ld, at.ptr, K,
                                    dh, slope, m["out"].ptr, m["out"].ld, m["lse"].ptr)
        ctx.sync()
        return m

    @staticmethod
    def export(ctx, m, alpha, rows=None, slope=ref.SLOPE):
        r0, r1 = rows if rows is not None else (0, m["n"])
        K, Zd = m["K"], m["Zd"]
        ctx.lib.mggcn_gatv2_alpha_f32(ctx.stream(0), r1 - r0, m["n_src"], m["ip"].data_ptr() + 4 * r0, m["ix"].data_ptr(),
                                      m["Zs"].ptr, m["Zs"].ld, Zd.ptr + 4 * r0 * Zd.ld, Zd.ld, m["att"].ptr,
                                      m["lse"].ptr + 4 * r0 * K, K, m["dh"], slope, alpha.ptr, alpha.ld)
        ctx.sync()


VARIANTS = [V1, V2]
IDS = [v.name for v in VARIANTS]


def _export(ctx, V, m, nnz, **kw):
    alpha = _alpha(nnz, m["K"])
    _sync()
    V.export(ctx, m, alpha, **kw)
    return alpha.numpy()


def _assert_alpha(what, got, want, cp, indptr):
    """the bar per entry, and per non-empty row |sum_j alpha - 1| <= bar max_p c_p, in fp64"""
    d, p, _ = ar.check(got, want, cp)
    sums = ar.row_sums(indptr, got)
    full = np.diff(indptr.astype(np.int64)) > 0
    off = float(np.abs(sums[full] - 1).max())
    print(f"[gat-alpha] {what}: worst {d:.3e} at entry {p[0]} head {p[1]} (bar {ar.BAR:.1e}); |sum - 1| <= {off:.3e} "
          f"(allowed {ar.BAR * cp.max():.3e})")
    assert np.isfinite(got).all()
    assert d <= ar.BAR, (what, p, d)
    assert off <= ar.BAR * cp.max(), (what, off)


# ---- (1) the kernel contract ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K,dh", ar.cases())
@pytest.mark.parametrize("V", VARIANTS, ids=IDS)
def test_alpha_against_the_restatement(ctx, V, name, K, dh):
    """the device's alpha against the fp64 restatement at the bar: (a) with the reference's fp32 scalars (v1: s_dst, s_src, lse;
    v2: lse) injected on both sides, (b) after the device's own scores and forward; every non-empty row sums to 1"""
    c = V.case(name, K, dh)
    nnz = c["indices"].size
    assert c["alpha"].min() >= ar.TINY
    got = _export(ctx, V, V.operands(ctx, c, K, dh, True), nnz)
    _assert_alpha(f"{V.name} {name} K={K} dh={dh} injected", got, c["alpha_inj"], c["cp_inj"], c["indptr"])
    got = _export(ctx, V, V.operands(ctx, c, K, dh, False), nnz)
    _assert_alpha(f"{V.name} {name} K={K} dh={dh} own forward", got, c["alpha"], c["cp"], c["indptr"])


# ---- (2) placement ---------------------------------------------------------------------------------------------------------------------
def _duplicates(name, c):
    """the two entry numbers of the duplicated (row, column) pair of gat_ref.kernel_graph_long, as F or transposed"""
    ip, ix = ref.kernel_graph_long()
    b = int(ip[ref.LONG_DUPLICATE_ROW])
    if name == "long":
        return b, b + 1
    row = int(ix[b])                                    # transposed: the row of that column lists row 13 twice
    beg, end = int(c["indptr"][row]), int(c["indptr"][row + 1])
    hits = beg + np.nonzero(c["indices"][beg:end] == ref.LONG_DUPLICATE_ROW)[0]
    assert hits.size == 2
    return int(hits[0]), int(hits[1])


@pytest.mark.parametrize("offset,pad", [(1, 3), (0, 4)], ids=["misaligned", "aligned"])
@pytest.mark.parametrize("name,K,dh", [("long", 4, 32), ("longT", 4, 32), ("long", 3, 7), ("longT", 3, 7)])
@pytest.mark.parametrize("V", VARIANTS, ids=IDS)
def test_placement(ctx, V, name, K, dh, offset, pad):
    """the raw entry point on a buffer pre-filled with 123.0, lda = K + 3 and one float off alignment (and lda = K + 4 on an
    aligned base, where v1 stores 16 bytes at K = 4): columns [K, lda) and the floats around the block keep 123.0, every
    entry is written, a call over rows [5, 13) writes those rows' entries with the whole call's bits and nothing else, and the
    two entries of the duplicated (row, column) pair are equal"""
    c = V.case(name, K, dh)
    indptr, nnz = c["indptr"].astype(np.int64), c["indices"].size
    m = V.operands(ctx, c, K, dh, False)
    whole, part = _alpha(nnz, K, offset, pad), _alpha(nnz, K, offset, pad)
    _sync()
    V.export(ctx, m, whole)
    V.export(ctx, m, part, rows=(5, 13))
    _sync()
    for a in (whole, part):
        assert (a.whole()[:, K:] == FILL).all() and (a.guards() == FILL).all()
    w, p = whole.numpy(), part.numpy()
    assert (w != FILL).all() and (w > 0).all() and (w <= 1.0 + 1e-6).all()
    _assert_alpha(f"{V.name} {name} K={K} dh={dh} lda={K + pad} offset={offset}", w, c["alpha"], c["cp"], c["indptr"])
    lo, hi = int(indptr[5]), int(indptr[13])
    assert hi - lo > 64
    np.testing.assert_array_equal(_bits(p[lo:hi]), _bits(w[lo:hi]))
    assert (p[:lo] == FILL).all() and (p[hi:] == FILL).all()
    a, b = _duplicates(name, c)
    np.testing.assert_array_equal(_bits(w[a]), _bits(w[b]))
    # the aligned and the misaligned buffer hold the same bits: where a value lands is no part of it
    np.testing.assert_array_equal(_bits(w), _bits(_export(ctx, V, m, nnz)))


@pytest.mark.parametrize("V", VARIANTS, ids=IDS)
def test_no_rows_writes_nothing_and_checks_no_operand(ctx, V):
    lib, st = ctx.lib, ctx.stream(0)
    if V is V1:
        lib.mggcn_gat_alpha_f32(st, 0, 320, None, None, None, None, None, 4, ref.SLOPE, None, 4)
    else:
        lib.mggcn_gatv2_alpha_f32(st, 0, 320, None, None, None, 128, None, 128, None, None, 4, 32, ref.SLOPE, None, 4)
    ctx.sync()


# ---- (3) reproducibility ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K,dh", [("long", 4, 32), ("longT", 3, 7), ("long", 1, 260), ("rect", 2, 65)])
@pytest.mark.parametrize("V", VARIANTS, ids=IDS)
def test_two_calls_give_the_same_bits(ctx, V, name, K, dh):
    c = V.case(name, K, dh)
    m = V.operands(ctx, c, K, dh, False)
    a, b = _export(ctx, V, m, c["indices"].size), _export(ctx, V, m, c["indices"].size)
    np.testing.assert_array_equal(_bits(a), _bits(b))


# ---- (4) the tie to the fused kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,dh", [(4, 32), (3, 7)])
@pytest.mark.parametrize("V", VARIANTS, ids=IDS)
def test_spmm_with_the_exported_values_reproduces_the_forward(pkg, ctx, V, K, dh):
    """per head k, csr_matrix(indptr, indices, alpha[:, k]) times Z[:, head k] through ops.matmul is the forward kernel's
    out[:, head k], row by row on the reference's scale of ``out`` at ROW_TOL"""
    c = V.case("long", K, dh)
    m = V.operands(ctx, c, K, dh, False)
    alpha = _export(ctx, V, m, c["indices"].size)
    out, Z = m["out"].numpy(), m["Z"].numpy()
    n, n_src = m["n"], m["n_src"]
    scale = c["scale"]["out"]
    for k in range(K):
        A = pkg.csr_matrix(c["indptr"].copy(), c["indices"].copy(), np.ascontiguousarray(alpha[:, k]), n_src)
        B, C = pkg.dn_matrix.from_numpy(np.ascontiguousarray(Z[:, k * dh:(k + 1) * dh])), pkg.dn_matrix(n, dh)
        pkg.ops.matmul(ctx, A, B, C, pkg.ops.get_matmul_buffer(ctx, A, B, C), 1.0, 0.0)
        ctx.sync()
        row, d = rowerr(C.numpy(), out[:, k * dh:(k + 1) * dh], scale[:, k * dh:(k + 1) * dh])
        print(f"[gat-alpha] {V.name} K={K} dh={dh} head {k}: SpMM(alpha) against the forward's out {d:.3e} at row {row}")
        assert d <= ROW_TOL, (k, row, d)


# ---- (5) stress --------------------------------------------------------------------------------------------------------------------------
def _assert_stress(what, got, c):
    d, p, small = ar.check(got, c["alpha"], c["cp"])
    n_small = int((c["alpha"] < ar.TINY).sum())
    print(f"[gat-alpha] stress {what}: worst {d:.3e} at entry {p[0]} head {p[1]} (bar {ar.BAR:.1e}); {n_small} of {c['alpha'].size} "
          f"entries below 2^-100, the device's largest there {small:.3e}")
    assert np.isfinite(got).all() and (got >= 0).all()
    assert d <= ar.BAR, (what, p, d)
    assert small <= ar.TINY_GOT, (what, small)


@pytest.mark.parametrize("kind", ref.STRESS_KINDS)
@pytest.mark.parametrize("K,dh", [(4, 32), (3, 7)])
def test_stress_v1(ctx, K, dh, kind):
    """gat_ref.stress_case (scores of -80 .. +80 along rows of 64 .. 4097 entries) with the reference's fp32 lse on both sides:
    entries whose exact alpha is below 2^-100 come out at most 2^-99, every other within the bar"""
    c = ar.stress_v1(kind, K, dh)
    _assert_stress(f"v1 {kind} K={K} dh={dh}", _export(ctx, V1, V1.operands(ctx, c, K, dh, True), c["indices"].size), c)


@pytest.mark.parametrize("K,dh", [(4, 32), (3, 7)])
def test_stress_v2(ctx, K, dh):
    """gatv2_ref.stress_case (exact scores in the hundreds, slope 0.25), likewise"""
    c = ar.stress_v2(K, dh)
    got = _export(ctx, V2, V2.operands(ctx, c, K, dh, True), c["indices"].size, slope=v2.STRESS_SLOPE)
    _assert_stress(f"v2 K={K} dh={dh}", got, c)


# ---- (6) the model -----------------------------------------------------------------------------------------------------------------------
MN, SIZES, HEADS = 320, [16, 32, 32, 5], [4, 2, 1]


def _model_graph():
    """A such that the forward matrix A.transpose() is kernel_graph_long's pattern with sorted rows (0 .. 4097 entries)"""
    ip, ix, _ = ref.edge_graphs()["longT"]
    return ip.copy(), ix.copy(), np.ones(ix.size, dtype=np.float32)


def _model_X():
    return np.random.default_rng(7).standard_normal((MN, SIZES[0]), dtype=np.float32)


def _reference(oracle, variant):
    cls = v2.oracle_gatv2 if variant == "v2" else ref.oracle_gat
    return cls(oracle, oracle.Csr(*_model_graph(), MN), SIZES, HEADS, dtype=np.float64)


def _weights(O):
    return [(L.lin.W.copy(), L.lin.b.copy(), L.att.copy()) for L in O.layers]


def _gat(pkg, weights, variant, **kw):
    return pkg.gat(pkg.csr_matrix(*_model_graph(), MN), SIZES, heads=HEADS, weights=weights, variant=variant, **kw)


@pytest.mark.parametrize("variant", ["v1", "v2"])
def test_attention_weights_against_the_reference_model(pkg, oracle, ctx, variant):
    """attention_weights(ctx, X) of a three-layer model with heads 4, 2, 1 against the reference model composed layer by layer
    from the same weights, at the bar; layers=[2, 0] returns those two in that order (and into ``out`` when given);
    attention_pattern() is A.transpose()'s arrays; ValueError before any forward"""
    O = _reference(oracle, variant)
    G = _gat(pkg, _weights(O), variant)
    with pytest.raises(ValueError, match="no forward has run"):
        G.attention_weights(ctx)
    with pytest.raises(ValueError, match="no forward has run"):
        G.layers()[1].alpha(ctx)
    X = _model_X()
    got = G.attention_weights(ctx, pkg.dn_matrix.from_numpy(X))
    ctx.sync()
    indptr, indices = G.attention_pattern()
    F = G.A.transpose()
    np.testing.assert_array_equal(indptr, F.indptr)
    np.testing.assert_array_equal(indices, F.indices)
    np.testing.assert_array_equal(indptr, O.indptr)
    np.testing.assert_array_equal(indices, O.indices)
    want = ar.model_alphas(O, X, variant)
    assert len(got) == 3
    for li, (g, (alpha, cp)) in enumerate(zip(got, want)):
        assert g.shape() == (indices.size, HEADS[li]) and alpha.min() >= ar.TINY
        _assert_alpha(f"{variant} model layer {li}", g.numpy(), alpha, cp, indptr)
    two = G.attention_weights(ctx, layers=[2, 0])
    into = [pkg.dn_matrix(indices.size, 1), pkg.dn_matrix(indices.size, 4)]
    back = G.attention_weights(ctx, layers=[2, 0], out=into)
    ctx.sync()
    assert len(two) == 2 and back[0] is into[0] and back[1] is into[1]
    for a, b, li in zip(two, into, (2, 0)):
        np.testing.assert_array_equal(_bits(a.numpy()), _bits(got[li].numpy()))
        np.testing.assert_array_equal(_bits(b.numpy()), _bits(got[li].numpy()))
    with pytest.raises(ValueError, match="out of range"):
        G.attention_weights(ctx, layers=[3])
    with pytest.raises(ValueError, match="out of layer 2 must be"):
        G.attention_weights(ctx, layers=[2], out=[into[1]])


def test_export_after_attention_dropout_is_the_plain_forwards(pkg, oracle, ctx):
    """attention_weights(ctx) after train_step with attn_dropout = 0.5 against the export after a plain forward of a second
    model built from the same weights.  Layer 0, whose input nothing drops, must match bit for bit.  The layers above cannot:
    their input is the dropped layer's output, which the plain model never sees -- so there the claim is checked on the
    layer's own state: a PLAIN scores + forward + export of the Z the training forward left in the layer, with the weights
    the step started from, gives the training state's export bit for bit.  Either way the state is the normalised
    coefficient before the dropout factor: every row sums to one and nothing carries 1 / (1 - p)."""
    ops, dn = pkg.ops, pkg.dn_matrix
    W = _weights(_reference(oracle, "v1"))
    X = _model_X()
    Y = np.random.default_rng(8).integers(0, SIZES[-1], size=(MN, 1)).astype(np.int32)
    Xd, Yd = dn.from_numpy(X), dn.from_numpy(Y)
    A, B = _gat(pkg, W, "v1", attn_dropout=0.5), _gat(pkg, W, "v1")
    A.set_dropout(0.0, seed=5, epoch=1, attn=0.5)
    A.train_step(ctx, Xd, Yd, *ref.ADAM)
    a = A.attention_weights(ctx)                        # the state of the training forward (Adam has moved the weights since)
    b = B.attention_weights(ctx, Xd)
    ctx.sync()
    np.testing.assert_array_equal(_bits(a[0].numpy()), _bits(b[0].numpy()))
    assert not np.array_equal(_bits(a[1].numpy()), _bits(b[1].numpy()))         # the dropout was real: layer 1 saw another input
    indptr, indices = A.attention_pattern()
    full = np.diff(indptr.astype(np.int64)) > 0
    for li, layer in enumerate(A.layers()):
        K, d = HEADS[li], SIZES[li + 1]
        att = dn.from_numpy(np.asarray(W[li][2], dtype=np.float32).reshape(2, d))
        s_dst, s_src, lse, out, alpha = dn(MN, K), dn(MN, K), dn(MN, K), dn(MN, d), dn(indices.size, K)
        ops.gat_scores(ctx, layer.Z, att, s_dst, s_src, K)
        ops.gat_forward(ctx, layer.F, layer.Z, s_dst, s_src, out, lse, K)
        ops.gat_alpha(ctx, layer.F, s_dst, s_src, lse, alpha, K)
        ctx.sync()
        np.testing.assert_array_equal(_bits(alpha.numpy()), _bits(a[li].numpy()), err_msg=f"layer {li}")
        assert np.abs(ar.row_sums(indptr, a[li].numpy())[full] - 1).max() <= ROW_TOL       # the bound test_gpu_gat_edges.py holds this sum to


# ---- (7) dist_gat on two ranks -----------------------------------------------------------------------------------------------------------
CHILD_LIMIT = 150           # seconds a rank may live; the parent gives up with the first rank that fails


def _pkg():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as ge
    return ge.load_package()


def _rank_worker(rank, P, port, weights, X, q):
    """a rank's export (after attention_weights(dctx, X), and again from the state) and its pattern"""
    signal.alarm(CHILD_LIMIT)                           # the rank's own time limit
    dist = _init(rank, P, port)
    try:
        pkg = _pkg()
        D = pkg.dist
        dctx = D.dist_context(overlap=True, device_index=0)
        A = pkg.csr_matrix(*_model_graph(), MN)
        A_T = A.transpose()
        p = D.partition_bounds(MN, P)
        G = D.dist_gat(dctx, D.dist_row_csr_matrix(dctx, A, p, p, keep_rows=True), D.dist_row_csr_matrix(dctx, A_T, p, p), SIZES,
                       heads=HEADS, weights=weights)
        refused = False
        try:
            G.attention_weights(dctx)
        except ValueError:
            refused = True
        first = G.attention_weights(dctx, D.dist_row_dn_matrix(dctx, X))
        again = G.attention_weights(dctx, layers=[2, 0])
        dctx.sync()
        first, again = [a.numpy().copy() for a in first], [a.numpy().copy() for a in again]
        ip, ix = G.attention_pattern()
        q.put((rank, dict(first=first, again=again, indptr=ip.copy(), indices=ix.copy(), refused=refused, bounds=list(p)), None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def _spawn(target, P, args):
    """P fresh children (P <= 3: never more than four processes with the parent), each under its own time limit; the parent
    stops at the first child that reports an error or dies, and ends the others"""
    assert P <= 3
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = _free_port()
    procs = [mpc.Process(target=target, args=(r, P, port) + tuple(args) + (q,)) for r in range(P)]
    for pr in procs:
        pr.start()
    res, deadline = {}, time.monotonic() + CHILD_LIMIT + 30
    try:
        while len(res) < P:
            try:
                r = q.get(timeout=0.25)
            except queue.Empty:
                dead = [(i, pr.exitcode) for i, pr in enumerate(procs) if pr.exitcode not in (None, 0)]
                assert not dead, f"rank(s) died: {dead}"
                assert time.monotonic() < deadline, "the ranks did not report in time"
                continue
            assert r[-1] is None, f"rank {r[0]} failed:\n{r[-1]}"
            res[r[0]] = r[1]
        for pr in procs:
            pr.join(timeout=60)
            assert pr.exitcode == 0
    finally:
        for pr in procs:
            if pr.is_alive():
                pr.terminate()
                pr.join(timeout=30)
    return [res[r] for r in range(P)]


def test_dist_gat_exports_the_single_gpu_rows_bit_for_bit(pkg, oracle, ctx):
    """two ranks sharing the GPU: rank r's export is rows [p_r, p_{r+1}) of the single-GPU gat's export from the same weights,
    bit for bit, in every layer; its pattern is those rows of the single-GPU pattern with global columns; an export from the
    state (layers=[2, 0]) repeats the bits; no forward yet is refused on every rank"""
    W = _weights(_reference(oracle, "v1"))
    X = _model_X()
    G = _gat(pkg, W, "v1")
    single = G.attention_weights(ctx, pkg.dn_matrix.from_numpy(X))
    ctx.sync()
    single = [a.numpy() for a in single]
    indptr, indices = G.attention_pattern()
    ip = indptr.astype(np.int64)
    res = _spawn(_rank_worker, 2, (W, X))
    covered = 0
    for rank, r in enumerate(res):
        assert r["refused"]
        lo, hi = r["bounds"][rank], r["bounds"][rank + 1]
        e0, e1 = int(ip[lo]), int(ip[hi])
        np.testing.assert_array_equal(r["indptr"].astype(np.int64), ip[lo:hi + 1] - ip[lo])
        np.testing.assert_array_equal(r["indices"], indices[e0:e1])
        for li in range(3):
            assert r["first"][li].shape == (e1 - e0, HEADS[li])
            np.testing.assert_array_equal(_bits(r["first"][li]), _bits(single[li][e0:e1]), err_msg=f"rank {rank} layer {li}")
        for a, li in zip(r["again"], (2, 0)):
            np.testing.assert_array_equal(_bits(a), _bits(single[li][e0:e1]), err_msg=f"rank {rank} layer {li} from the state")
        covered += e1 - e0
    assert covered == indices.size and e1 - e0 > 0
