"""The GAT kernels over a plan that cuts long rows (include/mggcn.h: mggcn_gat_*_split_f32; csrc/gat_split.hip) and
gat(row_split=S) on the device.  The graph is gat_ref.kernel_graph_long(): rows of 0 .. 4097 entries on both sides of the
96-entry threshold of split = 64 -- as F ("long"), where forward and backward_dst walk the long rows, and as F^T ("longT"),
where backward_src does.  The bar is
test_gpu_gat.py's: TOL = 1e-4 on the matrix-normalised distance from the fp64 restatement, the fp32 twin within a third of it
first.  Everything that is claimed bitwise is compared as bits."""
import numpy as np
import pytest

import gat_ref as ref
from gat_ref import relerr

pytestmark = pytest.mark.gpu

TOL = 1e-4
VARIANT_SHAPES = [(4, 32), (1, 260), (3, 7), (1, 130), (1, 257)]        # one (K, dh) per (VEC, NT, U)
OUTPUTS = ("out", "lse", "D", "ds_dst", "ds_src", "G_Z")
_graphs = {}


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


def _graph(pkg, name):
    """(F, F^T) as csr_matrix and the host pattern, once per module: a plan is kept on its matrix"""
    if name not in _graphs:
        indptr, indices, n_src = ref.probe_block() if name == "probe" else ref.kernel_graph_long() + (320,)
        if name == "longT":
            indptr, indices = ref.transpose_pattern(indptr, indices, n_src)
        t_indptr, t_indices = ref.transpose_pattern(indptr, indices, n_src)
        ones = lambda ix: np.ones(ix.size, dtype=np.float32)
        _graphs[name] = (pkg.csr_matrix(indptr, indices, ones(indices), n_src),
                         pkg.csr_matrix(t_indptr, t_indices, ones(t_indices), indptr.size - 1), indptr, indices)
    return _graphs[name]


def _run(pkg, ctx, name, Z, G, att, K, split=None, drop=None, scores=None, feed=None):
    """forward, backward_dst and backward_src over the plans of ``split`` (None: the plain calls); ``scores`` = (s_dst, s_src)
    in place of the scores kernel's; ``feed``: the forward's outputs the two backward calls read, in place of this run's"""
    ops, dn = pkg.ops, pkg.dn_matrix.from_numpy
    F, FT, _, _ = _graph(pkg, name)
    n, n_src, d = F.n(), F.m(), Z.shape[1]
    new = lambda rows, cols: dn(np.full((rows, cols), 123.0, dtype=np.float32))
    Zd, Gd, at = dn(Z), dn(G), dn(att)
    r = dict(out=new(n, d), G_Z=new(n_src, d), ds_src=new(n_src, K), **{k: new(n, K) for k in ("lse", "D", "ds_dst")})
    if scores is None:
        s_dst, s_src = new(n, K), new(n_src, K)
        ops.gat_scores(ctx, Zd, at, s_dst, s_src, K)
    else:
        s_dst, s_src = dn(scores[0]), dn(scores[1])
    kw = {} if drop is None else dict(drop=drop)
    plans = ((), ()) if split is None else tuple((ops.gat_split_plan(ctx, M, split, K, d),) for M in (F, FT))
    sfx = "" if split is None else "_split"
    getattr(ops, "gat_forward" + sfx)(ctx, F, Zd, s_dst, s_src, r["out"], r["lse"], K, *plans[0], **kw)
    fed = r if feed is None else {k: dn(v) for k, v in feed.items()}
    getattr(ops, "gat_backward_dst" + sfx)(ctx, F, Zd, s_dst, s_src, fed["lse"], Gd, fed["out"], r["D"], r["ds_dst"], K, *plans[0],
                                           **kw)
    fed = r if feed is None else fed
    getattr(ops, "gat_backward_src" + sfx)(ctx, FT, Zd, s_dst, s_src, fed["lse"], fed["D"], Gd, at,
                                           fed["ds_dst"] if n == n_src else None, r["ds_src"], r["G_Z"], K, *plans[1], **kw)
    ctx.sync()
    return {k: v.numpy() for k, v in r.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _parity(got, want, twin, what, names=OUTPUTS):
    for name in names:
        dg = relerr(got[name], want[name])
        dt = 0.0 if twin is None else relerr(twin[name], want[name])        # no twin: crafted scores, exact in fp32
        print(f"[gat split] {what} {name}: twin {dt:.3e} device {dg:.3e} (bar {TOL:.0e})")
        assert dt <= TOL / 3, ("the input is ill-conditioned for this bar", what, name, dt)
        assert dg <= TOL, (what, name, dg, "twin:", dt)


@pytest.mark.parametrize("K,dh", VARIANT_SHAPES)
@pytest.mark.parametrize("split", [64, 1024])
@pytest.mark.parametrize("graph", ["long", "longT"])
def test_every_output_against_the_restatement(pkg, ctx, graph, split, K, dh):
    """(1) split = 64: 129 -> 3 x 43, 128 and 192 -> slices of one chunk, 4097 -> 65 slices; split = 1024: 4097 -> 5 slices of
    about thirteen chunks"""
    _, _, indptr, indices = _graph(pkg, graph)
    Z, _, G, att = ref.tolerance_inputs(320, 320, K, dh)
    got = _run(pkg, ctx, graph, Z, G, att, K, split)
    _parity(got, ref.restate64(indptr, indices, Z, att, K, G=G), ref.twin32(indptr, indices, Z, att, K, G=G),
            f"{graph} split={split} K={K} dh={dh}")


@pytest.mark.parametrize("K,dh", [(4, 32), (3, 7)])
@pytest.mark.parametrize("graph", ["long", "longT"])
def test_unsplit_rows_have_the_plain_bits(pkg, ctx, graph, K, dh):
    """(2) on the same operands, every row the plan of split = 64 leaves whole (96 entries at the most) is the plain call's
    bit for bit, and so is every output at split = 8192, where nothing is cut"""
    F, FT, _, _ = _graph(pkg, graph)
    Z, _, G, att = ref.tolerance_inputs(320, 320, K, dh)
    plain = _run(pkg, ctx, graph, Z, G, att, K)
    feed = {k: plain[k] for k in ("out", "lse", "D", "ds_dst")}
    whole = {k: np.diff(M.indptr.astype(np.int64)) <= 96 for k, M in (("F", F), ("FT", FT))}
    cut = whole["FT" if graph == "longT" else "F"]
    assert 0 < (~cut).sum() < 20 and cut.sum() > 300             # the calls that walk the long side have rows of both kinds
    for split, rows in ((64, whole), (8192, {"F": slice(None), "FT": slice(None)})):
        got = _run(pkg, ctx, graph, Z, G, att, K, split, feed=feed)
        for name in OUTPUTS:
            keep = rows["FT" if name in ("ds_src", "G_Z") else "F"]
            np.testing.assert_array_equal(_bits(got[name][keep]), _bits(plain[name][keep]), err_msg=f"{name} split={split}")


@pytest.mark.parametrize("kind", ref.STRESS_KINDS)
def test_rescaling_between_slices(pkg, ctx, kind):
    """(3) gat_ref.stress_scores x 25 on its probe block (rows of 64 .. 4097 entries): scores of -2000 .. 2000, so a slice's
    exp(m_s - M) underflows to 0.  Every output finite, the coefficients of every row add up to 1, and parity at TOL of what
    the rescaling produces: out, lse and D = G . out.  The other three are finite and no more: with every weight on entries of
    positive score ds_dst is D - D, exactly 0 in fp64 and rounding noise in any fp32, so no matrix-normalised bar applies to
    it or to what is formed from it, and the backward kernels read lse and rescale nothing."""
    K, dh = 4, 32
    _, _, indptr, indices = _graph(pkg, "probe")
    n, n_src = indptr.size - 1, indices.size
    rng = np.random.default_rng(31)
    Z, G = (rng.standard_normal((r, K * dh), dtype=np.float32) for r in (n_src, n))
    att = (0.1 * rng.standard_normal((2, K * dh))).astype(np.float32)
    s_dst, s_src = np.zeros((n, K), dtype=np.float32), (25.0 * ref.stress_scores(kind, K)).astype(np.float32)
    got = _run(pkg, ctx, "probe", Z, G, att, K, 64, scores=(s_dst, s_src))
    assert all(np.isfinite(got[name]).all() for name in OUTPUTS)
    sums = ref.alpha_row_sums(indptr, indices, s_src, got["lse"])
    print(f"[gat split] {kind}: row sums of alpha within {np.abs(sums - 1).max():.3e} of 1")
    assert np.abs(sums - 1).max() <= TOL
    want = ref.restate64(indptr, indices, Z, att, K, G=G, Z_dst=np.zeros((n, K * dh), dtype=np.float32), s_dst=s_dst, s_src=s_src)
    _parity(got, want, None, kind, ("out", "lse", "D"))


@pytest.mark.parametrize("K,dh", [(4, 32), (3, 7)])
@pytest.mark.parametrize("graph", ["long", "longT"])
def test_two_calls_give_the_same_bits(pkg, ctx, graph, K, dh):
    """(4)"""
    Z, _, G, att = ref.tolerance_inputs(320, 320, K, dh)
    a, b = (_run(pkg, ctx, graph, Z, G, att, K, 64) for _ in range(2))
    for name in OUTPUTS:
        np.testing.assert_array_equal(_bits(a[name]), _bits(b[name]), err_msg=name)


@pytest.mark.parametrize("graph", ["long", "longT"])
def test_attention_dropout_draws_the_plain_mask(pkg, ctx, graph):
    """(5) p = 0.5: lse is the undropped split forward's bit for bit, and all six outputs are within TOL of the plain _drop
    calls', which test_gpu_gat_dropout.py ties to the reference"""
    K, dh = 4, 32
    Z, _, G, att = ref.tolerance_inputs(320, 320, K, dh)
    drop = pkg.ops.dropout_params(0.5) + (1234567, 3, 0, 0)
    got, plain = (_run(pkg, ctx, graph, Z, G, att, K, split, drop=drop) for split in (64, None))
    np.testing.assert_array_equal(_bits(got["lse"]), _bits(_run(pkg, ctx, graph, Z, G, att, K, 64)["lse"]))
    for name in OUTPUTS:
        d = relerr(got[name], plain[name])
        print(f"[gat split] drop {name}: {d:.3e}")
        assert d <= TOL, (name, d)


@pytest.mark.parametrize("attn_dropout", [0.0, 0.3])
def test_model_with_and_without_the_option(pkg, ctx, attn_dropout):
    """(6) gat(row_split=64) next to gat() from the same weights, on kernel_graph_long's pattern joined with its transpose
    (long rows in A and in A^T): three train_steps, then evaluate"""
    indptr, indices = ref.kernel_graph_long()
    rows = np.repeat(np.arange(320, dtype=np.uint32), np.diff(indptr.astype(np.int64)))
    r, c = np.concatenate([rows, indices]), np.concatenate([indices, rows])
    order = np.argsort(r, kind="stable")
    ip = np.zeros(321, dtype=np.uint32)
    ip[1:] = np.cumsum(np.bincount(r, minlength=320))
    ix = np.ascontiguousarray(c[order], dtype=np.uint32)
    sizes, rng = [16, 32, 8], np.random.default_rng(7)
    weights = [(0.3 * rng.standard_normal((a, b)), 0.1 * rng.standard_normal((1, b)), 0.3 * rng.standard_normal((2, b)))
               for a, b in zip(sizes, sizes[1:])]
    Xd = pkg.dn_matrix.from_numpy(rng.standard_normal((320, 16), dtype=np.float32))
    Yd = pkg.dn_matrix.from_numpy(rng.integers(0, 8, size=(320, 1)).astype(np.int32))
    models = [pkg.gat(pkg.csr_matrix(ip.copy(), ix.copy(), np.ones(ix.size, dtype=np.float32), 320), sizes, heads=4,
                      weights=weights, attn_dropout=attn_dropout, **kw) for kw in ({}, dict(row_split=64))]
    losses = [[np.asarray(M.train_step(ctx, Xd, Yd, 1e-2, 0.9, 0.999, 5e-4, 1e-8), dtype=np.float64) for _ in range(3)]
              for M in models]
    plan = pkg.ops.gat_split_plan(ctx, models[1].A, 64, 4, 32)
    assert plan.num_split_rows() > 5 and plan.num_slots() > 65 and "_gat_split_plans" not in models[0].A.__dict__
    for a, b in zip(*losses):
        print(f"[gat split] model attn_dropout={attn_dropout} loss {a} / {b}")
        assert np.all(np.abs(a - b) <= TOL * np.abs(a))
    for la, lb in zip(models[0].layers(), models[1].layers()):
        for t in ("W", "b", "att"):
            assert relerr(getattr(lb, t)().numpy(), getattr(la, t)().numpy()) <= TOL, (la.name, t)
    ea, eb = (M.evaluate(ctx, Xd, Yd) for M in models)
    assert ea.keys() == eb.keys() and all(abs(ea[k] - eb[k]) <= TOL for k in ea), (ea, eb)
