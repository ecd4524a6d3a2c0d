"""The skip kernels (include/mggcn.h: mggcn_gated_skip_forward_f32 / mggcn_gated_skip_backward_f32) and gat(skip=, norm=) on
the device, against the fp64 restatement and the reference models of gat_skip_ref.py.  Kernel level: every operand sits in a
guarded.Guarded buffer (NaN patterns around the logical matrix, checked bit for bit), every output is held to the bars
gat_skip_ref fixes on the CPU by the row-scaled measure, and everything that is claimed bitwise is compared as bits.  Model
level: the rules and TOL of test_gpu_gat.py."""
import numpy as np
import pytest

import bce_ref
import gat_skip_ref as gs
import layernorm_ref
from gat_ref import relerr, rowerr
from guarded import Guarded
from test_gpu_gat import N, TOL, _model_data
from test_gpu_gatv2 import MODELS, _gat

pytestmark = pytest.mark.gpu

ALL = ("o", "r", "y", "G", "act", "G_o", "G_r")         # the dense [n x m] operands of the two calls


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dense(n, m, pad, logical=None):
    """aligned: ld = m, base on a 256-byte boundary; padded: ld = m + 3, base one float off alignment"""
    return Guarded(n, m, m + 3 if pad else m, 1 if pad else 0, logical=logical, output=logical is None)


def run_device(ctx, c, padded=(), alias=None, rows=None):
    """both entry points once on case ``c`` through the C ABI with raw pointers; ``padded``: the operands of ALL that get
    ld = m + 3 and a base one float off alignment; ``alias``: "G" / "act" (G_o is that buffer) or "G_r" (G_r is G_o, add mode);
    ``rows``: (a, b) runs rows [a, b) alone.  Every buffer's guards are checked; returns the outputs as numpy arrays."""
    lib, st = ctx.lib, ctx.stream(0)
    a, b = (0, c["n"]) if rows is None else rows
    n, m, flags = b - a, c["m"], c["flags"]
    gated, leaky = bool(flags & gs.GATE), bool(flags & gs.LEAKY)
    cut = lambda M: None if M is None else np.ascontiguousarray(M[a:b])
    buf = {k: _dense(n, m, k in padded, cut(c[k])) for k in ("o", "r", "G")}
    buf["act"] = _dense(n, m, "act" in padded, cut(c["act"]))
    buf["y"] = _dense(n, m, "y" in padded)
    buf["G_o"] = buf[alias] if alias in ("G", "act") else _dense(n, m, "G_o" in padded)
    buf["G_r"] = buf["G_o"] if alias == "G_r" else _dense(n, m, "G_r" in padded)
    w = Guarded(3, m, m, 0, logical=c["w"]) if gated else None
    gate_out = Guarded(n, 1, 1, 0, output=True) if gated else None
    gate_in = Guarded(n, 1, 1, 0, logical=cut(c["gate"]).reshape(n, 1)) if gated else None
    G_w = Guarded(3, m, m, 0, output=True) if gated else None
    ptr = lambda g: None if g is None else g.ptr
    ctx.sync()
    lib.mggcn_gated_skip_forward_f32(st, buf["o"].ptr, buf["o"].ld, buf["r"].ptr, buf["r"].ld, ptr(w), buf["y"].ptr,
                                     buf["y"].ld, ptr(gate_out), n, m, flags)
    lib.mggcn_gated_skip_backward_f32(st, buf["G"].ptr, buf["G"].ld, buf["act"].ptr if leaky else None, buf["act"].ld,
                                      buf["o"].ptr if gated else None, buf["o"].ld, buf["r"].ptr if gated else None,
                                      buf["r"].ld, ptr(w), ptr(gate_in), buf["G_o"].ptr, buf["G_o"].ld, buf["G_r"].ptr,
                                      buf["G_r"].ld, ptr(G_w), n, m, flags)
    ctx.sync()
    what = f"n={n} m={m} flags={flags} padded={padded} alias={alias}"
    for k, g in list(buf.items()) + [("w", w), ("gate", gate_out), ("gate_in", gate_in), ("G_w", G_w)]:
        if g is None:
            continue
        g.check_guards(f"{what} {k}")
        if k in ("o", "r", "w", "gate_in") or (k in ("G", "act") and alias != k):
            g.check_unchanged(f"{what} {k}")
    got = {k: buf[k].values() for k in ("y", "G_o", "G_r")}
    if gated:
        got.update(gate=gate_out.values().reshape(-1), G_w=G_w.values())
    return got


def _assert_case(what, c, got):
    twin = gs.distances(c["twin"], c)
    for name, d in gs.distances(got, c).items():
        print(f"[gat-skip] {what} {name}: twin {twin[name]:.3e} device {d:.3e} (bar {gs.BAR[name]:.1e})")
        assert d <= gs.BAR[name], (what, name, d, "twin:", twin[name])


# ---- every entry point against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", gs.WIDTHS)
def test_every_entry_point_against_the_restatement(ctx, m):
    """y, gate, G_o, G_r and G_w within their bars at one width per instantiation and more, n = 1 and 37, with and without
    each flag, on aligned operands (float4 path where m % 4 == 0) -- and, where m % 4 == 0, with each dense operand in turn
    at ld = m + 3 one float off alignment, which moves the whole call to the element path"""
    for n in gs.ROWS:
        for flags in gs.FLAGS:
            c = gs.case(n, m, flags)
            _assert_case(f"n={n} m={m} flags={flags}", c, run_device(ctx, c))
    if m % 4 == 0:
        for flags in (gs.LEAKY, gs.GATE | gs.LEAKY):
            c = gs.case(37, m, flags)
            for k in ALL:
                _assert_case(f"n=37 m={m} flags={flags} padded {k}", c, run_device(ctx, c, padded=(k,)))


def test_all_operands_padded_at_the_widest_row(ctx):
    for flags in gs.FLAGS:
        c = gs.case(37, 1024, flags)
        _assert_case(f"n=37 m=1024 flags={flags} all padded", c, run_device(ctx, c, padded=ALL))


# ---- beyond one grid pass --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,vec", gs.INSTANTIATION_WIDTHS)
def test_more_rows_than_one_pass_of_the_grid(ctx, m, vec):
    """per instantiation the first row count that needs a second trip of the grid-stride loop (1024 workgroups x 256 / L
    groups x R rows in the first), plus 3: every row of y, gate, G_o and G_r and every column of G_w against the restatement"""
    inst = gs.instantiation(m, vec)
    n = gs.rows_per_pass(inst) + 1 + 3
    assert n * m <= 4200 * 1024
    for flags in (gs.LEAKY, gs.GATE | gs.LEAKY):
        c = gs.case(n, m, flags, seed=31, tail_gain=1000.0)
        got = run_device(ctx, c)
        _assert_case(f"{inst} n={n} m={m} flags={flags}", c, got)
        if flags & gs.GATE:                 # and the check can see the second trip: G_w without its rows is bars away
            k = gs.TAIL
            short = gs.restate64(c["o"][:-k], c["r"][:-k], c["w"], True, G=c["G"][:-k], act=c["act"][:-k], gate=c["gate"][:-k],
                                 exact=True)["G_w"]
            assert rowerr(short, c["want"]["G_w"], c["scale"]["G_w"])[1] > 100 * gs.BAR["G_w"]


# ---- bits ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [41, 128, 1024])
def test_bits_of_repeated_and_split_calls(ctx, m):
    """two calls give equal bits everywhere; every split of 37 rows into two calls gives the row-local bits of the whole
    call; G_w is equal across repeated calls"""
    for flags in (gs.LEAKY, gs.GATE | gs.LEAKY):
        c = gs.case(37, m, flags)
        whole = run_device(ctx, c)
        again = run_device(ctx, c)
        for k in whole:
            np.testing.assert_array_equal(_bits(whole[k]), _bits(again[k]), err_msg=f"m={m} flags={flags} {k}")
        for cut in range(1, 37):
            lo, hi = run_device(ctx, c, rows=(0, cut)), run_device(ctx, c, rows=(cut, 37))
            for k in ("y", "G_o", "G_r") + (("gate",) if flags & gs.GATE else ()):
                np.testing.assert_array_equal(_bits(np.concatenate([lo[k], hi[k]])), _bits(whole[k]),
                                              err_msg=f"m={m} flags={flags} cut={cut} {k}")


# ---- edges ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [7, 128])
def test_saturated_gates_and_equal_operands(ctx, m):
    """scores of exactly +-200 (w[0] = 1 in column 0, o[:, 0] = +-200, r[:, 0] = 0, the rest of w 0): g is exactly 1 / 0,
    nothing is NaN, ds = 0, so G_o = (1 - g) dy, G_r = g dy bit for bit and G_w = 0.  And o == r: dg = 0 exactly, so
    G_o = (1 - g) dy and G_r = g dy bit for bit with the gate that was handed in."""
    n = 37
    o, r, G, w = gs.inputs(n, m)
    w = np.zeros_like(w)
    w[0, 0] = 1.0
    o, r = o.copy(), r.copy()
    o[:, 0] = np.where(np.arange(n) % 2 == 0, 200.0, -200.0)
    r[:, 0] = 0.0
    want_g = np.where(np.arange(n) % 2 == 0, 1.0, 0.0).astype(np.float32)
    c = dict(n=n, m=m, flags=gs.GATE, o=o, r=r, G=G, w=w, act=None, gate=want_g)
    got = run_device(ctx, c)
    assert not any(np.isnan(v).any() for v in got.values())
    np.testing.assert_array_equal(_bits(got["gate"]), _bits(want_g))
    np.testing.assert_array_equal(got["y"], np.where(want_g[:, None] == 1, r, o))
    np.testing.assert_array_equal(got["G_o"], (1 - want_g)[:, None] * G)
    np.testing.assert_array_equal(got["G_r"], want_g[:, None] * G)
    assert not got["G_w"].any()
    o2, r2, G2, w2 = gs.inputs(n, m, seed=33)
    g2 = np.linspace(0.05, 0.95, n).astype(np.float32)
    c = dict(n=n, m=m, flags=gs.GATE, o=o2, r=o2.copy(), G=G2, w=w2, act=None, gate=g2)
    got = run_device(ctx, c)
    np.testing.assert_array_equal(_bits(got["G_o"]), _bits((np.float32(1) - g2)[:, None] * G2))
    np.testing.assert_array_equal(_bits(got["G_r"]), _bits(g2[:, None] * G2))
    assert not got["G_w"].any()


def test_no_rows(ctx):
    """n_rows = 0: the guards are intact, the backward's G_w is all +0.0 and nothing else is written"""
    for m in (7, 128):
        for flags in gs.FLAGS:
            c = gs.case(1, m, flags)
            got = run_device(ctx, c, rows=(0, 0))
            if flags & gs.GATE:
                np.testing.assert_array_equal(_bits(got["G_w"]), np.zeros((3, m), dtype=np.uint32))


@pytest.mark.parametrize("m", [41, 128])
def test_allowed_aliases(ctx, m):
    """G_o = G, G_o = act and (add mode) G_r = G_o give the bits of the call on separate buffers"""
    for flags in (gs.LEAKY, gs.GATE | gs.LEAKY):
        c = gs.case(37, m, flags)
        base = run_device(ctx, c)
        for alias in ("G", "act") + (() if flags & gs.GATE else ("G_r",)):
            got = run_device(ctx, c, alias=alias)
            for k in ("G_o", "G_r") + (("G_w",) if flags & gs.GATE else ()):
                np.testing.assert_array_equal(_bits(got[k]), _bits(base[k]), err_msg=f"m={m} flags={flags} alias={alias} {k}")


# ---- the model --------------------------------------------------------------------------------------------------------------------------------
def _oracle(oracle, csr, sizes, heads, variant, **kw):
    ip, ix, dv = csr
    per_layer = [heads] * (len(sizes) - 2) + [1]
    return gs.ORACLES[variant](oracle, oracle.Csr(ip.copy(), ix.copy(), dv.copy(), N), sizes, per_layer, **kw)


def _owners(layer):
    """(name, device owner, parameter, gradient, m, v) of everything the layer trains, in params() order"""
    out = [("W", layer.lin, "W", "G_W", "mW", "vW"), ("b", layer.lin, "b", "G_b", "mb", "vb")]
    if layer.attn.att is not None:
        out.append(("att", layer.attn, "att", "G_att", "m", "v"))
    if layer.res_lin is not None:
        out += [("W_r", layer.res_lin, "W", "G_W", "mW", "vW"), ("b_r", layer.res_lin, "b", "G_b", "mb", "vb")]
    if layer.gate is not None:
        out.append(("w", layer.gate, "w", "G_w", "m", "v"))
    if layer.norm is not None:
        out += [("gamma", layer.norm, "gamma", "G_gamma", "mg", "vg"), ("beta", layer.norm, "beta", "G_beta", "mb", "vb")]
    return out


def _oracle_slots(ol):
    """name -> (object, parameter, gradient, m, v, step) attribute names on the reference layer"""
    slots = {"W": (ol.lin, "W", "G_W", "mW", "vW", "step"), "b": (ol.lin, "b", "G_b", "mb", "vb", "step"),
             "att": (ol, "att", "G_att", "m", "v", "step"), "w": (ol, "w", "G_w", "wm", "wv", "wstep")}
    if ol.res is not None:
        slots.update({"W_r": (ol.res, "W", "G_W", "mW", "vW", "step"), "b_r": (ol.res, "b", "G_b", "mb", "vb", "step")})
    if ol.norm is not None:
        slots.update({"gamma": (ol.norm, "gamma", "G_gamma", "mg", "vg", "step"), "beta": (ol.norm, "beta", "G_beta", "mb", "vb", "step")})
    return slots


def _sync_oracle_state(G, O):
    """identical inputs for the next epoch: the reference takes over the device's parameters and Adam moments"""
    for layer, ol in zip(G.layers(), O.layers):
        slots = _oracle_slots(ol)
        for name, owner, p, _, m, v in _owners(layer):
            obj, op, _, om, ov, ostep = slots[name]
            setattr(obj, op, getattr(owner, p).numpy().copy())
            if getattr(owner, m) is not None:
                setattr(obj, om, getattr(owner, m).numpy().copy())
                setattr(obj, ov, getattr(owner, v).numpy().copy())
                setattr(obj, ostep, owner.step)


def _epochs(pkg, ctx, G, O, X, Y, what, epochs=3, score_tol=3.0 / N):
    """test_gpu_gat.test_gat_epochs_match_the_reference's rules over every trained tensor of the model: loss at TOL, the
    score within 3 / n, every gradient at TOL (G_W_r, G_b_r, G_w, G_gamma and G_beta as G_W is), every updated matrix parameter
    never more than a sign flip away and at TOL in the well-conditioned entries"""
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    lr = 1e-2
    for epoch in range(epochs):
        _sync_oracle_state(G, O)
        loss, acc = G.train_forward(ctx, Xd, Yd)
        G.backward(ctx)
        ctx.sync()
        grads = [{name: getattr(owner, g).numpy().copy() for name, owner, _, g, _, _ in _owners(l)} for l in G.layers()]
        G.adam_update(ctx, lr, 0.9, 0.999, 5e-4, 1e-8)
        ctx.sync()
        ol, oa = O.train_forward(X, Y)
        O.backward()
        ograds = [{name: np.array(getattr(obj, g)) for name, (obj, _, g, _, _, _) in _oracle_slots(l).items()
                   if name in grads[li]} for li, l in enumerate(O.layers)]
        O.adam_update()
        print(f"[gat-skip] {what} epoch {epoch}: loss {loss!r} (reference {ol!r}), score {acc!r} ({oa!r})")
        assert np.isfinite(ol)
        assert abs(loss - ol) <= TOL * abs(ol), (epoch, loss, ol)
        assert acc == oa or abs(acc - oa) <= score_tol, (epoch, acc, oa)
        for li, (layer, olayer) in enumerate(zip(G.layers(), O.layers)):
            assert set(grads[li]) == set(ograds[li])
            slots = _oracle_slots(olayer)
            for name, owner, p, _, _, _ in _owners(layer):
                d = relerr(grads[li][name], ograds[li][name])
                print(f"[gat-skip] {what} epoch {epoch} layer {li} G_{name}: {d:.3e}")
                assert d <= TOL, (what, epoch, li, name, d)
                if name in ("W", "att", "W_r", "w", "gamma"):
                    P, Po, g = getattr(owner, p).numpy(), getattr(slots[name][0], slots[name][1]), ograds[li][name]
                    assert np.abs(P - Po).max() <= 2.05 * lr, (epoch, li, name)          # never more than a sign flip
                    solid = np.abs(g) > 1e-2 * np.abs(g).max()                          # well-conditioned entries
                    assert np.abs(P - Po)[solid].max() <= TOL * np.abs(Po).max(), (epoch, li, name)


def _init_norms(G, O, seed=5):
    """a non-trivial gamma and beta on both sides (ones and zeros would hide a missing multiply or add)"""
    for li, (layer, ol) in enumerate(zip(G.layers(), O.layers)):
        assert (layer.norm is None) == (ol.norm is None)
        if layer.norm is not None:
            gamma, beta = layernorm_ref.params(layer.norm.gamma.m(), seed + li)
            layer.norm.init(gamma, beta)
            ol.norm.gamma, ol.norm.beta = gamma.copy(), beta.copy()


def _assert_same_init(G, O):
    for layer, ol in zip(G.layers(), O.layers):                     # same seed-99 init, bit for bit
        slots = _oracle_slots(ol)
        for name, owner, p, _, _, _ in _owners(layer):
            np.testing.assert_array_equal(getattr(owner, p).numpy(), getattr(slots[name][0], slots[name][1]), err_msg=name)


CASES = [("v1", dict(skip="gate"), {}),
         ("v2", dict(skip="add"), {}),
         ("dot", dict(skip="gate", norm="layer"), {}),
         ("v1", dict(skip="gate", norm="layer"), dict(dropout=0.5, attn_dropout=0.3))]


@pytest.mark.parametrize("variant,options,drop", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_epochs_match_the_reference(pkg, oracle, ctx, variant, options, drop):
    """three full epochs (forward, loss, backward, Adam) against the reference model on identical inputs"""
    sizes, heads = MODELS[1]
    csr, X, Y = _model_data(pkg, sizes)
    G = _gat(pkg, csr, sizes, heads, variant=variant, **options, **drop)
    okw = {}
    if drop:
        G.set_dropout(drop["dropout"], seed=0xC0FFEE123, epoch=4, attn=drop["attn_dropout"])
        okw = dict(p=drop["dropout"], attn_p=drop["attn_dropout"], seed=0xC0FFEE123, epoch=4)
    O = _oracle(oracle, csr, sizes, heads, variant, **options, **okw)
    _assert_same_init(G, O)
    _init_norms(G, O)
    assert [l.res_lin is not None for l in G.layers()] == [True] * 3
    assert [l.norm is not None for l in G.layers()] == [options.get("norm") is not None] * 2 + [False]
    _epochs(pkg, ctx, G, O, X, Y, f"{variant} {options} {drop}")
    if drop:
        assert G.dropout_epoch == 7


def test_bce_epoch_with_splits_matches_the_reference(pkg, oracle, ctx):
    """loss="bce" over the training rows of set_splits: one epoch of gat(variant="dot", skip="gate", norm="layer") against the
    reference model with the fp32 restatement of the multi-label loss"""
    sizes, heads = MODELS[1]
    csr, X, _ = _model_data(pkg, sizes)
    T = (np.random.default_rng(3).random((N, sizes[-1])) < 0.2).astype(np.int32)
    S = np.random.default_rng(4).choice(4, size=N, p=(0.5, 0.2, 0.25, 0.05)).astype(np.int32)
    train = S == 0
    G = _gat(pkg, csr, sizes, heads, loss="bce", variant="dot", skip="gate", norm="layer")
    G.set_splits(S)

    def loss(H):
        Gr = np.ascontiguousarray(bce_ref.grad32(H, T, 1.0 / (float(train.sum()) * H.shape[1])))
        Gr[~train] = 0
        return Gr, (float(bce_ref.loss32(H, T).astype(np.float64)[train].sum() / (train.sum() * H.shape[1])),
                    bce_ref.micro_f1(*bce_ref.counts(H[train], T[train])[0]))
    O = _oracle(oracle, csr, sizes, heads, "dot", skip="gate", norm="layer", loss=loss)
    _init_norms(G, O)
    _epochs(pkg, ctx, G, O, X, T, "bce + splits", epochs=1, score_tol=3.0 / int(train.sum()))
    assert G.split_metrics()["counts"]["train"] == int(train.sum())


def _state_bits(G):
    out = []
    for l in G.layers():
        for _, owner, p, g, m, v in _owners(l):
            out += [getattr(owner, a).numpy().view(np.uint32).copy() for a in (p, g, m, v)]
    return out


def _run_epochs(pkg, ctx, fused, step, variant, epochs=3, **kw):
    sizes, heads = MODELS[0]
    csr, X, Y = _model_data(pkg, sizes)
    G = _gat(pkg, csr, sizes, heads, fused=fused, variant=variant, **kw)
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
    return res, _state_bits(G), G


@pytest.mark.parametrize("variant", ["v1", "dot"])
def test_fused_and_per_tensor_adam_give_the_same_bits(pkg, ctx, variant):
    """fused=True against fused=False, and train_step against the three calls: the same losses and the same bits in every
    parameter, gradient and Adam moment -- W_r, b_r, w, gamma and beta included -- after three epochs"""
    kw = dict(skip="gate", norm="layer")
    base = _run_epochs(pkg, ctx, False, False, variant, **kw)
    # three layers of W, b, (att,) W_r, b_r, w, and gamma, beta in the two that have an activation: 4 arrays each
    assert len(base[1]) == 4 * (3 * (6 if variant == "v1" else 5) + 4)
    for fused, step in ((True, False), (True, True)):
        res, bits, _ = _run_epochs(pkg, ctx, fused, step, variant, **kw)
        assert res == base[0], (fused, step)
        for a, b in zip(bits, base[1]):
            np.testing.assert_array_equal(a, b)
    assert base[0][-1][0] < base[0][0][0], base[0]                 # and it trains


def test_evaluate_and_predict_agree_with_a_plain_forward(pkg, ctx):
    sizes, heads = MODELS[1]
    csr, X, Y = _model_data(pkg, sizes)
    S = np.random.default_rng(4).choice(3, size=N).astype(np.int32)
    G = _gat(pkg, csr, sizes, heads, variant="dot", skip="gate", norm="layer", dropout=0.5)
    Xd, Yd, Sd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y), pkg.dn_matrix.from_numpy(S.reshape(-1, 1))
    G.train_step(ctx, Xd, Yd, 1e-2, 0.9, 0.999, 5e-4, 1e-8)
    res = G.evaluate(ctx, Xd, Yd, Sd)
    out = G(ctx, Xd)
    ctx.sync()
    logits = out.numpy()
    hit = logits.argmax(axis=1) == Y.reshape(-1)
    assert res["all"] == float(hit.mean())
    for k, name in enumerate(("train", "val", "test")):
        assert res[name] == float(hit[S == k].mean())
    np.testing.assert_array_equal(G.predict(ctx, Xd).reshape(-1), logits.argmax(axis=1))
    assert G.dropout_epoch == 1                                    # neither dropped


def test_selector_restores_the_best_epoch_and_checkpoints_are_refused(pkg, ctx, tmp_path):
    """model_selector.restore brings back the best epoch's W, W_r, w and gamma bit for bit (and resets Adam) through the
    generic parameter readers; save, load and save_best raise and leave the directory empty"""
    sizes, heads = MODELS[0]
    csr, X, Y = _model_data(pkg, sizes)
    S = np.random.default_rng(4).choice(3, size=N).astype(np.int32)
    G = _gat(pkg, csr, sizes, heads, variant="v1", skip="gate", norm="layer")
    G.set_splits(S)
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    sel = pkg.model_selector(G, split="val", metric="loss")
    names = [name for name, _ in sel._params()]
    assert names[:8] == ["W0", "b0", "att0", "res_W0", "res_b0", "gate0", "gamma0", "beta0"] and "gamma2" not in names
    snaps = []
    for _ in range(4):
        snaps.append({name: t.numpy().view(np.uint32).copy() for name, t in sel._params()})
        sel.step(ctx, Xd, Yd, 0.3 if len(snaps) > 2 else 1e-2, 0.9, 0.999, 5e-4, 1e-8)
    assert sel.best_epoch is not None
    sel.restore(ctx)
    for name, t in sel._params():
        np.testing.assert_array_equal(t.numpy().view(np.uint32), snaps[sel.best_epoch][name], err_msg=name)
    for l in G.layers():
        for _, owner, _, _, m, v in _owners(l):
            assert owner.step == 0 and not getattr(owner, m).numpy().any() and not getattr(owner, v).numpy().any()
    path = str(tmp_path / "model.ckpt")
    for call in (lambda: G.save(ctx, path), lambda: G.load(ctx, path), lambda: sel.save_best(ctx, path)):
        with pytest.raises(ValueError, match="skip"):
            call()
    assert not list(tmp_path.iterdir())


# ---- the defaults ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["v1", "v2", "dot"])
def test_defaults_are_what_they_were(pkg, variant):
    """skip=None, norm=None spelled out: the timers, the parameters and the bits of a model built without the arguments"""
    sizes, heads = MODELS[0]
    csr, X, Y = _model_data(pkg, sizes)
    runs = []
    for kw in ({}, dict(skip=None, norm=None, skip_weights=None)):
        c = pkg.context(0)
        G = _gat(pkg, csr, sizes, heads, variant=variant, **kw)
        Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
        res = [G.train_step(c, Xd, Yd, 1e-2, 0.9, 0.999, 5e-4, 1e-8) for _ in range(2)]
        for l in G.layers():
            assert l.params() == ([l.lin] if variant == "dot" else [l.lin, l.attn])
            assert l.res_lin is None and l.gate is None and l.norm is None and l.skip is None
            assert (l.act is l.out) == (not l.activation)
        assert not hasattr(G, "skip_buffer")
        bits = [t.numpy().view(np.uint32).copy() for l in G.layers() for p in l.params() for t, *_ in p.adam_tensors(0.0)]
        runs.append((res, sorted(c.timers), bits))
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    assert not any("skip" in t or "norm" in t for t in runs[0][1])
    for a, b in zip(runs[0][2], runs[1][2]):
        np.testing.assert_array_equal(a, b)


def test_timers_of_a_full_layer(pkg, ctx):
    sizes, heads = MODELS[0]
    csr, X, Y = _model_data(pkg, sizes)
    c = pkg.context(0)
    G = _gat(pkg, csr, sizes, heads, variant="dot", skip="gate", norm="layer")
    G.train_step(c, pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y), 1e-2, 0.9, 0.999, 5e-4, 1e-8)
    for li in range(3):
        assert f"{li}_0_skip" in c.timers and f"{li}_1_skip" in c.timers
        assert (f"{li}_0_norm" in c.timers) == (li < 2) and (f"{li}_1_norm" in c.timers) == (li < 2)
        assert f"{li}_0_activation" not in c.timers
