"""gat(agg_dtype="bf16") on the device, by the twin method and bit for bit: the bf16 operators and models against fp32 ones
whose attention runs a driver written here -- it rounds an operand on the device (ops.convert_bf16), widens the image
exactly ((u16 << 16) as fp32) and calls the fp32 ops with the widened operand in the gathered roles and the fp32 tensor in
the own-row roles.  That pins the plumbing: which operand is rounded, when, and that the shared image buffers are never
read stale across layers.  Then what follows from the semantics: evaluate / predict, checkpoints across the two forms, the
exports, that it trains, and that the default is the model as it was."""
from importlib import import_module

import numpy as np
import pytest

import gat_ref as ref
from test_gpu_gat import N, _model_data

pytestmark = pytest.mark.gpu

ADAM = (1e-2, 0.9, 0.999, 5e-4, 1e-8)
MODELS = {"v1": ([48, 32, 32, 7], 4), "v2": ([20, 16, 12, 5], 4), "dot": ([48, 32, 32, 7], 4)}     # float4 and element paths
VARIANTS = ("v1", "v2", "dot")


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


@pytest.fixture(scope="module")
def gat(pkg):
    return import_module(pkg.__name__ + ".gat")


def _bits(t):
    return np.ascontiguousarray(t.numpy() if hasattr(t, "numpy") and not isinstance(t, np.ndarray) else t).view(np.uint32)


def _twin_classes(pkg, gat):
    """subclasses of the three attentions that run the driver: fp32 kernels on device-widened operands"""
    torch, ops = _torch(), pkg.ops

    def widen(self, ctx, M):
        img = torch.empty((M.n(), M.m()), dtype=torch.bfloat16, device="cuda")
        ops.convert_bf16(ctx, M, img)
        W = pkg.dn_matrix(M.n(), M.m())
        with torch.cuda.stream(ctx.cuda_streams[0]):
            W.t.copy_((img.view(torch.int16).to(torch.int32) << 16).view(torch.float32))
        self.__dict__.setdefault("_keep", []).extend((img, W))       # alive until the stream has used them
        return W

    class twin_v1(gat.attention):
        def __call__(self, ctx, F, Z, out, drop=None):
            ops.gat_scores(ctx, Z, self.att, self.s_dst, self.s_src, self.heads)
            ops.gat_forward(ctx, F, widen(self, ctx, Z), self.s_dst, self.s_src, out, self.lse, self.heads, self.slope, None, drop)

        def backward(self, ctx, F, F_T, Z, G, out, G_Z, drop=None):
            Zw, Gw = widen(self, ctx, Z), widen(self, ctx, G)
            ops.gat_backward_dst(ctx, F, Zw, self.s_dst, self.s_src, self.lse, G, out, self.D, self.ds_dst, self.heads,
                                 self.slope, None, drop)
            ops.gat_backward_src(ctx, F_T, Z, self.s_dst, self.s_src, self.lse, self.D, Gw, self.att, self.ds_dst, self.ds_src,
                                 G_Z, self.heads, self.slope, None, drop)
            ops.gat_scores_backward(ctx, self.ds_dst, Z, self.ds_src, Z, self.G_att, self.heads)

    class twin_v2(gat.attention_v2):
        def __call__(self, ctx, F, Z2, out, drop=None):
            ops.gatv2_forward(ctx, F, widen(self, ctx, Z2), Z2, self.att, out, self.lse, self.heads, self.slope)

        def backward(self, ctx, F, F_T, Z2, G, out, G_Z2, drop=None):
            Zw, Gw = widen(self, ctx, Z2), widen(self, ctx, G)
            ops.gatv2_backward_dst(ctx, F, Zw, Z2, self.att, self.lse, G, out, self.D, G_Z2, self.P, self.heads, self.slope)
            ops.gatv2_att_grad(ctx, self.P, self.G_att)
            ops.gatv2_backward_src(ctx, F_T, Z2, Zw, self.att, self.lse, self.D, Gw, G_Z2, self.heads, self.slope)

    class twin_dot(gat.attention_dot):
        def __call__(self, ctx, F, Z3, out, drop=None):
            Zw = widen(self, ctx, Z3)
            ops.gatdot_forward(ctx, F, Z3, Zw, Zw, out, self.lse, self.heads, self.scale)

        def backward(self, ctx, F, F_T, Z3, G, out, G_Z3, drop=None):
            Zw, Gw = widen(self, ctx, Z3), widen(self, ctx, G)
            ops.gatdot_backward_dst(ctx, F, Z3, Zw, Zw, self.lse, G, out, self.D, G_Z3, self.heads, self.scale)
            ops.gatdot_backward_src(ctx, F_T, Zw, Z3, Z3, self.lse, self.D, Gw, G_Z3, G_Z3, self.heads, self.scale)

    return {"v1": twin_v1, "v2": twin_v2, "dot": twin_dot}


def _operator(gat, variant, n, out, heads, agg_dtype):
    if variant == "v1":
        return gat.attention("0_", n, n, out, heads, agg_dtype=agg_dtype)
    if variant == "v2":
        return gat.attention_v2("0_", n, out, heads, agg_dtype=agg_dtype)
    return gat.attention_dot("0_", n, out, heads, agg_dtype=agg_dtype)


OPERATOR_OUTPUTS = {"v1": ("s_dst", "s_src", "lse", "D", "ds_dst", "ds_src", "G_att"), "v2": ("lse", "D", "P", "G_att"),
                    "dot": ("lse", "D")}


@pytest.mark.parametrize("K,dh", [(4, 32), (3, 7)])
@pytest.mark.parametrize("variant", VARIANTS)
def test_operator_twin(pkg, gat, ctx, variant, K, dh):
    """attention / attention_v2 / attention_dot built for "bf16", forward and backward on kernel_graph_long: every output
    has the driver's bits, and at least one differs from the all-fp32 operator (the rounding really happened)"""
    indptr, indices = ref.kernel_graph_long()
    n, d, zw = indptr.size - 1, K * dh, {"v1": 1, "v2": 2, "dot": 3}[variant]
    F = pkg.csr_matrix(indptr.copy(), indices.copy(), np.ones(indices.size, dtype=np.float32), n)
    F_T = F.transpose()
    rng = np.random.default_rng(31 + d)
    Z = pkg.dn_matrix.from_numpy(rng.standard_normal((n, zw * d), dtype=np.float32))
    G = pkg.dn_matrix.from_numpy(rng.standard_normal((n, d), dtype=np.float32))
    twin_cls = _twin_classes(pkg, gat)[variant]
    res = {}
    for key in ("bf16", "twin", "f32"):
        A = _operator(gat, variant, n, d, K, "bf16" if key == "bf16" else "f32")
        if key == "twin":
            A.__class__ = twin_cls
        out, G_Z = pkg.dn_matrix(n, d), pkg.dn_matrix(n, zw * d)
        A(ctx, F, Z, out)
        A.backward(ctx, F, F_T, Z, G, out, G_Z)
        ctx.sync()
        res[key] = dict(out=_bits(out), G_Z=_bits(G_Z), **{k: _bits(getattr(A, k)) for k in OPERATOR_OUTPUTS[variant]})
        assert np.isfinite(out.numpy()).all() and np.isfinite(G_Z.numpy()).all() and np.abs(G_Z.numpy()).max() > 0
        if key == "bf16":
            assert A.Z16.shape() == (n, zw * d) and A.G16.shape() == (n, d)
            assert "0_0_gat-convert" in ctx.timers and "0_1_gat-convert" in ctx.timers
    for k in res["bf16"]:
        np.testing.assert_array_equal(res["bf16"][k], res["twin"][k], err_msg=f"{variant} ({K}, {dh}) {k}")
    assert any((res["bf16"][k] != res["f32"][k]).any() for k in res["bf16"])


def _state(G):
    out = []
    for l in G.layers():
        ts = [l.W(), l.b(), l.GW(), l.Gb(), l.lin.mW, l.lin.vW, l.lin.mb, l.lin.vb, l.att(), l.Gatt(), l.attn.m, l.attn.v, l.G_Z]
        if l.res_lin is not None:
            ts += [l.res_lin.W, l.res_lin.b, l.res_lin.G_W, l.res_lin.G_b]
        if l.gate is not None:
            ts += [l.gate.w, l.gate.G_w]
        if l.label is not None:
            ts += [l.label.E, l.label.G_E]
        out += [None if t is None else _bits(t).copy() for t in ts]
    return out


def _build(pkg, gat, variant, agg_dtype, twin=False, prepare=None, **kw):
    sizes, heads = MODELS[variant]
    csr, X, Y = _model_data(pkg, sizes)
    ip, ix, dv = csr
    G = pkg.gat(pkg.csr_matrix(ip.copy(), ix.copy(), dv.copy(), N), sizes, heads=heads, variant=variant,
                agg_dtype=agg_dtype, **kw)
    if twin:
        cls = _twin_classes(pkg, gat)[variant]
        for layer in G.layers():
            layer.attn.__class__ = cls
    if prepare is not None:
        prepare(G, Y)
    return G, X, Y


def _train(pkg, ctx, G, X, T, steps=3):
    Xd, Td = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(T)
    losses = [G.train_step(ctx, Xd, Td, *ADAM) for _ in range(steps)]
    ctx.sync()
    return losses, _state(G)


def _assert_same_model(what, a, b):
    assert a[0] == b[0], (what, a[0], b[0])
    assert len(a[1]) == len(b[1])
    for i, (x, y) in enumerate(zip(a[1], b[1])):
        assert (x is None) == (y is None), (what, i)
        if x is not None:
            np.testing.assert_array_equal(x, y, err_msg=f"{what}: tensor {i}")


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("variant", VARIANTS)
def test_model_twin(pkg, gat, ctx, variant, fused):
    """three train_steps of gat(agg_dtype="bf16") against the fp32 model whose attentions run the driver: the three losses
    and every parameter, gradient and Adam moment bit for bit; the loss falls; the difference to the all-fp32 model is
    printed per epoch, not asserted"""
    G, X, Y = _build(pkg, gat, variant, "bf16", fused=fused)
    assert G.agg_dtype == "bf16" and G.Z_image_buffer.numel() == N * {"v1": 1, "v2": 2, "dot": 3}[variant] * max(G.sizes[1:])
    assert G.G_image_buffer.numel() == N * max(G.sizes[1:])
    mine = _train(pkg, ctx, G, X, Y)
    assert any(name.endswith("0_gat-convert") for name in ctx.timers) and any(name.endswith("1_gat-convert") for name in ctx.timers)
    T, _, _ = _build(pkg, gat, variant, "f32", twin=True, fused=fused)
    _assert_same_model((variant, fused), mine, _train(pkg, ctx, T, X, Y))
    assert mine[0][2][0] < mine[0][0][0], mine[0]
    P, _, _ = _build(pkg, gat, variant, "f32", fused=fused)
    plain = _train(pkg, ctx, P, X, Y)
    print(f"[gat bf16] {variant} fused={fused}: loss bf16 - f32 per epoch "
          + ", ".join(f"{a[0] - b[0]:+.3e}" for a, b in zip(mine[0], plain[0])) + f" (f32 losses {[round(b[0], 6) for b in plain[0]]})")
    assert any(x is not None and (x != y).any() for x, y in zip(mine[1], plain[1]))


def _splits():
    return np.random.default_rng(4).choice(4, size=N, p=(0.5, 0.2, 0.25, 0.05)).astype(np.int32)


def _prepare_labels(pkg):
    def prepare(G, Y):
        G.set_splits(pkg.dn_matrix.from_numpy(_splits().reshape(-1, 1)))
        G.set_label_input(pkg.dn_matrix.from_numpy(Y), seed=5)
    return prepare


def _prepare_splits(pkg):
    return lambda G, Y: G.set_splits(pkg.dn_matrix.from_numpy(_splits().reshape(-1, 1)))


@pytest.mark.parametrize("variant,kw,prepare,bce", [
    ("v1", dict(dropout=0.5, attn_dropout=0.6), None, False),
    ("dot", dict(skip="gate", norm="layer", label_input=0.5), _prepare_labels, False),
    ("v2", dict(loss="bce"), _prepare_splits, True)])
def test_options_compose(pkg, gat, ctx, variant, kw, prepare, bce):
    """both dropouts on v1; gated skip, layer norm and label input on dot; the multi-label loss with splits on GATv2: the
    twin's bits after three train_steps"""
    prep = prepare(pkg) if prepare is not None else None
    G, X, Y = _build(pkg, gat, variant, "bf16", prepare=prep, **kw)
    T, _, _ = _build(pkg, gat, variant, "f32", twin=True, prepare=prep, **kw)
    target = (np.random.default_rng(3).random((N, G.sizes[-1])) < 0.2).astype(np.int32) if bce else Y
    _assert_same_model((variant, kw), _train(pkg, ctx, G, X, target), _train(pkg, ctx, T, X, target))


@pytest.mark.parametrize("variant", VARIANTS)
def test_evaluate_and_predict_run_the_bf16_forward(pkg, gat, ctx, variant):
    G, X, Y = _build(pkg, gat, variant, "bf16")
    S = np.random.default_rng(4).choice(3, size=N).astype(np.int32)
    Xd, Yd, Sd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y), pkg.dn_matrix.from_numpy(S.reshape(-1, 1))
    res = G.evaluate(ctx, Xd, Yd, Sd)
    logits = G(ctx, Xd)
    ctx.sync()
    logits = logits.numpy().copy()
    hit = logits.argmax(axis=1) == Y.reshape(-1)
    assert res["all"] == float(hit.mean())
    pred = G.predict(ctx, Xd)
    ctx.sync()
    pred = pred.numpy() if hasattr(pred, "numpy") else np.asarray(pred)
    if pred.shape == logits.shape:
        np.testing.assert_array_equal(_bits(pred), _bits(logits))
    else:
        np.testing.assert_array_equal(pred.reshape(-1), logits.argmax(axis=1))
    P, _, _ = _build(pkg, gat, variant, "f32")
    plain = P(ctx, Xd)
    ctx.sync()
    assert (_bits(plain) != _bits(logits)).any()                    # it is the bf16 forward


def test_checkpoints_cross_the_two_forms_and_the_exports(pkg, gat, ctx, tmp_path):
    """agg_dtype is an execution option, not stored: a file saved by the bf16 v1 model loads into an f32 model and back with
    every parameter bit for bit; v1 attention_weights of LAYER 0 of the bf16 model are the f32 model's on the same weights
    and input (its scores and lse never see an image; the layers above read different inputs in the two models and are only
    checked to be finite); the GATv2 export under bf16 is refused"""
    B, X, Y = _build(pkg, gat, "v1", "bf16")
    _train(pkg, ctx, B, X, Y, steps=2)
    path = str(tmp_path / "bf16.ckpt")
    B.save(ctx, path)
    P, _, _ = _build(pkg, gat, "v1", "f32")
    P.load(ctx, path)
    ctx.sync()
    params = lambda G: [_bits(t) for l in G.layers() for t in (l.W(), l.b(), l.att(), l.lin.mW, l.lin.vW, l.attn.m, l.attn.v)]
    for x, y in zip(params(B), params(P)):
        np.testing.assert_array_equal(x, y)
    assert P.agg_dtype == "f32" and B.agg_dtype == "bf16"
    back = str(tmp_path / "f32.ckpt")
    P.save(ctx, back)
    B2, _, _ = _build(pkg, gat, "v1", "bf16")
    B2.load(ctx, back)
    ctx.sync()
    for x, y in zip(params(B), params(B2)):
        np.testing.assert_array_equal(x, y)
    Xd = pkg.dn_matrix.from_numpy(X)
    a, b = B.attention_weights(ctx, Xd), P.attention_weights(ctx, Xd)
    ctx.sync()
    np.testing.assert_array_equal(_bits(a[0]), _bits(b[0]))          # layer 0: the same weights and input, fp32 scores
    assert np.isfinite(a[-1].numpy()).all()
    V, _, _ = _build(pkg, gat, "v2", "bf16")
    with pytest.raises(ValueError, match="agg_dtype"):
        V.attention_weights(ctx, Xd)
    with pytest.raises(ValueError, match="agg_dtype"):
        V.layers()[0].alpha(ctx)


@pytest.mark.parametrize("variant", VARIANTS)
def test_the_default_is_the_model_as_it_was(pkg, gat, variant):
    """gat(agg_dtype="f32") and gat() give the same bits after one train_step, register no gat-convert timer and own no
    image buffer (a context of their own: the timers of the other tests are not theirs)"""
    ctx = pkg.context(0)
    sizes, heads = MODELS[variant]
    csr, X, Y = _model_data(pkg, sizes)
    ip, ix, dv = csr
    states = []
    for kw in ({}, {"agg_dtype": "f32"}):
        G = pkg.gat(pkg.csr_matrix(ip.copy(), ix.copy(), dv.copy(), N), sizes, heads=heads, variant=variant, **kw)
        states.append(_train(pkg, ctx, G, X, Y, steps=1))
        assert G.agg_dtype == "f32" and G.Z_image_buffer is None and G.G_image_buffer is None
        assert all(l.attn.Z16 is None and l.attn.G16 is None for l in G.layers())
    _assert_same_model(variant, *states)
    assert not any("gat-convert" in name for name in list(ctx.timers) + list(ctx.events))
