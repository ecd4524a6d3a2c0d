"""The label-input kernels (include/mggcn.h: mggcn_label_input_forward_f32 / mggcn_label_input_backward_f32) and
gat(label_input=rate) on the device, against the restatement of label_input_ref.py.  Kernel level: every dense operand sits
in a guarded.Guarded buffer (NaN patterns around the logical matrix, checked bit for bit); the forward is compared as bits
(every element is one fp32 add), the backward against the fp64 restatement at the derivable bound
|err| <= gamma_k sum |g_i|, k the fed rows of the class, and as bits across calls.  Model level: a second gat on the
augmented features [X | M onehot(y)] and weights [W ; E] is the reference, at the bars of test_gpu_gat.py."""
import numpy as np
import pytest

import label_input_ref as li
from gat_ref import ADAM, relerr
from guarded import Guarded
from test_gpu_gat import TOL

pytestmark = pytest.mark.gpu

L = li.CHUNK                                                   # the backward kernel's own chunk length
T_SIZES = (0, 1, L - 1, L, L + 1, 2 * L + 1)
ROW0_FAR = (1 << 32) + 77


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dense(n, m, pad, logical=None):
    """aligned: ld = m, base on a 256-byte boundary; padded: ld = m + 3, base one float off alignment (the element path)"""
    return Guarded(n, m, m + 3 if pad else m, 1 if pad else 0, logical=logical, output=logical is None)


def _int_tensor(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def make_case(T, width, C, classes, seed):
    """T training rows among n = T + 9 (scattered, so that rows outside the list exist on both sides), their classes by
    ``classes``: "spread" (drawn from every third class: the others are empty) or an int (that class owns every row)"""
    rng = np.random.default_rng(seed)
    n = T + 9
    S = rng.choice([1, 2, 3, 7], size=n).astype(np.int32)
    S[rng.choice(n, size=T, replace=False)] = 0
    Y = (rng.choice(np.arange(0, C, 3), size=n) if classes == "spread" else np.full(n, classes)).astype(np.int32)
    rows, cls, ptr = li.lists(S, Y, 0, C)
    assert rows.size == T
    return dict(T=T, n=n, width=width, C=C, S=S, rows=rows, cls=cls, ptr=ptr,
                Z=rng.standard_normal((n, width), dtype=np.float32), E=rng.standard_normal((C, width), dtype=np.float32),
                G=rng.standard_normal((n, width), dtype=np.float32))


def run_device(ctx, c, thr, feed_all, seed, epoch, row0, pad=(), with_S=True, before_backward=None):
    """both entry points once through the C ABI with raw pointers; ``pad``: the operands among Z, E, G that get ld = m + 3
    and a base one float off alignment; ``before_backward``: called between the two (another user of the scratch).  Every
    buffer's guards are checked; returns Z, S_out, G_E and G_E of a second backward call."""
    lib, st = ctx.lib, ctx.stream(0)
    T, n, width, C = c["T"], c["n"], c["width"], c["C"]
    Z, E, G = _dense(n, width, "Z" in pad, c["Z"]), _dense(C, width, "E" in pad, c["E"]), _dense(n, width, "G" in pad, c["G"])
    S0 = np.where(c["S"] == 0, 9, c["S"]).astype(np.int32).reshape(n, 1)      # the listed rows start at a value nobody writes
    S_out = Guarded(n, 1, 1, 0, logical=S0) if with_S else None
    G_E, again = _dense(C, width, "G_E" in pad), _dense(C, width, "G_E" in pad)
    rows, cls, ptr = _int_tensor(c["rows"]), _int_tensor(c["cls"]), _int_tensor(c["ptr"])
    ctx.sync()
    lib.mggcn_label_input_forward_f32(st, rows.data_ptr(), cls.data_ptr(), T, E.ptr, E.ld, C, width, thr, int(feed_all), seed,
                                      epoch, row0, 0, li.FED_SET, Z.ptr, Z.ld, n, S_out.ptr if with_S else None)
    if before_backward is not None:
        before_backward()
    for out in (G_E, again):
        lib.mggcn_label_input_backward_f32(st, rows.data_ptr(), cls.data_ptr(), ptr.data_ptr(), T, C, width, thr,
                                           int(feed_all), seed, epoch, row0, G.ptr, G.ld, n, out.ptr, out.ld)
        if before_backward is not None:
            before_backward()
    ctx.sync()
    what = f"T={T} width={width} C={C} thr={thr} feed_all={feed_all} row0={row0} pad={pad}"
    for k, g in (("Z", Z), ("E", E), ("G", G), ("S_out", S_out), ("G_E", G_E), ("G_E again", again)):
        if g is not None:
            g.check_guards(f"{what} {k}")
    E.check_unchanged(f"{what} E")
    G.check_unchanged(f"{what} G")
    return dict(Z=Z.values(), S=None if S_out is None else S_out.logical_bits().view(np.int32).reshape(-1), S0=S0.reshape(-1),
                G_E=G_E.values(), again=again.values(), what=what)


def check_case(c, got, thr, feed_all, seed, epoch, row0):
    fed = li.fed_mask(c["rows"].astype(np.uint64) + np.uint64(row0), thr, seed, epoch, feed_all)
    want_Z, want_S = li.forward(c["Z"], got["S0"], c["E"], c["rows"], c["cls"], fed)
    np.testing.assert_array_equal(_bits(got["Z"]), _bits(want_Z), err_msg=got["what"])
    if got["S"] is not None:
        np.testing.assert_array_equal(got["S"], want_S, err_msg=got["what"])
    want, A, k = li.backward64(c["G"], c["rows"], c["cls"], fed, c["C"])
    err = np.abs(got["G_E"].astype(np.float64) - want)
    bound = li.gamma(k)[:, None] * A
    assert (err <= bound).all(), (got["what"], float((err - bound).max()))
    empty = k == 0
    np.testing.assert_array_equal(_bits(got["G_E"][empty]), 0, err_msg=got["what"])          # +0.0, written
    np.testing.assert_array_equal(_bits(got["again"]), _bits(got["G_E"]), err_msg=got["what"])
    return fed


# ---- the two kernels against the restatement ----------------------------------------------------------------------------------------------
CLASSES = [(1, 0), (3, 1), (41, "spread"), (256, "spread")]    # (class count, who owns the rows); 3: class 1 owns them all
MASKS = [(0, False), (li.threshold(0.5), False), (li.threshold(0.999), False), (0, True)]


@pytest.mark.parametrize("width", [1, 5, 41, 128, 384])
def test_both_kernels_against_the_restatement(ctx, width):
    """T around the chunk length, every class layout, threshold 0 / mid-range / nearly 1 and feed_all, row0 = 0 and above
    2^32, on aligned operands (the float4 path where width % 4 == 0): Z and S_out bit for bit, G_E within the bound"""
    seen = set()
    for T in T_SIZES:
        for C, classes in CLASSES:
            c = make_case(T, width, C, classes, seed=T + width + C)
            for mi, (thr, feed_all) in enumerate(MASKS):
                row0 = ROW0_FAR if (T + C + mi) % 2 else 0
                got = run_device(ctx, c, thr, feed_all, 0xC0FFEE123456789, 5, row0)
                fed = check_case(c, got, thr, feed_all, 0xC0FFEE123456789, 5, row0)
                seen.add((int(fed.sum()) > 0, int(fed.sum()) < T))
    assert seen == {(False, True), (True, True), (True, False), (False, False)}         # nothing, some, all fed; T = 0


@pytest.mark.parametrize("width", [128, 384])
@pytest.mark.parametrize("which", ["Z", "E", "G", "G_E"])
def test_a_misaligned_operand_takes_the_element_path(ctx, width, which):
    """each dense operand in turn at ld = width + 3, one float off alignment, in guarded buffers: the same bits in Z and
    S_out (the element path adds the same two numbers) and G_E within the bound, nothing outside the logical matrices"""
    thr = li.threshold(0.5)
    for T, (C, classes) in ((2 * L + 1, CLASSES[1]), (L + 1, CLASSES[2])):
        c = make_case(T, width, C, classes, seed=width + T)
        base = run_device(ctx, c, thr, False, 3, 1, ROW0_FAR)
        got = run_device(ctx, c, thr, False, 3, 1, ROW0_FAR, pad=(which,))
        check_case(c, got, thr, False, 3, 1, ROW0_FAR)
        np.testing.assert_array_equal(_bits(got["Z"]), _bits(base["Z"]))
        if which in ("Z", "E"):                                 # the backward took the path it took in ``base``
            np.testing.assert_array_equal(_bits(got["G_E"]), _bits(base["G_E"]))


def test_odd_widths_on_padded_operands_and_without_S_out(ctx):
    thr = li.threshold(0.3)
    for width in (1, 5, 41):
        c = make_case(L + 1, width, 3, 1, seed=width)
        got = run_device(ctx, c, thr, False, 8, 2, 0, pad=("Z", "E", "G", "G_E"), with_S=False)
        check_case(c, got, thr, False, 8, 2, 0)


def test_long_segments_and_many_waves(ctx):
    """5000 training rows: one class that owns them all (79 chunks: every slice of the final pass adds many partials) and
    41 classes with empty ones between; the forward takes 79 waves"""
    thr = li.threshold(0.5)
    for C, classes in ((3, 1), (41, "spread")):
        c = make_case(5000, 41, C, classes, seed=C)
        got = run_device(ctx, c, thr, False, 1, 0, ROW0_FAR)
        fed = check_case(c, got, thr, False, 1, 0, ROW0_FAR)
        assert 2300 < fed.sum() < 2700
        # the bound can see a missing chunk: G_E without the last 64 fed rows of a class is outside it
        last = np.flatnonzero(fed)[-L:]
        short = fed.copy()
        short[last] = False
        want, A, k = li.backward64(c["G"], c["rows"], c["cls"], fed, C)
        less, _, _ = li.backward64(c["G"], c["rows"], c["cls"], short, C)
        assert (np.abs(less - want) > li.gamma(k)[:, None] * A).any()


def test_the_same_bits_after_another_kernel_used_the_scratch(pkg, ctx):
    """G_E is equal, bit for bit, whether or not the column-sum scratch was used (and grown) by an unrelated kernel --
    GATv2's att_grad over 3000 rows of width 512 -- between the calls"""
    P = pkg.dn_matrix.from_numpy(np.random.default_rng(0).standard_normal((3000, 512), dtype=np.float32))
    G_att = pkg.dn_matrix(1, 512)
    thr = li.threshold(0.5)
    c = make_case(2 * L + 1, 128, 3, 1, seed=12)
    quiet = run_device(ctx, c, thr, False, 4, 4, 0)
    noisy = run_device(ctx, c, thr, False, 4, 4, 0, before_backward=lambda: pkg.ops.gatv2_att_grad(ctx, P, G_att, None))
    check_case(c, noisy, thr, False, 4, 4, 0)
    np.testing.assert_array_equal(_bits(noisy["G_E"]), _bits(quiet["G_E"]))
    np.testing.assert_array_equal(_bits(noisy["again"]), _bits(quiet["G_E"]))


def test_the_mask_depends_on_the_global_row_alone(ctx):
    """a rank of a row partition draws the single-GPU bits: rows [a, n) as a call of their own with row0 = a give the Z and
    S_out rows of the whole call"""
    thr, width, C = li.threshold(0.5), 41, 3
    c = make_case(2 * L + 1, width, C, "spread", seed=4)
    whole = run_device(ctx, c, thr, False, 6, 3, 1000)
    a = 50
    keep = c["rows"] >= a
    part = dict(c, n=c["n"] - a, T=int(keep.sum()), S=c["S"][a:], Z=c["Z"][a:], G=c["G"][a:], rows=c["rows"][keep] - a,
                cls=c["cls"][keep])
    part["ptr"] = np.searchsorted(part["cls"], np.arange(C + 1)).astype(np.int32)
    got = run_device(ctx, part, thr, False, 6, 3, 1000 + a)
    np.testing.assert_array_equal(_bits(got["Z"]), _bits(whole["Z"][a:]))
    np.testing.assert_array_equal(got["S"], whole["S"][a:])


# ---- the model ------------------------------------------------------------------------------------------------------------------------------
N, SIZES, HEADS, C = 600, [16, 32, 5], 4, 5
ZW = {"v1": 1, "v2": 2, "dot": 3}


@pytest.fixture(scope="module")
def data():
    ip, ix, dv, _ = li.planted_partition(N, C, 8, 0.7, seed=21)
    rng = np.random.default_rng(22)
    X = rng.standard_normal((N, SIZES[0]), dtype=np.float32)
    Y = rng.integers(0, C, size=(N, 1)).astype(np.int32)
    S = rng.choice(4, size=N, p=(0.5, 0.2, 0.25, 0.05)).astype(np.int32)
    return (ip, ix, dv), X, Y, S


def _gat(pkg, csr, sizes, **kw):
    ip, ix, dv = csr
    return pkg.gat(pkg.csr_matrix(ip.copy(), ix.copy(), dv.copy(), N), sizes, heads=HEADS, **kw)


def _label_model(pkg, data, variant, rate=0.5, seed=77, epoch=0, **kw):
    csr, X, Y, S = data
    G = _gat(pkg, csr, SIZES, variant=variant, label_input=rate, **kw)
    G.set_splits(S)
    G.set_label_input(pkg.dn_matrix.from_numpy(Y), seed=seed, epoch=epoch)
    return G


def _weights_of(G, E=None):
    """the weights= list that rebuilds G's layers; with ``E`` layer 0's W becomes [W ; E]"""
    out = []
    for li_, l in enumerate(G.layers()):
        W = l.W().numpy()
        if li_ == 0 and E is not None:
            W = np.concatenate([W, E], axis=0)
        out.append((W, l.b().numpy()) + (() if l.attn.att is None else (l.attn.att.numpy(),)))
    return out


def _augmented(pkg, data, G, **kw):
    """a plain gat on sizes[0] + C features whose first W is [W ; E] of ``G``"""
    csr = data[0]
    return _gat(pkg, csr, [SIZES[0] + C] + SIZES[1:], variant=G.variant, weights=_weights_of(G, G.label.E.numpy()), **kw)


@pytest.mark.parametrize("variant", ["v1", "v2", "dot"])
def test_a_zero_table_gives_the_plain_logits(pkg, ctx, data, variant):
    csr, X, Y, S = data
    zw = ZW[variant] * SIZES[1]
    G = _gat(pkg, csr, SIZES, variant=variant, label_input=0.5, label_weights=np.zeros((C, zw), dtype=np.float32))
    G.set_splits(S)
    G.set_label_input(Y.reshape(-1))                          # a host array of n integers is taken too
    P = _gat(pkg, csr, SIZES, variant=variant)
    assert G.layers()[0].label is G.label and G.label.E.shape() == (C, zw) and P.label is None
    assert (G.label_input_p, G.label_seed, G.label_epoch) == (0.5, 0, 0)
    Xd = pkg.dn_matrix.from_numpy(X)
    a, b = G(ctx, Xd), P(ctx, Xd)
    ctx.sync()
    np.testing.assert_array_equal(a.numpy(), b.numpy())
    np.testing.assert_array_equal(G.predict(ctx, Xd), P.predict(ctx, Xd))
    assert G.label_epoch == 0                                 # neither was a training forward


CASES = [("v1", {}), ("v2", {}), ("dot", {}), ("dot", dict(skip="gate", norm="layer", dropout=0.5)),
         ("v1", dict(skip="add", dropout=0.3, attn_dropout=0.3))]


@pytest.mark.parametrize("variant,options", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_one_epoch_agrees_with_the_augmented_model(pkg, ctx, data, variant, options):
    """train_forward + backward of gat(label_input=0.5) at training forward 3 against a second gat built on
    [X | M onehot(y)], [W ; E] and set_splits(S_e): loss at TOL, the score within 3 / the rows it is taken over, every
    gradient at TOL -- G_E against the last C rows of the augmented G_W --, and the counts of that epoch"""
    csr, X, Y, S = data
    seed, epoch = 0xABCDEF0123, 3
    G = _label_model(pkg, data, variant, seed=seed, epoch=epoch, **options)
    A = _augmented(pkg, data, G, **options)
    if options:
        for m in (G, A):
            m.set_dropout(options.get("dropout", 0.0), seed=5, epoch=2, attn=options.get("attn_dropout", 0.0))
        for lg, la in zip(G.layers(), A.layers()):           # the skip's own tensors: the linear's first weight sees H only
            if lg.res_lin is not None and lg is not G.layers()[0]:
                la.res_lin.W.init(lg.res_lin.W.numpy())
    M, S_e = li.epoch_sets(S, 0, li.threshold(0.5), seed, epoch)
    assert 100 < M.sum() < 200
    if options.get("skip") is not None:                       # res_lin of layer 0 reads the augmented H there: zero rows for it
        W_r = G.layers()[0].res_lin.W.numpy()
        A.layers()[0].res_lin.W.init(np.concatenate([W_r, np.zeros((C, W_r.shape[1]), dtype=np.float32)], axis=0))
    A.set_splits(S_e)
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    Xa = pkg.dn_matrix.from_numpy(li.augmented_features(X, Y, M, C))
    loss, acc = G.train_forward(ctx, Xd, Yd)
    G.backward(ctx)
    la, aa = A.train_forward(ctx, Xa, Yd)
    A.backward(ctx)
    ctx.sync()
    assert G.label_epoch == epoch + 1
    counts = li.counts(S_e)
    assert G.split_metrics()["counts"] == counts == A.split_metrics()["counts"]
    print(f"[label-input] {variant} {options}: loss {loss!r} (augmented {la!r}), score {acc!r} ({aa!r})")
    assert abs(loss - la) <= TOL * abs(la) and abs(acc - aa) <= 3.0 / counts["train"]
    for name in ("val", "test", "other"):
        g, a = G.split_metrics()[name], A.split_metrics()[name]
        assert abs(g[0] - a[0]) <= TOL * abs(a[0]) and abs(g[1] - a[1]) <= 3.0 / counts[name], name
    F = SIZES[0]
    g0, a0 = G.layers()[0], A.layers()[0]
    pairs = [("G_W0", g0.GW().numpy(), a0.GW().numpy()[:F]), ("G_E", G.label.G_E.numpy(), a0.GW().numpy()[F:]),
             ("G_b0", g0.Gb().numpy(), a0.Gb().numpy())]
    for k in (1,):
        pairs += [(f"G_W{k}", G.layers()[k].GW().numpy(), A.layers()[k].GW().numpy())]
    if g0.attn.att is not None:
        pairs.append(("G_att0", g0.Gatt().numpy(), a0.Gatt().numpy()))
    if g0.res_lin is not None:
        pairs.append(("G_W_r0", g0.res_lin.G_W.numpy(), a0.res_lin.G_W.numpy()[:F]))
    for name, a, b in pairs:
        d = relerr(a, b)
        print(f"[label-input] {variant} {options} {name}: {d:.3e}")
        assert np.abs(b).max() > 0 and d <= TOL, (name, d)


@pytest.mark.parametrize("variant", ["v1", "v2", "dot"])
def test_a_plain_call_feeds_every_training_row(pkg, ctx, data, variant):
    """a plain call, evaluate() and predict() against the augmented model on [X | onehot(y) of every training row]"""
    csr, X, Y, S = data
    G = _label_model(pkg, data, variant)
    A = _augmented(pkg, data, G)
    M, _ = li.epoch_sets(S, 0, 0, 0, 0, feed_all=True)
    assert M.sum() == (S == 0).sum()
    Xd, Yd, Sd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y), pkg.dn_matrix.from_numpy(S.reshape(-1, 1))
    Xa = pkg.dn_matrix.from_numpy(li.augmented_features(X, Y, M, C))
    a, b = G(ctx, Xd), A(ctx, Xa)
    ctx.sync()
    la, lb = a.numpy(), b.numpy()
    d = relerr(la, lb)
    print(f"[label-input] {variant} plain call against the augmented model: {d:.3e}")
    assert d <= TOL
    res = G.evaluate(ctx, Xd, Yd, Sd)
    hit = la.argmax(axis=1) == Y.reshape(-1)
    assert res["all"] == float(hit.mean()) and res["val"] == float(hit[S == 1].mean())
    np.testing.assert_array_equal(G.predict(ctx, Xd).reshape(-1), la.argmax(axis=1))
    assert G.label_epoch == 0
    # a training forward afterwards, then a plain one again: the splits of the loss layer are set_splits' own again
    G.train_forward(ctx, Xd, Yd)
    assert G.split_metrics()["counts"]["other"] > int((S == 3).sum())
    G.loss_layer(ctx, G(ctx, Xd), Yd)
    assert G.split_metrics()["counts"] == li.counts(S)


def _state_bits(G):
    out = []
    for l in G.layers():
        for p in l.params():
            for t in p.adam_tensors(0.0):
                out += [x.numpy().view(np.uint32).copy() for x in t[:4]]
    return out


def _three_steps(pkg, ctx, data, variant, fused, **kw):
    _, X, Y, _ = data
    G = _label_model(pkg, data, variant, fused=fused, **kw)
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    res = [G.train_step(ctx, Xd, Yd, *ADAM) for _ in range(3)]
    return res, _state_bits(G), G


@pytest.mark.parametrize("variant", ["v1", "dot"])
def test_three_steps_twice_give_the_same_bits(pkg, ctx, data, variant):
    """two runs of three train_steps, and fused=False against fused=True: the same losses and the same bits in every
    parameter, gradient and Adam moment, E included; E is a row of Adam's table and moves"""
    res, bits, G = _three_steps(pkg, ctx, data, variant, True)
    assert G.layers()[0].params()[-1] is G.label and all(l.label is None for l in G.layers()[1:])
    assert len(bits) == 4 * (2 * (3 if variant == "v1" else 2) + 1)
    for fused in (True, False):
        res2, bits2, G2 = _three_steps(pkg, ctx, data, variant, fused)
        assert res2 == res, fused
        for a, b in zip(bits, bits2):
            np.testing.assert_array_equal(a, b)
    assert G.label_epoch == 3 and G.label.step == 3
    E0 = _label_model(pkg, data, variant).label.E.numpy()
    assert np.abs(G.label.E.numpy() - E0).max() > 1e-3
    assert len({r[0] for r in res}) == 3


def test_replay_by_epoch(pkg, ctx, data):
    """set_label_input(Y, seed, epoch=e) replays training forward e: the same loss bits, the same counts, other masks in
    other epochs"""
    _, X, Y, S = data
    G = _label_model(pkg, data, "dot", seed=9)
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    runs = []
    for e in range(3):
        runs.append((G.train_forward(ctx, Xd, Yd), G.split_metrics()["counts"]))
        assert runs[-1][1] == li.counts(li.epoch_sets(S, 0, li.threshold(0.5), 9, e)[1])
    assert len({r[0][0] for r in runs}) == 3
    G.set_label_input(Yd, seed=9, epoch=1)
    assert G.label_epoch == 1 and G.label_input_p == 0.5
    assert (G.train_forward(ctx, Xd, Yd), G.split_metrics()["counts"]) == runs[1]
    G.set_label_input(Yd, rate=0.25, seed=9, epoch=1)
    assert G.label_input_p == 0.25
    G.train_forward(ctx, Xd, Yd)
    assert G.split_metrics()["counts"] == li.counts(li.epoch_sets(S, 0, li.threshold(0.25), 9, 1)[1])
    # new splits rebuild the lists: another training set, the same labels
    S2 = np.roll(S, 7)
    G.set_splits(S2)
    G.set_label_input(Yd, rate=0.5, seed=9, epoch=0)
    G.train_forward(ctx, Xd, Yd)
    assert G.split_metrics()["counts"] == li.counts(li.epoch_sets(S2, 0, li.threshold(0.5), 9, 0)[1])
    G.set_splits(S)                                            # ... and without a new set_label_input too
    G.train_forward(ctx, Xd, Yd)
    assert G.split_metrics()["counts"] == li.counts(li.epoch_sets(S, 0, li.threshold(0.5), 9, 1)[1])


def test_selector_restores_the_table(pkg, ctx, data, tmp_path):
    """model_selector.restore brings back the best epoch's parameters, E included; save, load and save_best raise and leave
    the directory empty"""
    _, X, Y, _ = data
    G = _label_model(pkg, data, "v1")                          # ("dot" is refused for its own reason first)
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    sel = pkg.model_selector(G, split="val", metric="loss", clean=False)
    names = [name for name, _ in sel._params()]
    assert names == ["W0", "b0", "att0", "label0", "W1", "b1", "att1"]
    snaps = []
    for _ in range(4):
        snaps.append({name: t.numpy().view(np.uint32).copy() for name, t in sel._params()})
        sel.step(ctx, Xd, Yd, 0.5 if len(snaps) > 2 else 1e-2, *ADAM[1:])
    assert sel.best_epoch is not None
    sel.restore(ctx)
    for name, t in sel._params():
        np.testing.assert_array_equal(t.numpy().view(np.uint32), snaps[sel.best_epoch][name], err_msg=name)
    assert G.label.step == 0 and not G.label.m.numpy().any()
    path = str(tmp_path / "model.ckpt")
    for call in (lambda: G.save(ctx, path), lambda: G.load(ctx, path), lambda: sel.save_best(ctx, path)):
        with pytest.raises(ValueError, match="label_input"):
            call()
    assert not list(tmp_path.iterdir())


@pytest.mark.parametrize("variant", ["v1", "v2", "dot"])
def test_defaults_are_what_they_were(pkg, data, variant):
    """label_input=0.0 spelled out, next to a label-input model: the timers, the parameters and the bits of a model built
    without the arguments; the label-input model registers its two timers in layer 0 alone"""
    csr, X, Y, _ = data
    runs = []
    for kw in ({}, dict(label_input=0.0, label_weights=None)):
        c = pkg.context(0)
        other = _label_model(pkg, data, variant)
        G = _gat(pkg, csr, SIZES, variant=variant, **kw)
        Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
        other.train_step(pkg.context(0), Xd, Yd, *ADAM)
        res = [G.train_step(c, Xd, Yd, *ADAM) for _ in range(2)]
        for l in G.layers():
            assert l.params() == ([l.lin] if variant == "dot" else [l.lin, l.attn]) and l.label is None
        assert G.label is None and G.label_input_p == 0.0 and "label" not in vars(G)
        bits = [t.numpy().view(np.uint32).copy() for l in G.layers() for p in l.params() for t, *_ in p.adam_tensors(0.0)]
        runs.append((res, sorted(c.timers), bits))
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    assert not any("label" in t for t in runs[0][1])
    for a, b in zip(runs[0][2], runs[1][2]):
        np.testing.assert_array_equal(a, b)
    c = pkg.context(0)
    _label_model(pkg, data, variant).train_step(c, pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y), *ADAM)
    assert sorted(t for t in c.timers if "label" in t) == ["0_0_label-input", "0_1_label-input"]


def test_label_inputs_learn_what_the_plain_model_cannot(pkg, ctx):
    """The planted-partition fixture of label_input_ref (noise features, the neighbours' labels determine the class): after
    60 epochs gat(variant="dot", label_input=0.5) must reach a validation accuracy above LEARN_BARS["label"] = 0.75 and the
    plain model must stay below LEARN_BARS["plain"] = 0.55.  The reference alone on the CPU gives 0.950 and 0.346
    (LEARN_REFERENCE; test_label_input_cpu.py measures them)."""
    k = li.LEARN
    (ip, ix, dv), X, Y, S = li.learning_case()
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    Sd = pkg.dn_matrix.from_numpy(S.reshape(-1, 1))
    got = {}
    for name, kw in (("plain", {}), ("label", dict(label_input=k["rate"]))):
        G = pkg.gat(pkg.csr_matrix(ip.copy(), ix.copy(), dv.copy(), k["n"]), [k["features"], k["hidden"], k["classes"]],
                    heads=k["heads"], variant="dot", **kw)
        G.set_splits(S)
        if kw:
            G.set_label_input(Yd, seed=k["label_seed"])
        for _ in range(k["epochs"]):
            G.train_step(ctx, Xd, Yd, *ADAM)
        got[name] = G.evaluate(ctx, Xd, Yd, Sd)["val"]
    print(f"[label-input] validation accuracy: {got} (reference {li.LEARN_REFERENCE})")
    assert got["label"] >= li.LEARN_BARS["label"], got
    assert got["plain"] <= li.LEARN_BARS["plain"], got
