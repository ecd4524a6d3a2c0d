"""GraphSAGE without a GPU: the numpy restatement (tests/sage_ref.py) against torch autograd on the CPU in fp64, the refusals
of sage(...) and of the ops wrappers (before any device work: the context is None), and the ABI's two new entries."""
import os
import re

import numpy as np
import pytest

import sage_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _graph(n=60, seed=1):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 9, size=n)
    lens[3] = 0
    indptr = np.concatenate(([0], np.cumsum(lens))).astype(np.uint32)
    indices = rng.integers(0, n, size=int(indptr[-1])).astype(np.uint32)       # unsorted, duplicates happen
    data = rng.random(int(indptr[-1])).astype(np.float32)
    return indptr, indices, data, n


# ---- the selection ------------------------------------------------------------------------------------------------------------
def test_agg_max_is_the_amax_of_torch_with_the_smallest_index_on_ties():
    import torch
    indptr, indices, _, n = _graph()
    rng = np.random.default_rng(2)
    B = rng.choice(np.array([-2, -1, -0.0, 0.0, 1, 2], dtype=np.float64), size=(n, 5))
    out, arg = ref.agg_max(indptr, indices, B)
    for i in range(n):
        js = np.unique(indices[indptr[i]:indptr[i + 1]])
        if js.size == 0:
            assert (arg[i] == ref.NONE).all() and not np.signbit(out[i]).any() and (out[i] == 0).all()
            continue
        want = torch.amax(torch.from_numpy(B[js]), dim=0).numpy()
        assert (out[i] == want).all()
        for c in range(5):
            assert arg[i, c] == js[B[js, c] == want[c]].min()                  # -0.0 == +0.0: the smaller j
            assert out[i, c].tobytes() == B[arg[i, c], c].tobytes()            # the winner's bits


def test_agg_max_order_nan_inf_duplicates_and_src0():
    indptr = np.array([0, 4, 6, 8, 8, 11], dtype=np.uint32)
    indices = np.array([3, 1, 3, 2, 0, 4, 4, 4, 2, 1, 0], dtype=np.uint32)
    B = np.array([[np.nan, np.nan], [-0.0, 1.0], [0.0, -np.inf], [0.0, np.nan], [-np.inf, np.nan]], dtype=np.float32)
    out, arg = ref.agg_max(indptr, indices, B, src0=100)
    assert arg.tolist() == [[101, 101], [104, ref.NONE], [104, ref.NONE], [ref.NONE, ref.NONE], [101, 101]]
    assert np.signbit(out[0, 0]) and out[0, 1] == 1.0                          # -0.0 of j = 1 beats +0.0 of j = 2, 3
    assert out[1, 0] == -np.inf and out[1, 1] == 0 and not np.signbit(out[1, 1])    # a row of NaNs only: +0.0 and NONE
    assert (out[3] == 0).all() and not np.signbit(out[3]).any()
    # the order of the entries and duplicates do not matter
    perm = np.array([2, 3, 0, 1, 5, 4, 7, 6, 10, 8, 9])
    out2, arg2 = ref.agg_max(indptr, indices[perm], B, src0=100)
    assert out2.tobytes() == out.tobytes() and (arg2 == arg).all()


def test_agg_max_backward_is_the_autograd_of_the_gather_and_skips_adjacent_duplicates():
    import torch
    indptr, indices, _, n = _graph(seed=4)
    rng = np.random.default_rng(5)
    B = rng.standard_normal((n, 6))
    G = rng.standard_normal((n, 6))
    out, arg = ref.agg_max(indptr, indices, B)
    t_indptr, t_indices = ref.transpose_pattern(indptr, indices, n)
    assert any((np.diff(t_indices[t_indptr[j]:t_indptr[j + 1]].astype(np.int64)) == 0).any() for j in range(n)), "no duplicate pair"
    got = ref.agg_max_backward(t_indptr, t_indices, arg, G, n)
    Bt = torch.from_numpy(B).requires_grad_()
    idx = torch.from_numpy(np.where(arg == ref.NONE, 0, arg).astype(np.int64))
    M = torch.where(torch.from_numpy(arg == ref.NONE), torch.zeros((), dtype=torch.float64), Bt.gather(0, idx))
    assert (M.detach().numpy() == out).all()
    M.backward(torch.from_numpy(G))
    want = Bt.grad.numpy()
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(ref.scatter_arg(G, arg, n) - want).max() <= 1e-12 * np.abs(want).max()


# ---- the model ------------------------------------------------------------------------------------------------------------------
def _torch_sage(F, sizes, weights, aggr, norm, loss, masks, X, Y, args):
    """the model with torch autograd in fp64: the same formulas written independently, the selection given"""
    import torch
    indptr, indices, data = F
    n = len(indptr) - 1
    rows = torch.from_numpy(np.repeat(np.arange(n), np.diff(indptr.astype(np.int64))))
    cols = torch.from_numpy(indices.astype(np.int64))
    vals = torch.from_numpy(data.astype(np.float64))
    params = [[torch.from_numpy(np.asarray(w, dtype=np.float64)).clone().requires_grad_() for w in ws] for ws in weights]
    L = len(sizes) - 1
    norms = [[torch.ones(1, sizes[l + 1], dtype=torch.float64, requires_grad=True),
              torch.zeros(1, sizes[l + 1], dtype=torch.float64, requires_grad=True)] if norm and l + 1 < L else None
             for l in range(L)]
    H = torch.from_numpy(np.asarray(X, dtype=np.float64))
    for l in range(L):
        if masks[l] is not None:
            keep, scale = masks[l]
            H = torch.where(torch.from_numpy(keep), H * float(scale), torch.zeros((), dtype=torch.float64))
        if aggr == "mean":
            M = torch.zeros(n, H.shape[1], dtype=torch.float64).index_add(0, rows, vals[:, None] * H[cols])
        else:
            a = np.asarray(args[l]).astype(np.int64) & 0xFFFFFFFF
            none = torch.from_numpy(a == ref.NONE)
            M = torch.where(none, torch.zeros((), dtype=torch.float64), H.gather(0, torch.from_numpy(np.where(a == ref.NONE, 0, a))))
        W_l, b_l, W_r, b_r = params[l]
        Z = M @ W_l + b_l + H @ W_r + b_r
        if l + 1 < L:
            if norms[l] is not None:
                Z = torch.nn.functional.layer_norm(Z, (Z.shape[1],), norms[l][0][0], norms[l][1][0], ref.EPS)
            Z = torch.nn.functional.leaky_relu(Z, ref.SLOPE)
        H = Z
    if loss == "bce":
        val = torch.nn.functional.binary_cross_entropy_with_logits(H, torch.from_numpy((Y != 0).astype(np.float64)))
    else:
        val = torch.nn.functional.cross_entropy(H, torch.from_numpy(Y.reshape(-1).astype(np.int64)))
    val.backward()
    return float(val.detach()), H.detach().numpy(), params, norms


@pytest.mark.parametrize("aggr", ["mean", "max"])
@pytest.mark.parametrize("norm,loss,drop", [(None, "softmax", False), ("layer", "softmax", False), (None, "bce", True),
                                            ("layer", "bce", True)])
def test_restatement_against_autograd_fp64(aggr, norm, loss, drop):
    indptr, indices, data, n = _graph(seed=8)
    sizes = [9, 12, 10, 4]
    rng = np.random.default_rng(3)
    X = rng.standard_normal((n, sizes[0]))
    Y = rng.integers(0, 2, size=(n, sizes[-1])) if loss == "bce" else rng.integers(0, sizes[-1], size=(n, 1))
    weights = ref.init_weights(sizes)
    masks = [None] + [((rng.random((n, w)) >= 0.5), np.float32(2.0)) if drop else None for w in sizes[1:-1]]
    R = ref.Sage((indptr, indices, data), sizes, weights, aggr, np.float64, norm=norm, loss=loss, masks=masks)
    got_loss = R.train_forward(X, Y)
    grads = R.backward()
    want_loss, logits, params, norms = _torch_sage((indptr, indices, data), sizes, weights, aggr, norm, loss, masks, X, Y, R.args)
    assert abs(got_loss - want_loss) <= 1e-12 * abs(want_loss)
    assert np.abs(R.logits - logits).max() <= 1e-12 * np.abs(logits).max()

    def close(got, want, what):
        want = want.grad.numpy().reshape(got.shape)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), what
    for l, g in enumerate(grads):
        for k, name in enumerate(("W_l", "b_l", "W_r", "b_r")):
            close(g[name], params[l][k], (l, name))
        if norms[l] is not None:
            close(g["gamma"], norms[l][0], (l, "gamma"))
            close(g["beta"], norms[l][1], (l, "beta"))
    if aggr == "max":                                    # the model's own selection is agg_max on each layer's input
        for l in range(len(sizes) - 1):
            assert (R.args[l] == ref.agg_max(indptr, indices, R.tape[l]["H"])[1]).all()


# ---- the package ------------------------------------------------------------------------------------------------------------------
def test_exports(pkg):
    for name in ("sage", "sage_layer", "max_aggregate"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    assert callable(pkg.ops.agg_max_forward) and callable(pkg.ops.agg_max_backward)
    assert pkg.ops.AGG_NONE == 0xFFFFFFFF and pkg.ops.AGG_ACCUMULATE == 1


def test_both_entries_are_declared_and_bound(pkg):
    text = open(os.path.join(ROOT, "include", "mggcn.h")).read()
    lib = pkg._lib.load()
    for name in ("mggcn_agg_max_forward_f32", "mggcn_agg_max_backward_f32"):
        assert re.search(r"\bvoid %s\s*\(" % name, text), name
        assert name in pkg._lib.PROTOTYPES and hasattr(lib, name)
    assert re.search(r"#define MGGCN_AGG_ACCUMULATE 1u", text) and re.search(r"#define MGGCN_AGG_NONE 0xFFFFFFFFu", text)
    assert len(pkg._lib.PROTOTYPES["mggcn_agg_max_forward_f32"][1]) == 13
    assert len(pkg._lib.PROTOTYPES["mggcn_agg_max_backward_f32"][1]) == 14


def _csr(pkg, n=6, m=None):
    indptr, indices, data, _ = _graph(n=n, seed=1)
    return pkg.csr_matrix(indptr, indices % (m or n), data, m or n)


@pytest.mark.parametrize("kw,word", [(dict(aggr="sum"), "aggr"), (dict(aggr=None), "aggr"), (dict(norm="batch"), "norm"),
                                     (dict(loss="hinge"), "loss"), (dict(dropout=1.0), "dropout"),
                                     (dict(dropout=-0.1), "dropout")])
def test_sage_refuses_options_before_any_device_work(pkg, kw, word):
    A = _csr(pkg)
    before = A.data.copy()
    with pytest.raises(ValueError, match=word):
        pkg.sage(A, [4, 3, 2], **kw)
    assert (A.data == before).all() and A._dev is None


def test_sage_refuses_a_matrix_that_is_not_square(pkg):
    with pytest.raises(ValueError, match="square"):
        pkg.sage(_csr(pkg, 6, 7), [4, 3, 2])


def test_sage_refuses_checkpoints_and_creates_nothing(pkg, tmp_path):
    model = object.__new__(pkg.sage)                    # the members refuse before they look at the model or the context
    path = tmp_path / "model.ckpt"
    with pytest.raises(ValueError, match="sage"):
        model.save(None, str(path))
    with pytest.raises(ValueError, match="sage"):
        model.load(None, str(path))
    with pytest.raises(ValueError, match="sage"):
        model._write_checkpoint(None, str(path), {}, False, 0)       # what model_selector.save_best calls
    assert not path.exists() and list(tmp_path.iterdir()) == []
    with pytest.raises(pkg.datasets.format_error):
        pkg.datasets.write_checkpoint(str(path), dict(sizes=[4, 2], model="sage"), {})
    assert not path.exists()


def _dn(pkg, n, m, dtype=np.float32):
    return pkg.dn_matrix(n, m, dtype=dtype, device="cpu")


def test_ops_wrappers_refuse_before_the_library(pkg):
    ops = pkg.ops
    F = _csr(pkg, 6)
    B, out, arg = _dn(pkg, 6, 8), _dn(pkg, 6, 8), _dn(pkg, 6, 8, np.int32)
    cases = [
        (ops.agg_max_forward, (F, _dn(pkg, 5, 8), out), {}, "shape"),
        (ops.agg_max_forward, (F, B, _dn(pkg, 6, 7)), {}, "shape"),
        (ops.agg_max_forward, (F, _dn(pkg, 6, 1025), _dn(pkg, 6, 1025)), {}, "width"),
        (ops.agg_max_forward, (F, _dn(pkg, 6, 0), _dn(pkg, 6, 0)), {}, "width"),
        (ops.agg_max_forward, (F, B, out, _dn(pkg, 6, 8)), {}, "arg"),                  # fp32
        (ops.agg_max_forward, (F, B, out, _dn(pkg, 6, 4, np.int32)), {}, "arg"),
        (ops.agg_max_forward, (F, B, B), {}, "alias"),
        (ops.agg_max_forward, (F, B, out, arg), dict(src0=0xFFFFFFFF), "src0"),
        (ops.agg_max_backward, (F, arg, _dn(pkg, 5, 8), out), {}, "shape"),
        (ops.agg_max_backward, (F, arg, B, _dn(pkg, 6, 7)), {}, "shape"),
        (ops.agg_max_backward, (F, _dn(pkg, 6, 1025, np.int32), _dn(pkg, 6, 1025), _dn(pkg, 6, 1025)), {}, "width"),
        (ops.agg_max_backward, (F, _dn(pkg, 6, 8), B, out), {}, "arg"),
        (ops.agg_max_backward, (F, None, B, out), {}, "arg"),
        (ops.agg_max_backward, (F, arg, B, B), {}, "alias"),
    ]
    for fn, args, kw, word in cases:
        with pytest.raises(ValueError, match=word):
            fn(None, *args, **kw)
    assert F._dev is None
