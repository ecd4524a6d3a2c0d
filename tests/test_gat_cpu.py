"""The host references of the GAT tests, checked without a GPU: the fp64 restatement (gat_ref.restate64) against torch's
autograd in fp64, the fp32 twin against the restatement on the inputs the device tests use, and the option checks of the
gat constructor, which come before any device work."""
import numpy as np
import pytest

import gat_ref as ref


@pytest.fixture(scope="module")
def graph():
    return ref.kernel_graph()


def _autograd(indptr, indices, Z, att, K, G, slope):
    import torch
    n, d = indptr.size - 1, Z.shape[1]
    dh = d // K
    rows = torch.from_numpy(np.repeat(np.arange(n), np.diff(indptr.astype(np.int64))))
    cols = torch.from_numpy(indices.astype(np.int64))
    Zt = torch.tensor(Z, dtype=torch.float64, requires_grad=True)
    at = torch.tensor(att, dtype=torch.float64, requires_grad=True)
    Z3, a3 = Zt.view(-1, K, dh), at.view(2, K, dh)
    s_dst, s_src = (Z3 * a3[0]).sum(-1), (Z3 * a3[1]).sum(-1)
    e = torch.nn.functional.leaky_relu(s_dst[rows] + s_src[cols], slope)
    p = torch.exp(e)                                   # |score| <~ 10 on these inputs: no max to subtract
    alpha = p / torch.zeros(n, K, dtype=torch.float64).index_add(0, rows, p)[rows]
    out = torch.zeros(n, K, dh, dtype=torch.float64).index_add(0, rows, alpha[:, :, None] * Z3[cols]).view(n, d)
    out.backward(torch.tensor(G, dtype=torch.float64))
    return out.detach().numpy(), Zt.grad.numpy(), at.grad.numpy()


@pytest.mark.parametrize("K,dh", [(3, 7), (4, 8), (1, 5)])
def test_restatement_matches_autograd(graph, K, dh):
    """out, G_Z and G_att of the fp64 restatement against torch CPU autograd in fp64, on the kernel-test graph (empty rows,
    one entry, 64 / 65 / 1000 / 4097 entries, a duplicated column, an unreferenced column): <= 1e-12"""
    indptr, indices = graph
    Z, _, G, att = ref.tolerance_inputs(320, 320, K, dh)
    r = ref.restate64(indptr, indices, Z, att, K, G=G, exact=True)
    out, G_Z, G_att = _autograd(indptr, indices, Z, att, K, G, ref.SLOPE)
    for what, got, want in (("out", r["out"], out), ("G_Z", r["G_Z"], G_Z), ("G_att", r["G_att"], G_att)):
        d = ref.relerr(got, want)
        print(f"[gat] restatement against autograd K={K} dh={dh} {what}: {d:.3e}")
        assert d <= 1e-12, (what, d)


@pytest.mark.parametrize("K,dh", [(1, 1), (5, 1), (3, 7), (1, 41), (4, 32), (2, 65), (1, 128), (8, 32), (16, 64)])
def test_twin_is_close_to_the_restatement(graph, K, dh):
    """on the tolerance inputs the fp32 twin is within 1e-5 of the restatement in every output; if it is not, the input is
    at fault, not a kernel"""
    indptr, indices = graph
    Z, _, G, att = ref.tolerance_inputs(320, 320, K, dh)
    want = ref.restate64(indptr, indices, Z, att, K, G=G)
    twin = ref.twin32(indptr, indices, Z, att, K, G=G)
    for what in ref.NAMES:
        d = ref.relerr(twin[what], want[what])
        print(f"[gat] twin against restatement K={K} dh={dh} {what}: {d:.3e}")
        assert d <= 1e-5, ("the input is ill-conditioned for the device tests' bar", what, d)


def test_rectangular_restatement_leaves_the_destination_term_out():
    """200 destinations x 320 sources: G_Z has one row per source and no ds_dst term; G_att[0] sums over destinations"""
    indptr, indices = ref.kernel_graph(200, 320)
    Z, Z_dst, G, att = ref.tolerance_inputs(200, 320, 4, 32)
    r = ref.restate64(indptr, indices, Z, att, 4, G=G, Z_dst=Z_dst, exact=True)
    assert r["G_Z"].shape == (320, 128) and r["ds_dst"].shape == (200, 4) and r["ds_src"].shape == (320, 4)
    want = (r["ds_src"][ref.UNREFERENCED][:, None] * att.astype(np.float64).reshape(2, 4, 32)[1]).reshape(-1)
    np.testing.assert_array_equal(r["G_Z"][ref.UNREFERENCED], want)          # ds_src of an unreferenced column is 0
    assert not r["G_Z"][ref.UNREFERENCED].any()


def test_attention_with_zero_att_is_the_row_mean(graph):
    indptr, indices = graph
    Z, _, _, att = ref.tolerance_inputs(320, 320, 4, 8)
    r = ref.restate64(indptr, indices, Z, np.zeros_like(att), 4, exact=True)
    assert ref.relerr(r["out"], ref.row_mean(indptr, indices, Z)) <= 1e-14


@pytest.mark.parametrize("sizes,heads,what", [
    ([16, 30, 5], 4, "not divisible"),             # 30 columns into 4 heads
    ([16, 32, 6], [4, 4], "not divisible"),        # the last layer's 6 into 4
    ([16, 34, 5], 17, "heads"),                    # more than 16 heads
    ([16, 32, 5], 0, "heads"),
    ([16, 2048, 5], 8, "1024"),                    # wider than the kernels take
    ([16, 32, 5], [4], "lists"),                   # one entry for two layers
    ([16, 32, 5], 2.5, "heads"),
])
def test_constructor_refusals_need_no_gpu(pkg, sizes, heads, what):
    n = 8
    A = pkg.csr_matrix(np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32), np.ones(n, dtype=np.float32), n)
    with pytest.raises(ValueError, match=what):
        pkg.gat(A, sizes, heads=heads)


def test_constructor_refuses_an_unknown_loss_and_a_rectangular_matrix(pkg):
    n = 8
    A = pkg.csr_matrix(np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32), np.ones(n, dtype=np.float32), n)
    with pytest.raises(ValueError, match="loss"):
        pkg.gat(A, [16, 32, 5], loss="hinge")
    R = pkg.csr_matrix(np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32), np.ones(n, dtype=np.float32), n + 3)
    with pytest.raises(ValueError, match="square"):
        pkg.gat(R, [16, 32, 5])


def test_heads_default_gives_the_last_layer_one_head(pkg):
    from importlib import import_module
    gat = import_module(pkg.__name__ + ".gat")
    assert gat.check_heads([16, 32, 32, 7], 4) == [4, 4, 1]
    assert gat.check_heads([16, 32, 32, 8], [2, 4, 8]) == [2, 4, 8]
