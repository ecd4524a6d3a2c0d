"""The host references of the gat(edge_attr=E) tests, checked without a GPU: the fp64 restatement (gat_efeat_ref) against
torch's autograd in fp64 on a dense formulation of the same layer, the mutations the bars must tell apart, the host
permutation between the two copies of E, the bar of every output by the project's rule, the refusals of the option (all
before any device work), the default-off path, the ABI's prototypes and the register report of csrc/gat_efeat.hip."""
import inspect
import os
import re
import shutil
import subprocess
from importlib import import_module

import numpy as np
import pytest

import gat_efeat_ref as er
import gat_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the formula against autograd --------------------------------------------------------------------------------------------------
def _small_graph(n=40, seed=17):
    """a square pattern of 1..7 distinct entries per row, one row empty"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 8, size=n)
    lens[5] = 0
    indptr = np.zeros(n + 1, dtype=np.uint32)
    indptr[1:] = np.cumsum(lens)
    indices = np.concatenate([np.sort(rng.choice(n, size=int(l), replace=False)) for l in lens]).astype(np.uint32)
    return indptr, indices


def test_restatement_matches_autograd():
    """G_Z, G_att and G_U (and out) of the fp64 restatement against torch CPU autograd in fp64 on a DENSE formulation of the
    layer -- a masked softmax over an n x n x K score tensor with a dense [n x n x de] edge tensor --, n = 40, K = 3,
    de = 3, duplicates removed.  Both sides are fp64: 1e-9 of the largest element, anything else is a formula error."""
    import torch
    n, K, dh, de = 40, 3, 5, 3
    indptr, indices = _small_graph(n)
    rng = np.random.default_rng(3)
    Z, G = rng.standard_normal((n, K * dh)), rng.standard_normal((n, K * dh))
    att = 0.3 * rng.standard_normal((2, K * dh))
    E, U = 0.5 * rng.standard_normal((indices.size, de)), 0.4 * rng.standard_normal((K, de))
    r = er.attention(indptr, indices, Z, att, K, E, U, G=G, dtype=np.float64)

    rows = np.repeat(np.arange(n), np.diff(indptr.astype(np.int64)))
    cols = indices.astype(np.int64)
    mask = np.zeros((n, n), dtype=bool)
    mask[rows, cols] = True
    Ed = np.zeros((n, n, de))
    Ed[rows, cols] = E
    z, a, u = (torch.tensor(M, dtype=torch.float64, requires_grad=True) for M in (Z, att, U))
    z3, a3 = z.view(n, K, dh), a.view(2, K, dh)
    s_dst, s_src = (z3 * a3[0]).sum(-1), (z3 * a3[1]).sum(-1)
    x = s_dst[:, None, :] + s_src[None, :, :] + torch.tensor(Ed) @ u.T
    e = torch.nn.functional.leaky_relu(x, ref.SLOPE).masked_fill(~torch.tensor(mask)[:, :, None], -float("inf"))
    alpha = torch.nan_to_num(torch.softmax(e, dim=1), nan=0.0)          # the empty row: all -inf
    out = torch.einsum("ijk,jkd->ikd", alpha, z3).reshape(n, K * dh)
    (out * torch.tensor(G)).sum().backward()
    for what, got, want in (("out", r["out"], out.detach().numpy()), ("G_Z", r["G_Z"], z.grad.numpy()),
                            ("G_att", r["G_att"], a.grad.numpy()), ("G_U", r["G_U"], u.grad.numpy())):
        d = ref.relerr(got, want)
        print(f"[gat_efeat] restatement against autograd {what}: {d:.3e}")
        assert d <= 1e-9, (what, d)
    assert not r["out"][5].any() and not r["P_e"][5].any()


# ---- the mutations the bars must tell apart --------------------------------------------------------------------------------------------
def _mutant(case, **mut):
    c = er.efeat_case(*case)
    kw = dict(c["kw"])
    got = er.restate64(c["indptr"], c["indices"], c["Z"], c["att"], case[1], c["E"], c["U"], G=c["G"], Z_dst=c["Z_dst"], **kw,
                       **mut)
    return c, er.distances({k: got[k] for k in er.NAMES}, c)


def test_wrong_entry_order_of_the_transposed_copy_breaks_the_bar():
    """backward_src given E in F's entry order where it walks F^T: ds_src and G_Z leave their bars, the rest is untouched"""
    case = ("long", 4, 32, 8, None)
    c, d = _mutant(case, E_T=er.efeat_case(*case)["E"])
    print("[gat_efeat] E in the wrong order for the transposed walk:", {k: f"{v:.2e}" for k, v in d.items()})
    tol = er.EFEAT_TOL["plain"]
    assert d["ds_src"] > 10 * tol["ds_src"] and d["G_Z"] > 10 * tol["G_Z"]
    assert all(d[k] <= tol[k] for k in ("out", "lse", "D", "ds_dst", "P_e", "G_U"))


def test_one_heads_vector_for_every_head_breaks_the_bar():
    c, d = _mutant(("long", 4, 32, 8, None), head0_U=True)
    print("[gat_efeat] U[0] for every head:", {k: f"{v:.2e}" for k, v in d.items()})
    tol = er.EFEAT_TOL["plain"]
    assert all(d[k] > 10 * tol[k] for k in ("out", "ds_dst", "ds_src", "G_Z", "P_e"))


def test_P_e_without_q_breaks_the_bar():
    c, d = _mutant(("long", 4, 32, 8, 0.5), pe_without_q=True)
    print("[gat_efeat] P_e from a ds without q:", {k: f"{v:.2e}" for k, v in d.items()})
    tol = er.EFEAT_TOL["drop"]
    assert d["P_e"] > 10 * tol["P_e"] and d["G_U"] > 10 * tol["G_U"]
    assert all(d[k] <= tol[k] for k in ("out", "lse", "D", "ds_dst", "ds_src", "G_Z"))


# ---- the permutation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["long", "rect"])
def test_permutation_lines_up_with_the_transpose(pkg, graph):
    """E[perm] is E in the entry order of the transposed pattern, on kernel_graph_long (the duplicate row included) and on
    the rectangular block: against gat_ref.transpose_pattern, and against the library's own transpose, which carries the
    entry numbers in its values (exact in fp32 below 2^24)"""
    indptr, indices, n_src = ref.edge_graphs()[graph]
    n = indptr.size - 1
    perm = er.edge_perm(indices)
    assert sorted(perm.tolist()) == list(range(indices.size))
    rows = np.repeat(np.arange(n, dtype=np.uint32), np.diff(indptr.astype(np.int64)))
    t_indptr, t_indices = ref.transpose_pattern(indptr, indices, n_src)
    assert np.array_equal(t_indices, rows[perm])
    assert np.array_equal(indices[perm], np.repeat(np.arange(n_src, dtype=np.uint32), np.diff(t_indptr.astype(np.int64))))
    if graph == "long":
        b = int(indptr[ref.LONG_DUPLICATE_ROW])
        assert indices[b] == indices[b + 1]
        where = {int(p): q for q, p in enumerate(perm)}
        assert where[b] + 1 == where[b + 1]                 # the pair keeps its order: a consistent bijection
    assert indices.size < 1 << 24
    A = pkg.csr_matrix(indptr.copy(), indices.copy(), np.arange(indices.size, dtype=np.float32), n_src)
    gat = import_module(pkg.__name__ + ".gat")
    mine = gat.edge_permutation(A)
    assert np.array_equal(mine, perm)
    T = A.transpose()
    assert np.array_equal(T.indptr, t_indptr) and np.array_equal(T.indices, t_indices)
    assert np.array_equal(T.data.astype(np.int64), mine)


# ---- the bars --------------------------------------------------------------------------------------------------------------------------
def test_bars_follow_from_the_twin():
    """the fp32 twin's worst rowdist per mode and output over the device cases: it is what gat_efeat_ref records (within the
    rounding of three digits), and every bar is bar_rule of the record -- the floor where the twin is within an eighth of
    it, eight times the twin's worst rounded up otherwise"""
    worst = {md: dict.fromkeys(er.NAMES, 0.0) for md in ("plain", "drop")}
    for case in er.efeat_cases():
        c = er.efeat_case(*case)
        for k, v in er.distances({k: c["twin"][k] for k in er.NAMES}, c).items():
            worst[er.mode(case[-1])][k] = max(worst[er.mode(case[-1])][k], v)
    for md in worst:
        for k in er.NAMES:
            rec, bar = er.TWIN_EFEAT_MEASURED[md][k], er.EFEAT_TOL[md][k]
            print(f"[gat_efeat] twin {md} {k}: worst {worst[md][k]:.3e}, recorded {rec:.2e}, bar {bar:.1e}")
            assert worst[md][k] <= rec * 1.0001 and rec <= worst[md][k] * 1.02, (md, k, worst[md][k], rec)
            assert bar == er.bar_rule(rec, er.floor_of(md, k)), (md, k, bar)
            assert bar >= ref.ROW_TOL


def test_cases_cover_the_shapes():
    cases = er.efeat_cases()
    assert {c[0] for c in cases} == {"long", "longT", "rect"}
    assert {(K, dh) for _, K, dh, _, _ in cases} == set(er.EFEAT_SHAPES)
    for K, dh in er.EFEAT_CROSS:
        assert {de for _, k, d, de, _ in cases if (k, d) == (K, dh)} == {1, 3, 8, 16}
    assert {p for *_, p in cases} == {None, 0.5, 0.9}
    variants = {ref.head_geometry_for(dh, dh % 4 == 0)[0] for _, dh in er.EFEAT_SHAPES}
    assert variants == {(4, 1, 4), (1, 1, 4), (4, 4, 1), (1, 16, 1)}


# ---- the option ------------------------------------------------------------------------------------------------------------------------
def _tiny(pkg, n=8):
    return pkg.csr_matrix(np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32), np.ones(n, dtype=np.float32), n)


def test_constructor_refusals_need_no_gpu(pkg):
    """every refusal of the option through pkg.gat(None, ...): a ValueError naming edge_attr before the matrix is looked at"""
    E = np.zeros((8, 3), dtype=np.float32)
    sizes = [16, 32, 5]
    for variant in ("v2", "dot"):
        with pytest.raises(ValueError, match=r"edge_attr"):
            pkg.gat(None, sizes, variant=variant, edge_attr=E)
    with pytest.raises(ValueError, match=r"bf16.*edge_attr"):
        pkg.gat(None, sizes, agg_dtype="bf16", edge_attr=E)
    for bad in (np.zeros((8, 0)), np.zeros((8, 17)), np.zeros(8), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError, match=r"edge_attr"):
            pkg.gat(None, sizes, edge_attr=bad)
    for value in (np.nan, np.inf, -np.inf):
        bad = E.copy()
        bad[3, 1] = value
        with pytest.raises(ValueError, match=r"edge_attr.*not finite"):
            pkg.gat(None, sizes, edge_attr=bad)
    with pytest.raises(ValueError, match=r"edge_weights needs edge_attr"):
        pkg.gat(None, sizes, edge_weights=[np.zeros((4, 3)), np.zeros((1, 3))])
    with pytest.raises(ValueError, match=r"edge_weights.*edge_attr"):
        pkg.gat(None, sizes, edge_attr=E, edge_weights=[np.zeros((4, 3))])
    with pytest.raises(ValueError, match=r"edge_attr.*edge_weights of layer 1"):
        pkg.gat(None, sizes, edge_attr=E, edge_weights=[np.zeros((4, 3)), np.zeros((4, 3))])
    with pytest.raises(ValueError, match=r"edge_attr must have one row per entry of A, 8, got 7"):
        pkg.gat(_tiny(pkg), sizes, edge_attr=E[:7])
    shifted = pkg.csr_matrix(np.arange(1, 10, dtype=np.uint32), np.arange(8, dtype=np.uint32), np.ones(8, dtype=np.float32), 8)
    with pytest.raises(ValueError, match=r"edge_attr.*indptr begins with 0"):
        pkg.gat(shifted, sizes, edge_attr=E)


def test_dist_gat_does_not_take_the_arguments(pkg):
    dist = import_module(pkg.__name__ + ".dist")
    assert "edge_attr" not in inspect.signature(dist.dist_gat.__init__).parameters
    with pytest.raises(TypeError):
        dist.dist_gat(None, None, None, [16, 32, 5], edge_attr=np.zeros((8, 3)))


def test_export_and_checkpoints_are_refused(pkg, tmp_path):
    """attention_weights, gat_layer.alpha, save, load and the selector's save_best raise ValueError naming edge_attr with None
    in the place of the context; nothing is written, read or created"""
    gat = import_module(pkg.__name__ + ".gat")
    G = gat.gat.__new__(gat.gat)
    G.variant, G.edge_dim, G.layers_, G.heads = "v1", 3, [], [4, 1]
    with pytest.raises(ValueError, match="edge_attr"):
        G.attention_weights(None, None)
    layer = gat.gat_layer.__new__(gat.gat_layer)
    layer.name, layer.H = "0_", None
    layer.attn = gat.attention_efeat.__new__(gat.attention_efeat)
    layer.attn.edge_dim = 3
    with pytest.raises(ValueError, match="edge_attr"):
        layer.alpha(None)
    with pytest.raises(ValueError, match="edge_attr"):
        layer.attn.alpha(None, None, None, None)
    path = tmp_path / "model.ckpt"
    with pytest.raises(ValueError, match="edge_attr"):
        G.save(None, str(path))
    with pytest.raises(ValueError, match="edge_attr"):
        G.load(None, str(path))                            # refused before the (missing) file is opened
    with pytest.raises(ValueError, match="edge_attr"):
        G._write_checkpoint(None, str(path), {}, False, 0)
    assert not path.exists() and not list(tmp_path.iterdir())


def test_default_is_off(pkg):
    """edge_attr=None takes the code path that existed before: the check returns None whatever the other options are, the
    model's attributes read "no edge features", a layer builds the plain attention, and the plain attention's table and the
    prototypes of the existing entry points are what they were"""
    gat = import_module(pkg.__name__ + ".gat")
    for variant in gat.VARIANTS:
        for agg in ("f32", "bf16"):
            assert gat.check_edge_attr(None, None, variant, agg, 2) is None
    assert gat.gat.edge_dim == 0 and gat.gat.E_A is None and gat.gat.E_F is None and gat.gat.P_e_buffer is None
    sig = inspect.signature(gat.gat.__init__).parameters
    assert sig["edge_attr"].default is None and sig["edge_weights"].default is None
    assert inspect.signature(gat.gat_layer.__init__).parameters["edge"].default is None
    assert gat.attention.params_table == (("att", "att", "G_att", "m", "v", True),)
    assert [row[0] for row in gat.attention_efeat.params_table] == ["att", "att_edge"]
    assert gat.attention_efeat.params_table[1] == ("att_edge", "att_edge", "G_att_edge", "m_edge", "v_edge", True)
    protos = pkg._lib.PROTOTYPES
    assert len(protos["mggcn_gat_forward_f32"][1]) == 15 and len(protos["mggcn_gat_backward_dst_f32"][1]) == 19
    assert len(protos["mggcn_gat_backward_src_f32"][1]) == 21


def test_abi_lists_the_six_entry_points(pkg):
    """each efeat entry: its twin's list plus (E, lde, att_edge, de), and (P_e, ldp) on backward_dst"""
    protos, ops = pkg._lib.PROTOTYPES, pkg.ops
    for name, more in (("forward", 4), ("backward_dst", 6), ("backward_src", 4)):
        for drop in ("", "_drop"):
            twin = protos[f"mggcn_gat_{name}{drop}_f32"][1]
            mine = protos[f"mggcn_gat_{name}_efeat{drop}_f32"][1]
            assert mine[:len(twin)] == twin and len(mine) == len(twin) + more, (name, drop)
    assert ops.GAT_MAX_EDGE_DIM == 16
    header = open(os.path.join(ROOT, "include", "mggcn.h")).read()
    assert "#define MGGCN_GAT_MAX_EDGE_DIM 16u" in header
    for name in ("forward", "backward_dst", "backward_src"):
        for drop in ("", "_drop"):
            assert f"void mggcn_gat_{name}_efeat{drop}_f32(" in header


def test_ops_refuse_bad_shapes_before_the_library(pkg):
    """the wrappers raise ValueError on stand-ins that own no device memory"""
    class M:
        def __init__(self, n, m): self.N, self.Mm = n, m
        def n(self): return self.N
        def m(self): return self.Mm
        def shape(self): return (self.N, self.Mm)
        def nnz(self): return 20
        def buffer(self): return 0
    ops = pkg.ops
    F, Z, s, o = M(8, 8), M(8, 32), M(8, 4), M(8, 32)
    with pytest.raises(ValueError, match="edge dimension"):
        ops.gat_forward_efeat(None, F, Z, s, s, o, s, M(20, 17), M(4, 17), 4)
    with pytest.raises(ValueError, match="one row per entry"):
        ops.gat_forward_efeat(None, F, Z, s, s, o, s, M(19, 3), M(4, 3), 4)
    with pytest.raises(ValueError, match="att_edge"):
        ops.gat_forward_efeat(None, F, Z, s, s, o, s, M(20, 3), M(1, 3), 4)
    with pytest.raises(ValueError, match="P_e"):
        ops.gat_backward_dst_efeat(None, F, Z, s, s, s, o, o, s, s, M(20, 3), M(4, 3), M(8, 3), 4)
    with pytest.raises(ValueError, match="att_edge"):
        ops.gat_backward_src_efeat(None, F, Z, s, s, s, s, o, M(2, 32), s, s, o, M(20, 3), M(3, 3), 4)


GAT_KERNELS = ("gat_forward_kernel", "gat_backward_dst_kernel", "gat_backward_src_kernel")


def test_no_instantiation_uses_scratch(tmp_path):
    """csrc/gat_efeat.hip compiled for gfx950 to assembly: the resource metadata of all thirty instantiations -- the three
    kernels of gat_kernels.h with the edge term, which their mangled names carry as the type gat_edge, x gat_dispatch's five
    (VEC, NT, U) x DROP -- reports a private segment of zero bytes and no spilled vector register (backward_dst holds
    sixteen P_e slots per lane on top of the plain kernel's state); the file instantiates none of the three without it"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path / "gat_efeat.s"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-S",
                        "--cuda-device-only", os.path.join(ROOT, "mg-gcn_amd", "csrc", "gat_efeat.hip"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels"):]
    seen = {}
    for b in re.split(r"\n\s*- \.agpr_count:", "\n" + meta)[1:]:
        blk = ".agpr_count:" + b
        nm = re.search(r"\.name:\s+(\S+)", blk)
        if not nm or not any(kernel in nm.group(1) for kernel in GAT_KERNELS):
            continue
        assert "gat_edge" in nm.group(1), nm.group(1)
        field = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                 for k in ("private_segment_fixed_size", "vgpr_spill_count", "vgpr_count", "agpr_count")}
        seen[nm.group(1)] = field
        print(f"[gat_efeat.hip] {nm.group(1)}: {field}")
        assert field["private_segment_fixed_size"] == 0 and field["vgpr_spill_count"] == 0, (nm.group(1), field)
    assert len(seen) == 30, sorted(seen)
    for kernel in GAT_KERNELS:
        assert sum(kernel in k for k in seen) == 10, (kernel, sorted(seen))


def test_the_file_defines_no_kernel():
    """csrc/gat_efeat.hip holds entry points and the check of their edge operands: every kernel it launches is a template of
    gat_kernels.h, the one the plain entry points instantiate"""
    text = open(os.path.join(ROOT, "mg-gcn_amd", "csrc", "gat_efeat.hip")).read()
    assert "__global__" not in text
    assert '#include "gat_kernels.h"' in text
