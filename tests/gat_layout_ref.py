"""The attention kernels on independently padded, guarded operands (test_gpu_gat_layouts.py, test_gat_layouts_cpu.py): the
small rectangular graph, the layout table that gives every dense operand of a chain its own leading dimension and offset,
the guard-sizing rule, a restatement of the host-side choice of the kernel variant, the checks (a)-(d) on guarded buffers,
and a numpy model of the addressing that the CPU tests run with named mutations to show that those checks have teeth.

Three families: "gat" (mggcn_gat_*), "gat-drop" (the _drop twins at p = 0.5 with gat_dropout_ref's seed and stream) and
"gatv2" (mggcn_gatv2_*).  One operand naming for all three: Zs is the source transform (GAT's Z), Zd the destination
transform (GAT's Z_dst: the block is rectangular), G_Zs the gradient of Zs (GAT's G_Z); ds_src_r / G_Zs_r are what the
packed-record form of backward_src writes, in buffers of their own with the layout of ds_src / G_Zs."""
import numpy as np

import dropout_ref
import gat_alpha_ref as ar
import gat_dropout_ref as dr
import gat_ref as ref
import gatv2_ref as v2
from guarded import IN_NAN32, OUT_NAN32, Guarded

# ---- the graph ---------------------------------------------------------------------------------------------------------------------------
N_DST, N_SRC = 37, 53               # both = 1 mod 4: the last workgroup (four rows) of F and of F^T holds one row
ROW_LENS = {0: 1, 1: 2, 2: 63, 3: 64, 4: 65, 5: 129, 34: 0, 36: 200}
DUPLICATE_ROW = 6
UNREFERENCED = ref.UNREFERENCED     # a source nobody gathers: an empty row of F^T


def layout_graph(seed=17):
    """(indptr, indices) of the N_DST x N_SRC pattern: rows of ROW_LENS entries -- below, at and above one 64-entry chunk and
    past the two-chunk index prefetch, the empty row and the 200-entry row in the last four --, row 6 with one column twice,
    every other row of 1..8 entries; random columns, none of them UNREFERENCED"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 9, size=N_DST)
    for r, l in ROW_LENS.items():
        lens[r] = l
    lens[DUPLICATE_ROW] = 3
    allowed = np.array([c for c in range(N_SRC) if c != UNREFERENCED], dtype=np.uint32)
    indptr = np.zeros(N_DST + 1, dtype=np.uint32)
    indptr[1:] = np.cumsum(lens)
    indices = allowed[rng.integers(0, allowed.size, size=int(indptr[-1]))]
    b = int(indptr[DUPLICATE_ROW])
    indices[b + 1] = indices[b]
    return indptr, np.ascontiguousarray(indices, dtype=np.uint32)


# ---- families, shapes, operands ----------------------------------------------------------------------------------------------------------
FAMILIES = ("gat", "gat-drop", "gatv2")
# one (K, dh) per compiled (VEC, NT, U) variant on aligned operands, and (16, 4): K % 4 == 0 with one float4 per head, the
# 16-byte store form of mggcn_gat_alpha_f32 next to (4, 32)
SHAPES = {"gat": ref.EDGE_RECT + [(16, 4)], "gat-drop": ref.EDGE_RECT + [(16, 4)], "gatv2": v2.RECT_SHAPES + [(16, 4)]}
ONE_PADDED_SHAPE = (4, 32)
# The seed of gat_ref.tolerance_inputs / gatv2_ref.inputs, for all three families.  Their default (11) draws, at (1, 130), a
# row 15 whose only kept entry under the dropout mask has G . Z = -8e-4 against sum |G Z| = 83: D cancels to 1e-5 of its
# terms and the fp32 twin's ds_dst of that row is 1.1e-3 off on the row-scaled measure, above gat_dropout_ref.DROP_TOL.  That
# is the input, not a kernel (gat_dropout_ref explains the mechanism), so the input changes and the bar stays.
INPUT_SEED = 12
DROP_P = 0.5

# operand -> (rows, width, output): rows "dst" | "src" | "nnz" | a number, width "d" | "K" | "4K" | "2K"
_GAT_OPS = dict(Zs=("src", "d", False), Zd=("dst", "d", False), G=("dst", "d", False), att=(2, "d", False),
                s_dst=("dst", "K", True), s_src=("src", "K", True), out=("dst", "d", True), lse=("dst", "K", True),
                D=("dst", "K", True), ds_dst=("dst", "K", True), ds_src=("src", "K", True), G_Zs=("src", "d", True),
                rec=("dst", "4K", True), ds_src_r=("src", "K", True), G_Zs_r=("src", "d", True), G_att=(2, "d", True),
                alpha=("nnz", "K", True))
_V2_OPS = dict(Zs=("src", "d", False), Zd=("dst", "d", False), G=("dst", "d", False), att=(1, "d", False),
               out=("dst", "d", True), lse=("dst", "K", True), D=("dst", "K", True), G_Zd=("dst", "d", True), P=("dst", "d", True),
               G_att=(1, "d", True), G_Zs=("src", "d", True), rec=("dst", "2K", True), G_Zs_r=("src", "d", True),
               alpha=("nnz", "K", True))
OPERANDS = {"gat": _GAT_OPS, "gat-drop": _GAT_OPS, "gatv2": _V2_OPS}
LAYOUT_OF = dict(ds_src_r="ds_src", G_Zs_r="G_Zs")      # the record form's outputs take the plain form's layout
DENSE = ("Zs", "Zd", "G", "out", "G_Zs", "G_Zd", "P", "alpha")     # operands with a leading dimension argument
FLAT = ("att", "G_att", "s_dst", "s_src", "lse", "D", "ds_dst", "ds_src", "rec")     # contiguous by the ABI: an offset only


def dense_operands(family):
    return [k for k in DENSE if k in OPERANDS[family]]


# ---- the layout table ----------------------------------------------------------------------------------------------------------------------
def _row(pads=None, offs=None):
    pads, offs = pads or {}, offs or {}
    assert set(pads) <= set(DENSE) and set(offs) <= set(DENSE + FLAT)
    return {k: (pads.get(k, 0), offs.get(k, 0)) for k in DENSE + FLAT}


# layout -> operand -> (ld - width, offset) in floats.  alpha's pad "vec" is resolved with K: lda = K rounded up to a multiple
# of 4, plus 4.  rec must stay 16-byte (GAT) / 8-byte (GATv2) aligned: its offsets are multiples of 4 and, in "off-base", the
# smallest offset that keeps the alignment (4 floats / 2 floats, see rec_offset).
LAYOUTS = {
    "contiguous": _row(),
    "vec-padded": _row(dict(Zs=4, Zd=8, G=12, out=16, G_Zs=20, G_Zd=24, P=28, alpha="vec"),
                       dict(Zs=4, Zd=8, G=12, out=16, G_Zs=20, G_Zd=24, P=28, alpha=32, att=36, G_att=40, s_dst=4, s_src=8, lse=12,
                            D=16, ds_dst=20, ds_src=24, rec=4)),
    "odd-ld": _row(dict(Zs=1, Zd=3, G=5, out=7, G_Zs=9, G_Zd=11, P=13, alpha=1)),
    "off-base": _row(dict(Zs=4, Zd=8, G=0, out=12, G_Zs=16, G_Zd=20, P=24, alpha=4),
                     dict(Zs=1, Zd=2, G=3, out=1, G_Zs=2, G_Zd=3, P=1, alpha=1, att=2, G_att=3, s_dst=1, s_src=2, lse=3, D=1,
                          ds_dst=2, ds_src=3, rec="rec")),
    # GATv2's model layout with unequal partners: Zs | Zd and G_Zs | G_Zd are the halves of one [rows x 2 K dh] buffer each
    # (plan() builds them), G, out and P each have another padded leading dimension
    "halves": _row(dict(G=4, out=8, P=12)),
}
for _x in DENSE:
    LAYOUTS[f"one-padded[{_x}]"] = _row({_x: 4})
TABLE = ("contiguous", "vec-padded", "odd-ld", "off-base")      # run at every shape; one-padded[X] at ONE_PADDED_SHAPE only


def one_padded(family):
    return [f"one-padded[{x}]" for x in dense_operands(family)]


def layouts_for(family, K, dh):
    return list(TABLE) + (one_padded(family) if (K, dh) == ONE_PADDED_SHAPE else [])


def rec_offset(family):
    return 2 if family == "gatv2" else 4


# ---- plans: every operand's place, with the guard-sizing rule ---------------------------------------------------------------------------------
class Place:
    """one operand: rows x cols at leading dimension ld, `off` floats past an aligned base, `tail_rows` guard rows behind;
    ``view`` = (buffer, first column) for a half of a wider buffer"""

    def __init__(self, rows, cols, ld, off, output, view=None):
        self.rows, self.cols, self.ld, self.off, self.output, self.view, self.tail_rows = rows, cols, ld, off, output, view, 1


def _width(w, K, dh):
    return {"d": K * dh, "K": K, "4K": 4 * K, "2K": 2 * K}[w]


def plan(family, K, dh, layout, nnz, n=N_DST, n_src=N_SRC):
    """operand -> Place for one (family, shape, layout).  The guard behind every buffer follows one rule: with ANY leading
    dimension of the chain used on ANY operand, and one row more than the operand has, every access stays inside the
    allocation -- at least rows x (largest ld - own ld) plus one row (guard_need)."""
    table = LAYOUTS[layout]
    rows_of = {"dst": n, "src": n_src, "nnz": nnz}
    p = {}
    for name, (rows, w, output) in OPERANDS[family].items():
        pad, off = table[LAYOUT_OF.get(name, name)]
        cols = _width(w, K, dh)
        if pad == "vec":
            pad = -(-K // 4) * 4 + 4 - K
        if off == "rec":
            off = rec_offset(family)
        p[name] = Place(rows_of.get(rows, rows), cols, cols + pad, off, output)
    if layout == "halves":
        assert family == "gatv2"
        d, big = K * dh, max(n, n_src)
        p["Z2"], p["G_Z2"] = Place(big, 2 * d, 2 * d, 0, False), Place(big, 2 * d, 2 * d, 0, True)
        for name, buf, half in (("Zs", "Z2", 0), ("Zd", "Z2", 1), ("G_Zs", "G_Z2", 0), ("G_Zd", "G_Z2", 1)):
            p[name] = Place(p[name].rows, d, 2 * d, 0, p[name].output, view=(buf, half * d))
        p["G_Zs_r"] = Place(n_src, d, 2 * d, 0, True)               # a buffer of its own at G_Zs's leading dimension
    for name, q in p.items():
        if q.view is None:
            q.tail_rows = -(-guard_need(p, name, nnz, n, n_src) // q.ld)
    return p


def largest_ld(p):
    return max(q.ld for q in p.values())


def guard_need(p, name, nnz, n=N_DST, n_src=N_SRC):
    """floats behind operand `name` that the rule asks for: row (most rows of its kind) walked with the largest leading
    dimension of the plan must still lie inside, whole"""
    q = p[name]
    most = nnz if name == "alpha" else max(n, n_src)
    return max((most + 1) * largest_ld(p) - q.rows * q.ld, q.ld)


def make_buffers(p, values, host=False):
    """operand -> Guarded (views: operand -> (Guarded, first column)).  Inputs hold ``values[name]`` with IN_NAN32 around
    them, outputs OUT_NAN32 everywhere"""
    bufs = {}
    for name, q in p.items():
        if q.view is None:
            bufs[name] = Guarded(q.rows, q.cols, q.ld, q.off, None if q.output else values[name], output=q.output,
                                 tail_rows=q.tail_rows, host=host)
    return bufs


def halves_values(c, K, dh):
    """Z2 of the "halves" layout as bit patterns: [Zs | Zd], IN_NAN32 where Zd has no row"""
    d = K * dh
    Z2 = np.full((max(c["n"], c["n_src"]), 2 * d), IN_NAN32, dtype=np.uint32)
    Z2[:c["n_src"], :d] = c["Zs"].view(np.uint32)
    Z2[:c["n"], d:] = c["Zd"].view(np.uint32)
    return Z2


# ---- which kernel a call reaches: csrc/gat_internal.h rows16, head_geometry_for and gat_dispatch restated -------------------------------------
def rows16(q):
    """aligned16(pointer) && ld % 4 == 0; the allocations are 256-byte aligned and the front guard is a multiple of 64 floats"""
    col0 = q.view[1] if q.view else 0
    return (q.off + col0) % 4 == 0 and q.ld % 4 == 0


def aligned16(q):
    return q.off % 4 == 0


# family -> call -> (operands whose leading dimension the call takes, operands that decide float4 / element, whether att's
# alignment decides too, outputs, the calls whose outputs it reads).  "one" in the place of the deciders: a single form.
_GAT_CALLS = {
    "scores": (("Zs", "Zd"), "one", False, ("s_dst", "s_src"), ()),
    "forward": (("Zs", "out"), ("Zs", "out"), False, ("out", "lse"), ("scores",)),
    "backward_dst": (("Zs", "G", "out"), ("Zs", "G", "out"), False, ("D", "ds_dst"), ("forward",)),
    "backward_src": (("Zs", "G", "G_Zs"), ("Zs", "G", "G_Zs"), True, ("ds_src", "G_Zs"), ("backward_dst",)),
    "pack_dst": ((), "one", False, ("rec",), ("backward_dst",)),
    "backward_src_rec": (("Zs", "G", "G_Zs_r"), ("Zs", "G", "G_Zs_r"), True, ("ds_src_r", "G_Zs_r"), ("pack_dst",)),
    "scores_backward": (("Zd", "Zs"), "one", False, ("G_att",), ("backward_src",)),
    "alpha": (("alpha",), "alpha", False, ("alpha",), ("forward",)),
}
_V2_CALLS = {
    "forward": (("Zs", "Zd", "out"), ("Zs", "Zd", "out"), True, ("out", "lse"), ()),
    "backward_dst": (("Zs", "Zd", "G", "out", "G_Zd", "P"), ("Zs", "Zd", "G", "out", "G_Zd", "P"), True, ("D", "G_Zd", "P"),
                     ("forward",)),
    "att_grad": (("P",), "one", False, ("G_att",), ("backward_dst",)),
    "backward_src": (("Zs", "Zd", "G", "G_Zs"), ("Zs", "Zd", "G", "G_Zs"), True, ("G_Zs",), ("backward_dst",)),
    "pack_dst": ((), "one", False, ("rec",), ("backward_dst",)),
    "backward_src_rec": (("Zs", "Zd", "G", "G_Zs_r"), ("Zs", "Zd", "G", "G_Zs_r"), True, ("G_Zs_r",), ("pack_dst",)),
    "alpha": (("Zs", "Zd", "alpha"), ("Zs", "Zd"), True, ("alpha",), ("forward",)),
}
CALLS = {"gat": _GAT_CALLS, "gat-drop": _GAT_CALLS, "gatv2": _V2_CALLS}
SPARSE = ("forward", "backward_dst", "backward_src", "backward_src_rec")      # the calls that go through gat_dispatch
VARIANTS = ((4, 1, 4), (4, 4, 1), (1, 1, 4), (1, 4, 2), (1, 16, 1))


def classify(family, call, K, dh, p):
    """the form `call` takes on the operands of plan p: "one" (a single kernel), ("KV", 4 | 1) for mggcn_gat_alpha_f32, or the
    (VEC, NT, U) of gat_dispatch"""
    _, deciders, with_att, _, _ = CALLS[family][call]
    if deciders == "one":
        return "one"
    if deciders == "alpha":
        return ("KV", 4 if K % 4 == 0 and rows16(p["alpha"]) else 1)
    vec = dh % 4 == 0 and all(rows16(p[x]) for x in deciders) and (not with_att or aligned16(p["att"]))
    return ref.head_geometry_for(dh, vec)[0]


def same_bits_as_contiguous(family, K, dh, p, p0):
    """call -> whether its outputs must carry the contiguous run's bits: it takes the variant it takes there, and so does
    every call it reads from.  The bits of mggcn_gat_alpha_f32 do not depend on its store form (one value per entry and
    head, no sum), so for that call the calls it reads from decide alone."""
    same = {}
    for call, (_, deciders, _, _, deps) in CALLS[family].items():            # in the order of the chain
        own = deciders == "alpha" or classify(family, call, K, dh, p) == classify(family, call, K, dh, p0)
        same[call] = own and all(same[x] for x in deps)
    return same


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
_cases = {}


def case(family, K, dh):
    """the graph, the inputs, the exact restatement with its row scales, the fp32 twin, and the exact alpha with its c_p
    (gat_alpha_ref's measure); computed once per process and left unchanged by everyone who reads it"""
    key = (family, K, dh)
    if key in _cases:
        return _cases[key]
    indptr, indices = layout_graph()
    t_indptr, t_indices = ref.transpose_pattern(indptr, indices, N_SRC)
    c = dict(indptr=indptr, indices=indices, t_indptr=t_indptr, t_indices=t_indices, n=N_DST, n_src=N_SRC, nnz=indices.size)
    if family == "gatv2":
        Zs, Zd, G, att = v2.inputs(N_DST, N_SRC, K, dh, seed=INPUT_SEED)
        c["want"] = v2.restate64(indptr, indices, Zs, Zd, att, K, G=G, exact=True, scales=True)
        c["twin"] = v2.twin32(indptr, indices, Zs, Zd, att, K, G=G)
        c["cp"] = ar.cp_v2(indptr, ar.alpha_v2(indptr, indices, Zs, Zd, att, K)["mag"], c["want"]["lse"])
        c["bar"] = dict(v2.BAR)
    else:
        Zs, Zd, G, att = ref.tolerance_inputs(N_DST, N_SRC, K, dh, seed=INPUT_SEED, att_scale=0.1 * min(1.0, (32.0 / dh) ** 0.5))
        if family == "gat-drop":
            c["keep"] = dr.keep_mask(indptr, indices, K, DROP_P, dr.SEED, dr.STREAM)
            c["qscale"] = dropout_ref.params(DROP_P)[1]
            c["drop"] = dr.drop_tuple(DROP_P, dr.SEED, dr.STREAM)
            a = (indptr, indices, Zs, att, K, c["keep"], c["qscale"])
            c["want"] = dr.restate64(*a, G=G, Z_dst=Zd, exact=True, scales=True)
            c["twin"] = dr.twin32(*a, G=G, Z_dst=Zd)
            sc = c["want"]["scale"]
            # G_att has no bar of its own under dropout: it is the column sum of ds x Z, so an error of ds within its bar
            # moves it by at most that bar times sum |ds scale| |Z| -- the scale below -- plus the sum's own rounding
            sc["s_dst"], sc["s_src"] = (np.abs(x.reshape(-1, K, dh) * y.reshape(K, dh)).sum(axis=2)
                                        for x, y in ((Zd.astype(np.float64), att[0]), (Zs.astype(np.float64), att[1])))
            sc["G_att"] = np.stack([(np.repeat(sc["ds_dst"], dh, axis=1) * np.abs(Zd)).sum(axis=0),
                                    (np.repeat(sc["ds_src"], dh, axis=1) * np.abs(Zs)).sum(axis=0)])
            c["bar"] = dict(dr.DROP_TOL, s_dst=ref.ROW_TOL, s_src=ref.ROW_TOL,
                            G_att=max(dr.DROP_TOL["ds_dst"], dr.DROP_TOL["ds_src"]) + ref.ROW_TOL)
        else:
            c["want"] = ref.restate64(indptr, indices, Zs, att, K, G=G, Z_dst=Zd, exact=True, scales=True)
            c["twin"] = ref.twin32(indptr, indices, Zs, att, K, G=G, Z_dst=Zd)
            c["bar"] = dict.fromkeys(ref.NAMES, ref.ROW_TOL)
        w = c["want"]
        c["cp"] = ar.cp_v1(indptr, indices, w["s_dst"], w["s_src"], w["lse"])
    c.update(Zs=Zs, Zd=Zd, G=G, att=att, scale=c["want"]["scale"], alpha=c["want"]["alpha"])
    _cases[key] = c
    return c


RESULT = dict(G_Zs="G_Z")           # operand -> its name in gat_ref's / gat_dropout_ref's results


def result_name(family, name):
    return name if family == "gatv2" else RESULT.get(name, name)


def compared(family):
    """the operands held against the restatement on the row-scaled measure (alpha has its own, rec and the record form's
    outputs are held against the plain form's bits)"""
    return [k for k, (_, _, output) in OPERANDS[family].items() if output and k not in ("rec", "ds_src_r", "G_Zs_r", "alpha")]


# The fp32 twins on THIS graph: worst rowdist from the exact restatement per family and output over SHAPES[family], and the
# worst distance of the twin's alpha on gat_alpha_ref's measure, as test_gat_layouts_cpu.py measures them (it prints and
# asserts them).  Each stays within an eighth of its bar (gatv2_ref.bar_rule), so the bars of the families stand as they are.
TWIN_MEASURED = {
    "gat": dict(s_dst=1.26e-07, s_src=1.37e-07, out=3.70e-07, lse=1.45e-07, D=9.99e-07, ds_dst=4.59e-07, ds_src=5.52e-07,
                G_Zs=5.42e-07, G_att=9.12e-08, alpha=2.09e-07),
    "gat-drop": dict(s_dst=1.26e-07, s_src=1.37e-07, out=4.04e-07, lse=1.45e-07, D=5.62e-07, ds_dst=9.41e-06, ds_src=8.64e-07,
                     G_Zs=7.38e-07, G_att=1.39e-07, alpha=2.09e-07),
    "gatv2": dict(out=2.77e-07, lse=1.58e-07, D=6.67e-07, G_Zd=1.15e-06, P=1.22e-06, G_att=2.43e-07, G_Zs=5.67e-07, alpha=1.96e-07),
}


def twin_errors(family, K, dh):
    """operand -> (the twin's worst rowdist, its bar), and alpha on gat_alpha_ref's measure"""
    c = case(family, K, dh)
    res = {}
    for name in compared(family):
        rn = result_name(family, name)
        res[name] = (ref.rowerr(c["twin"][rn], c["want"][rn], c["scale"][rn])[1], c["bar"][rn])
    res["alpha"] = (ar.check(c["twin"]["alpha"], c["alpha"], c["cp"])[0], ar.BAR)
    return res


# ---- the checks (a)-(d) ------------------------------------------------------------------------------------------------------------------------
def violations(bufs, p):
    """[(check, operand, message)] over guarded buffers after a chain: (a) an output changed outside its logical window,
    (b) an input buffer changed, (c) a logical output element still holds OUT_NAN32, (d) a logical output element that was
    written is not finite.  A buffer's ``mask`` is its logical window (the caller may have narrowed it)."""
    found = []
    for name, g in bufs.items():
        bits = g.bits()
        if not p[name].output:
            try:
                g.check_unchanged(name)
            except AssertionError as e:
                found.append(("b", name, str(e)))
            continue
        try:
            g.check_guards(name, bits)
        except AssertionError as e:
            found.append(("a", name, str(e)))
        logical = bits[g.mask]
        left = logical == OUT_NAN32
        if left.any():
            found.append(("c", name, f"{name}: {int(left.sum())} logical element(s) never written"))
        bad = ~np.isfinite(logical.view(np.float32)) & ~left
        if bad.any():
            found.append(("d", name, f"{name}: {int(bad.sum())} logical element(s) not finite"))
    return found


def input_values(family, c):
    return {k: c[k] for k in ("Zs", "Zd", "G", "att")}


# ---- the numpy model of the addressing -----------------------------------------------------------------------------------------------------------
def _load(g, ld=None):
    """the matrix a kernel reads through base + r ld + c; an index outside the buffer raises (the guard-sizing rule)"""
    idx = g.start + np.arange(g.rows)[:, None] * (g.ld if ld is None else ld) + np.arange(g.cols)[None, :]
    return g.host[idx].view(np.float32)


def _store(g, vals, ld=None, row0=0, col0=0):
    vals = np.ascontiguousarray(vals, dtype=np.float32)
    idx = g.start + (row0 + np.arange(vals.shape[0]))[:, None] * (g.ld if ld is None else ld) + col0 + np.arange(vals.shape[1])
    g.host[idx] = vals.view(np.uint32)


MUTATIONS = ("G walked with ldz", "out stored with ldz", "a float4 that straddles the last column", "a store for row n_rows",
             "lse for the fifth row of the last workgroup", "alpha stored at column K")


def run_model(family, K, dh, layout, mutation=None):
    """the whole chain of one family on host-side guarded buffers: every input is gathered and every output scattered through
    its own base, leading dimension and offset, the arithmetic between them is the family's fp64 restatement.  ``mutation``
    (one of MUTATIONS) is an addressing mistake a kernel could make.  Returns (buffers, plan)."""
    assert (mutation is None or mutation in MUTATIONS) and layout != "halves"
    c = case(family, K, dh)
    p = plan(family, K, dh, layout, c["nnz"])
    b = make_buffers(p, input_values(family, c), host=True)
    indptr, indices, n = c["indptr"], c["indices"], c["n"]
    Zs, Zd, att = _load(b["Zs"]), _load(b["Zd"]), _load(b["att"])
    G = _load(b["G"], b["Zs"].ld if mutation == "G walked with ldz" else None)
    with np.errstate(all="ignore"):
        if family == "gatv2":
            r = v2.restate64(indptr, indices, Zs, Zd, att, K, G=G)
            r["rec"] = np.stack([r["lse"], r["D"]], axis=2).reshape(n, 2 * K)
        else:
            if family == "gat-drop":
                r = dr.restate64(indptr, indices, Zs, att, K, c["keep"], c["qscale"], G=G, Z_dst=Zd)
            else:
                r = ref.restate64(indptr, indices, Zs, att, K, G=G, Z_dst=Zd)
            r["rec"] = np.stack([r["s_dst"], r["lse"], r["D"], np.zeros_like(r["D"])], axis=2).reshape(n, 4 * K)
            r["ds_src_r"] = r["ds_src"]
    r["G_Zs_r"] = r[result_name(family, "G_Zs")]
    for name, q in p.items():
        if q.output:
            _store(b[name], r[result_name(family, name)], b["Zs"].ld if (name, mutation) == ("out", "out stored with ldz") else None)
    if mutation == "a float4 that straddles the last column":
        _store(b["out"], r["out"][:, -2:], col0=K * dh)
    elif mutation == "a store for row n_rows":
        _store(b["out"], r["out"][-1:], row0=n)
    elif mutation == "lse for the fifth row of the last workgroup":
        _store(b["lse"], r["lse"][-1:], row0=4 * ((n - 1) // 4) + 4)
    elif mutation == "alpha stored at column K":
        _store(b["alpha"], r["alpha"][:, :1], col0=K)
    return b, p
