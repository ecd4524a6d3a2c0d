"""The row-partitioned GATv2 attention on the host, for the dist_gat(variant="v2") tests: the algebra of
mg-gcn_amd/dist_gat.py (dist_attention_v2) restated in numpy on gatv2_ref.attention_v2.  Every "rank" function sees only its
rows of Z2 = [Zs | Zd] and of G, its row blocks of F and F^T (global columns) and the arrays a collective delivers (Z2_all,
G_all, and lse / D of all destinations); the driver partitioned() plays the collectives by concatenation.  Also the packed
(lse, D) record of mggcn_gatv2_pack_dst_f32 in numpy, the four mutations the device tests must be able to see, and the bytes
a rank hands to the exchange."""
import numpy as np

import gat_ref as ref
import gatv2_ref as v2
from dist_gat_ref import bounds, row_block

ROW_NAMES = ("out", "lse", "D", "G_Zd", "P", "G_Zs")                # row-local: the single-GPU bits on the device
MUTATIONS = ("Zd rows", "halves swapped", "local lse/D", "att_grad whole")
OP_SHAPES = [(4, 32), (3, 7), (1, 260)]          # float4 nt 1, the element path, float4 nt 2 (gatv2_ref.SHAPES)


def halves(Z2):
    """(Zs, Zd) of a [rows x 2 d] buffer: columns [0, d) and [d, 2 d)"""
    d = Z2.shape[1] // 2
    return np.ascontiguousarray(Z2[:, :d]), np.ascontiguousarray(Z2[:, d:])


def rank_forward(F_blk, Z2_all, Z2_loc, att, K, T=np.float64):
    """out_loc and lse_loc over the rank's row block of F: Zs of all vertices, Zd of the rank's rows"""
    r = v2.attention_v2(*F_blk, halves(Z2_all)[0], halves(Z2_loc)[1], att, K, dtype=T)
    return dict(out=r["out"], lse=r["lse"])


def rank_backward_dst(F_blk, Z2_all, Z2_loc, G_loc, att, K, lse_loc, T=np.float64):
    """D_loc, G_Zd_loc, P_loc and the rank's partial G_att (the column sums of its P) over the same row block, from the
    forward's lse (out is recomputed with it)"""
    r = v2.attention_v2(*F_blk, halves(Z2_all)[0], halves(Z2_loc)[1], att, K, G=G_loc, dtype=T, lse=lse_loc)
    return dict(D=r["D"], G_Zd=r["G_Zd"], P=r["P"], G_att=r["P"].sum(axis=0, dtype=T).reshape(1, -1))


def rank_backward_src(FT_blk, Z2_loc, Z2_all, G_all, att, K, lse_all, D_all, T=np.float64):
    """G_Zs_loc over the rank's row block of F^T (rows: local sources, entries: global destinations): Zs of the rank's rows,
    Zd, G, lse and D of all destinations"""
    n = G_all.shape[0]
    ip, ix = ref.transpose_pattern(*FT_blk, n)                  # n destinations x local sources
    r = v2.attention_v2(ip, ix, halves(Z2_loc)[0], halves(Z2_all)[1], att, K, G=G_all, dtype=T, lse=lse_all, D=D_all)
    return dict(G_Zs=r["G_Zs"])


def partitioned(indptr, indices, Zs, Zd, G, att, K, P, T=np.float64, mutation=None, rank=1):
    """the outputs of ROW_NAMES assembled from P ranks, G_att as the sum of their partials (summed in ``T``) and the partials.
    ``mutation`` (one of MUTATIONS) is applied on ``rank`` alone:
      "Zd rows"         the rank takes rows [0, rows) of Zd for its own in the forward and in backward_dst
      "halves swapped"  the rank reads Z2_all and its Z2 with the halves exchanged, in all three calls
      "local lse/D"     backward_src indexes the rank's OWN lse / D with global destinations (restated by repeating the
                        rank's [rows x K] arrays down the n destinations; the device would read past their end)
      "att_grad whole"  the rank's partial G_att is taken for the total"""
    n = indptr.size - 1
    p = bounds(n, P)
    t_indptr, t_indices = ref.transpose_pattern(indptr, indices, n)
    Z2 = np.concatenate([np.asarray(Zs), np.asarray(Zd)], axis=1)
    Z2_all = np.concatenate([Z2[p[r]:p[r + 1]] for r in range(P)])                # the all-gather of the Z2 shards
    G_all = np.concatenate([G[p[r]:p[r + 1]] for r in range(P)])
    swapped = np.concatenate(halves(Z2_all)[::-1], axis=1)
    blocks = [(row_block(indptr, indices, p[r], p[r + 1]), row_block(t_indptr, t_indices, p[r], p[r + 1])) for r in range(P)]

    def operands(r):
        """(Z2_all, the rank's Z2 for the calls over F, the rank's Z2 for the call over F^T) as rank r reads them"""
        lo, hi = p[r], p[r + 1]
        mut = mutation if r == rank else None
        if mut == "halves swapped":
            return swapped, swapped[lo:hi], swapped[lo:hi]
        if mut == "Zd rows":
            return Z2_all, np.concatenate([Z2_all[lo:hi, :Z2.shape[1] // 2], Z2_all[0:hi - lo, Z2.shape[1] // 2:]], axis=1), Z2_all[lo:hi]
        return Z2_all, Z2_all[lo:hi], Z2_all[lo:hi]

    fwd, bwd = [], []
    for r in range(P):
        lo, hi = p[r], p[r + 1]
        Za, Zl, _ = operands(r)
        f = rank_forward(blocks[r][0], Za, Zl, att, K, T)
        fwd.append(f)
        bwd.append(rank_backward_dst(blocks[r][0], Za, Zl, G[lo:hi], att, K, f["lse"], T))
    # the record exchange: lse and D of all destinations, as every rank sent them
    lse_all, D_all = np.concatenate([f["lse"] for f in fwd]), np.concatenate([b["D"] for b in bwd])
    src = []
    for r in range(P):
        lo, hi = p[r], p[r + 1]
        Za, _, Zl = operands(r)
        la, Da = lse_all, D_all
        if r == rank and mutation == "local lse/D":
            la, Da = np.resize(fwd[r]["lse"], lse_all.shape), np.resize(bwd[r]["D"], D_all.shape)
        src.append(rank_backward_src(blocks[r][1], Zl, Za, G_all, att, K, la, Da, T))
    res = {k: np.concatenate([x[k] for x in fwd]) for k in ("out", "lse")}
    res.update({k: np.concatenate([x[k] for x in bwd]) for k in ("D", "G_Zd", "P")})
    res["G_Zs"] = np.concatenate([x["G_Zs"] for x in src])
    parts = [b["G_att"] for b in bwd]
    total = parts[0].astype(T)
    for x in parts[1:]:
        total = (total + x).astype(T)
    res["G_att"] = parts[rank].copy() if mutation == "att_grad whole" else total
    res["G_att_partials"] = parts
    return res


# ---- the packed destination record (include/mggcn.h: mggcn_gatv2_pack_dst_f32) ----------------------------------------------------
def pack_dst(lse, D):
    """rec[(i K + k) 2 + {0, 1}] = lse[i, k], D[i, k] as float32 [n x K x 2]; bit patterns are copied as they are"""
    lse, D = (np.asarray(a, dtype=np.float32) for a in (lse, D))
    assert lse.shape == D.shape and lse.ndim == 2
    rec = np.empty(lse.shape + (2,), dtype=np.float32)
    rec.view(np.uint32)[:, :, 0], rec.view(np.uint32)[:, :, 1] = lse.view(np.uint32), D.view(np.uint32)
    return rec


def unpack_dst(rec):
    rec = np.ascontiguousarray(rec, dtype=np.float32).view(np.uint32)
    return rec[:, :, 0].copy().view(np.float32), rec[:, :, 1].copy().view(np.float32)


# ---- the cases the CPU and the device tests share -----------------------------------------------------------------------------------
def op_case(K, dh):
    """gatv2_ref.case on kernel_graph_long as F: inputs, the exact whole-graph restatement and its row scales"""
    return v2.case("long", K, dh)


def exchange_bytes_v2(n, P, sizes, heads):
    """bytes one rank hands to the shard exchange in one training epoch of dist_gat(variant="v2"): per
    layer the Z2 shard (2 out floats a row) in the forward, the G shard (out floats) and the records (8 bytes a head) in
    the backward"""
    per_layer = list(heads) if isinstance(heads, (list, tuple)) else [heads] * (len(sizes) - 2) + [1]
    rows = n // P
    return sum(rows * (3 * out * 4 + 8 * K) for out, K in zip(sizes[1:], per_layer))
