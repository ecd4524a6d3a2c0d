"""The row-partitioned attention on the host, for the dist_gat tests: the algebra of mg-gcn_amd/dist_gat.py restated in numpy
on gat_ref.attention / gat_dropout_ref.attention.  Every "rank" function sees only its rows of Z and G, its row blocks of F
and F^T (global columns) and the arrays a collective delivers (Z_all, G_all, and s_dst / lse / D of all destinations); the
driver partitioned() plays the collectives by concatenation.  Also the packed destination record of
mggcn_gat_pack_dst_f32 in numpy, and the three offset mutations the device tests must be able to see."""
import numpy as np

import dropout_ref
import gat_dropout_ref as dref
import gat_ref as ref

ROW_NAMES = ("out", "lse", "D", "ds_dst", "ds_src", "G_Z")          # row-local: the single-GPU bits on the device
MUTATIONS = ("s_dst rows", "forward dst0", "backward_src offsets")
DROP_P = 0.5


def bounds(n, P):
    assert n % P == 0
    return [i * n // P for i in range(P + 1)]


def row_block(indptr, indices, a, b):
    """rows [a, b) of a CSR pattern, columns unchanged"""
    lo, hi = int(indptr[a]), int(indptr[b])
    return (indptr[a:b + 1] - indptr[a]).astype(np.uint32), np.ascontiguousarray(indices[lo:hi])


def scores(Z, att, K, T=np.float64):
    """s_dst, s_src [rows x K] of the rows of Z"""
    n, d = Z.shape
    Z3, a3 = np.asarray(Z, dtype=T).reshape(n, K, d // K), np.asarray(att, dtype=T).reshape(2, K, d // K)
    return (Z3 * a3[0]).sum(axis=2, dtype=T), (Z3 * a3[1]).sum(axis=2, dtype=T)


def _attend(indptr, indices, Z, att, K, drop, dst0, src0, T, **kw):
    """gat_ref.attention, or gat_dropout_ref.attention with the mask of ``drop`` = (p, seed, stream) at the offsets"""
    if drop is None:
        return ref.attention(indptr, indices, Z, att, K, dtype=T, **kw)
    p, seed, stream = drop
    keep = dref.keep_mask(indptr, indices, K, p, seed, stream, dst0, src0)
    return dref.attention(indptr, indices, Z, att, K, keep, dropout_ref.params(p)[1], dtype=T, **kw)


def rank_forward(F_blk, Z_all, att, K, lo, hi, drop=None, T=np.float64, s_dst_rows=None, dst0=None):
    """out_loc, lse_loc, and the scores of all vertices; ``s_dst_rows`` / ``dst0``: the mutations (None: [lo, hi) and lo)"""
    s_dst_all, s_src_all = scores(Z_all, att, K, T)
    a, b = (lo, hi) if s_dst_rows is None else s_dst_rows
    r = _attend(*F_blk, Z_all, att, K, drop, lo if dst0 is None else dst0, 0, T, Z_dst=np.zeros((hi - lo, Z_all.shape[1])),
                s_dst=s_dst_all[a:b], s_src=s_src_all)
    return dict(out=r["out"], lse=r["lse"], s_dst_all=s_dst_all, s_src_all=s_src_all, s_dst=s_dst_all[a:b])


def rank_backward_dst(F_blk, Z_all, G_loc, att, K, lo, hi, fwd, drop=None, T=np.float64, dst0=None):
    """D_loc, ds_dst_loc over the same row block, from the forward's scalars (out is recomputed with them)"""
    r = _attend(*F_blk, Z_all, att, K, drop, lo if dst0 is None else dst0, 0, T, G=G_loc, Z_dst=np.zeros((hi - lo, Z_all.shape[1])),
                s_dst=fwd["s_dst"], s_src=fwd["s_src_all"], lse=fwd["lse"])
    return dict(D=r["D"], ds_dst=r["ds_dst"])


def rank_backward_src(FT_blk, Z_loc, G_all, att, K, lo, hi, s_dst_all, lse_all, D_all, s_src_loc, ds_dst_loc, drop=None,
                      T=np.float64, offsets=None):
    """ds_src_loc, G_Z_loc and the rank's partial G_att over the row block of F^T (rows: local sources, entries: global
    destinations); ``offsets``: (dst0, src0) of the mask (None: (0, lo); the mutation passes them swapped)"""
    n, d = G_all.shape
    dst0, src0 = (0, lo) if offsets is None else offsets
    ip, ix = ref.transpose_pattern(*FT_blk, n)                  # n destinations x (hi - lo) local sources
    r = _attend(ip, ix, Z_loc, att, K, drop, dst0, src0, T, G=G_all, Z_dst=np.zeros((n, d)), s_dst=s_dst_all, s_src=s_src_loc,
                lse=lse_all, D=D_all)
    a3 = np.asarray(att, dtype=T).reshape(2, K, d // K)
    dd = np.asarray(ds_dst_loc, dtype=T)
    G_Z = r["G_Z"].reshape(hi - lo, K, d // K) + dd[:, :, None] * a3[0]          # ds_dst is the rank's own: indexed by source
    Z3 = np.asarray(Z_loc, dtype=T).reshape(hi - lo, K, d // K)
    G_att = np.stack([(dd[:, :, None] * Z3).sum(axis=0, dtype=T), (r["ds_src"][:, :, None] * Z3).sum(axis=0, dtype=T)])
    return dict(ds_src=r["ds_src"], G_Z=G_Z.reshape(hi - lo, d), G_att=G_att.reshape(2, d))


def partitioned(indptr, indices, Z, G, att, K, P, drop=None, T=np.float64, mutation=None, rank=1):
    """the outputs of ROW_NAMES assembled from P ranks, and G_att as the sum of their partials.  ``mutation`` (one of
    MUTATIONS) is applied on ``rank`` alone."""
    n = indptr.size - 1
    p = bounds(n, P)
    t_indptr, t_indices = ref.transpose_pattern(indptr, indices, n)
    Z_all = np.concatenate([Z[p[r]:p[r + 1]] for r in range(P)])                  # the all-gather of the Z shards
    G_all = np.concatenate([G[p[r]:p[r + 1]] for r in range(P)])
    blocks = [(row_block(indptr, indices, p[r], p[r + 1]), row_block(t_indptr, t_indices, p[r], p[r + 1])) for r in range(P)]
    fwd, bwd = [], []
    for r in range(P):
        lo, hi = p[r], p[r + 1]
        mut = mutation if r == rank else None
        f = rank_forward(blocks[r][0], Z_all, att, K, lo, hi, drop, T, s_dst_rows=(0, hi - lo) if mut == MUTATIONS[0] else None,
                         dst0=0 if mut == MUTATIONS[1] else None)
        fwd.append(f)
        bwd.append(rank_backward_dst(blocks[r][0], Z_all, G[lo:hi], att, K, lo, hi, f, drop, T,
                                     dst0=0 if mut == MUTATIONS[1] else None))
    # the record exchange: s_dst, lse and D of all destinations, as every rank sent them
    s_dst_all = np.concatenate([f["s_dst"] for f in fwd])
    lse_all, D_all = np.concatenate([f["lse"] for f in fwd]), np.concatenate([b["D"] for b in bwd])
    src = []
    for r in range(P):
        lo, hi = p[r], p[r + 1]
        src.append(rank_backward_src(blocks[r][1], Z[lo:hi], G_all, att, K, lo, hi, s_dst_all, lse_all, D_all,
                                     fwd[r]["s_src_all"][lo:hi], bwd[r]["ds_dst"], drop, T,
                                     offsets=(lo, 0) if (r == rank and mutation == MUTATIONS[2]) else None))
    res = {k: np.concatenate([x[k] for x in fwd]) for k in ("out", "lse")}
    res.update({k: np.concatenate([x[k] for x in bwd]) for k in ("D", "ds_dst")})
    res.update({k: np.concatenate([x[k] for x in src]) for k in ("ds_src", "G_Z")})
    res["G_att"] = sum(x["G_att"] for x in src)
    res["G_att_partials"] = [x["G_att"] for x in src]
    return res


# ---- the packed destination record (include/mggcn.h: mggcn_gat_pack_dst_f32) ------------------------------------------------------
def pack_dst(s_dst, lse, D):
    """rec[(i K + k) 4 + {0, 1, 2, 3}] = s_dst[i, k], lse[i, k], D[i, k], 0 as float32 [n x K x 4]"""
    s_dst, lse, D = (np.asarray(a, dtype=np.float32) for a in (s_dst, lse, D))
    assert s_dst.shape == lse.shape == D.shape and s_dst.ndim == 2
    return np.ascontiguousarray(np.stack([s_dst, lse, D, np.zeros_like(D)], axis=2))


def unpack_dst(rec):
    rec = np.asarray(rec, dtype=np.float32)
    return rec[:, :, 0].copy(), rec[:, :, 1].copy(), rec[:, :, 2].copy()


# ---- the cases the CPU and the device tests share -----------------------------------------------------------------------------------
OP_SHAPES = [(4, 32), (3, 7), (1, 260)]          # float4 nt 1, the element path, float4 nt 2 (gat_ref.EDGE_SHAPES)


def op_case(K, dh, drop):
    """gat_ref.edge_case / gat_dropout_ref.drop_case on kernel_graph_long as F: inputs, the exact whole-graph restatement
    and its row scales.  ``drop``: False, or True for p = DROP_P at gat_dropout_ref's SEED and STREAM"""
    c = dref.drop_case("long", K, dh, DROP_P) if drop else ref.edge_case("long", K, dh)
    return c, ((DROP_P, dref.SEED, dref.STREAM) if drop else None)


def exchange_bytes(n, P, sizes, heads):
    """bytes one rank hands to the shard exchange in one training epoch: per layer the Z shard in the
    forward, the G shard and the records in the backward"""
    per_layer = list(heads) if isinstance(heads, (list, tuple)) else [heads] * (len(sizes) - 2) + [1]
    rows = n // P
    return sum(rows * (2 * out * 4 + 16 * K) for out, K in zip(sizes[1:], per_layer))
