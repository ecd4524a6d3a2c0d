"""Do two trees compute the same bits in every GAT entry point?  
Every call of the GAT part of ops -- scores, forward, backward_dst, backward_src with and without attention dropout,
pack_dst, backward_src_rec with and without dropout, scores_backward, the three edge-feature calls with and without dropout
at de = 8 and de = 3 (E in the entry order of the matrix walked), the four GATv2 calls on [rows x width] operands and on the model's [Zs | Zd] buffers, and the three dot-product calls (inputs of gatdot_ref) on [rows x width] operands and
on the thirds of [rows x 3 width] buffers -- on the graphs "long", "longT" and "rect" of gat_ref.edge_graphs(), at one (K, dh)
per compiled (VEC, NT, U) variant (gat_ref.EDGE_RECT) plus (1, 1024) with every dense operand one float off, which is the
16-tile element path; and att_grad beyond two passes of its capped grid.  One line per output: the entry point, the graph,
the shape and the SHA-256 of the raw bytes.  The tests hold the kernels against an fp64 restatement within a tolerance and
would not see a reordered sum; the lines of two trees compared with diff do.  A manual script, not a test: run it once per
tree, each in its own process.
Usage: python profiles/experiments/gat_bits.py --root DIR      (DIR: the tree whose package is imported and run)"""
import argparse
import hashlib
import os
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
root = os.path.abspath(ap.parse_args().root)
sys.path[:0] = [root, os.path.join(root, "tests")]
import __graft_entry__ as g
import gat_efeat_ref
import gat_ref
import gatdot_ref
import gatv2_ref
import torch

pkg = g.load_package()
ctx = pkg.context(0)
ops, dn = pkg.ops, pkg.dn_matrix
DROP = ops.dropout_params(0.5) + (0x1234567890ABCDEF, 7, 1000, 70000)        # seed, stream, dst0, src0
COLSUM_BLOCKS = 512                                                         # csrc/gat_internal.h kGatColsumBlocks


def dense(a, off=0):
    """the array (or zeros of the shape) a on the device, its first element ``off`` floats past a 16-byte boundary"""
    a = np.zeros(a, dtype=np.float32) if isinstance(a, tuple) else np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.zeros(a.size + off, dtype=torch.float32, device=ctx.device)
    M = dn(a.shape[0], a.shape[1], buffer=buf[off:])
    M.t.copy_(torch.from_numpy(a))
    torch.cuda.synchronize()
    return M


def report(call, tag, **outs):
    ctx.sync()
    for name, t in outs.items():
        a = (t.t if isinstance(t, dn) else t).detach().cpu().numpy()
        print(f"{call:28s} {tag:32s} {name:7s} {'x'.join(map(str, a.shape)):12s} {hashlib.sha256(a.tobytes()).hexdigest()}", flush=True)


def csr(indptr, indices, m):
    return pkg.csr_matrix(indptr.copy(), indices.copy(), np.ones(indices.size, dtype=np.float32), m)


def run_v1(tag, F, F_T, n, n_src, K, dh, off):
    d = K * dh
    Zh, Zdh, Gh, atth = gat_ref.tolerance_inputs(n, n_src, K, dh)
    Z, G, att = dense(Zh, off), dense(Gh, off), dense(atth, off)
    Zd = Z if n == n_src else dense(Zdh, off)
    s_dst, s_src = dense((n, K)), dense((n_src, K))
    ops.gat_scores(ctx, Zd, att, s_dst, None, K)
    ops.gat_scores(ctx, Z, att, None, s_src, K)
    report("gat_scores", tag, s_dst=s_dst, s_src=s_src)
    for drop, sfx in ((None, ""), (DROP, "+drop")):
        out, lse, D, ds_dst = dense((n, d), off), dense((n, K)), dense((n, K)), dense((n, K))
        ops.gat_forward(ctx, F, Z, s_dst, s_src, out, lse, K, drop=drop)
        report("gat_forward" + sfx, tag, out=out, lse=lse)
        ops.gat_backward_dst(ctx, F, Z, s_dst, s_src, lse, G, out, D, ds_dst, K, drop=drop)
        report("gat_backward_dst" + sfx, tag, D=D, ds_dst=ds_dst)
        dd = ds_dst if n == n_src else None                                   # indexed by source: the square case only
        ds_src, G_Z = dense((n_src, K)), dense((n_src, d), off)
        ops.gat_backward_src(ctx, F_T, Z, s_dst, s_src, lse, D, G, att, dd, ds_src, G_Z, K, drop=drop)
        report("gat_backward_src" + sfx, tag, ds_src=ds_src, G_Z=G_Z)
        rec = torch.zeros(n * K * 4, dtype=torch.float32, device=ctx.device)
        torch.cuda.synchronize()            # the fill runs on torch's stream, the pack on the context's
        ops.gat_pack_dst(ctx, s_dst, lse, D, rec)
        report("gat_pack_dst" + sfx, tag, rec=rec)
        ds_src_r, G_Z_r = dense((n_src, K)), dense((n_src, d), off)
        ops.gat_backward_src_rec(ctx, F_T, Z, rec, s_src, G, att, dd, ds_src_r, G_Z_r, K, drop=drop)
        report("gat_backward_src_rec" + sfx, tag, ds_src=ds_src_r, G_Z=G_Z_r)
        G_att = dense((2, d), off)
        ops.gat_scores_backward(ctx, ds_dst, Zd, ds_src, Z, G_att, K)
        report("gat_scores_backward" + sfx, tag, G_att=G_att)


def run_efeat(tag, F, F_T, perm, n, n_src, K, dh, off):
    """the edge-feature calls: de = 8 reads a row of E with 16-byte loads, de = 3 element by element; E_F is in F's entry
    order (forward, backward_dst), E_F[perm] in F_T's (backward_src)"""
    d = K * dh
    Zh, Zdh, Gh, atth = gat_ref.tolerance_inputs(n, n_src, K, dh)
    Z, G, att = dense(Zh, off), dense(Gh, off), dense(atth, off)
    s_dst, s_src = dense((n, K)), dense((n_src, K))
    ops.gat_scores(ctx, Z if n == n_src else dense(Zdh, off), att, s_dst, None, K)
    ops.gat_scores(ctx, Z, att, None, s_src, K)
    for de in (8, 3):
        Eh, Uh = gat_efeat_ref.efeat_inputs(F.nnz(), K, de)
        E_F, E_T, U = dense(Eh), dense(Eh[perm]), dense(Uh)
        for drop, sfx in ((None, ""), (DROP, "+drop")):
            etag = f"{tag} de={de}"
            out, lse, D, ds_dst, P_e = dense((n, d), off), dense((n, K)), dense((n, K)), dense((n, K)), dense((n, K * de))
            ops.gat_forward_efeat(ctx, F, Z, s_dst, s_src, out, lse, E_F, U, K, drop=drop)
            report("gat_forward_efeat" + sfx, etag, out=out, lse=lse)
            ops.gat_backward_dst_efeat(ctx, F, Z, s_dst, s_src, lse, G, out, D, ds_dst, E_F, U, P_e, K, drop=drop)
            report("gat_backward_dst_efeat" + sfx, etag, D=D, ds_dst=ds_dst, P_e=P_e)
            dd = ds_dst if n == n_src else None
            ds_src, G_Z = dense((n_src, K)), dense((n_src, d), off)
            ops.gat_backward_src_efeat(ctx, F_T, Z, s_dst, s_src, lse, D, G, att, dd, ds_src, G_Z, E_T, U, K, drop=drop)
            report("gat_backward_src_efeat" + sfx, etag, ds_src=ds_src, G_Z=G_Z)


def run_v2(tag, F, F_T, n, n_src, K, dh, off):
    d = K * dh
    Zsh, Zdh, Gh, atth = gatv2_ref.inputs(n, n_src, K, dh)
    G, att = dense(Gh, off), dense(atth, off)
    forms = {"": (dense(Zsh, off), dense(Zdh, off), d),
             "[Zs|Zd]": (dense(np.concatenate([Zsh, np.zeros_like(Zsh)], axis=1), off),
                         dense(np.concatenate([np.zeros_like(Zdh), Zdh], axis=1), off), 2 * d)}
    for sfx, (Zs, Zd, gw) in forms.items():
        out, lse, D, P = dense((n, d), off), dense((n, K)), dense((n, K)), dense((n, d), off)
        G_Zd, G_Zs, G_att = dense((n, gw), off), dense((n_src, gw), off), dense((1, d), off)
        ops.gatv2_forward(ctx, F, Zs, Zd, att, out, lse, K)
        report("gatv2_forward" + sfx, tag, out=out, lse=lse)
        ops.gatv2_backward_dst(ctx, F, Zs, Zd, att, lse, G, out, D, G_Zd, P, K)
        report("gatv2_backward_dst" + sfx, tag, D=D, G_Zd=G_Zd, P=P)
        ops.gatv2_att_grad(ctx, P, G_att)
        report("gatv2_att_grad" + sfx, tag, G_att=G_att)
        ops.gatv2_backward_src(ctx, F_T, Zs, Zd, att, lse, D, G, G_Zs, K)
        report("gatv2_backward_src" + sfx, tag, G_Zs=G_Zs)


def run_dot(tag, F, F_T, n, n_src, K, dh, off):
    d = K * dh
    Zqh, Zkh, Zvh, Gh = gatdot_ref.inputs(n, n_src, K, dh)
    G = dense(Gh, off)
    zq, zs = np.zeros_like(Zqh), np.zeros_like(Zkh)
    Zkv = dense(np.concatenate([zs, Zkh, Zvh], axis=1), off)                  # one buffer passed as Zk and as Zv
    forms = {"": (dense(Zqh, off), dense(Zkh, off), dense(Zvh, off), d),
             "[Zq|Zk|Zv]": (dense(np.concatenate([Zqh, zq, zq], axis=1), off), Zkv, Zkv, 3 * d)}
    for sfx, (Zq, Zk, Zv, gw) in forms.items():
        out, lse, D = dense((n, d), off), dense((n, K)), dense((n, K))
        G_Zq, G_Zk = dense((n, gw), off), dense((n_src, gw), off)
        G_Zv = G_Zk if sfx else dense((n_src, gw), off)                        # the thirds of one gradient buffer
        ops.gatdot_forward(ctx, F, Zq, Zk, Zv, out, lse, K)
        report("gatdot_forward" + sfx, tag, out=out, lse=lse)
        ops.gatdot_backward_dst(ctx, F, Zq, Zk, Zv, lse, G, out, D, G_Zq, K)
        report("gatdot_backward_dst" + sfx, tag, D=D, G_Zq=G_Zq)
        ops.gatdot_backward_src(ctx, F_T, Zq, Zk, Zv, lse, D, G, G_Zk, G_Zv, K)
        report("gatdot_backward_src" + sfx, tag, G_Zk=G_Zk, G_Zv=G_Zv)


for name, (indptr, indices, n_src) in gat_ref.edge_graphs().items():
    n = indptr.size - 1
    F, F_T = csr(indptr, indices, n_src), csr(*gat_ref.transpose_pattern(indptr, indices, n_src), n)
    perm = gat_efeat_ref.edge_perm(indices)
    for K, dh, off in [(K, dh, 0) for K, dh in gat_ref.EDGE_RECT] + [(1, 1024, 1)]:
        tag = f"{name} K={K} dh={dh}" + (" off=1" if off else "")
        run_v1(tag, F, F_T, n, n_src, K, dh, off)
        run_efeat(tag, F, F_T, perm, n, n_src, K, dh, off)
        run_v2(tag, F, F_T, n, n_src, K, dh, off)
        run_dot(tag, F, F_T, n, n_src, K, dh, off)

rows = 2 * 256 * COLSUM_BLOCKS + 77                 # width 1: a workgroup takes 256 rows, so this is beyond two passes
P, G_att = dense(np.random.default_rng(1).standard_normal((rows, 1), dtype=np.float32)), dense((1, 1))
ops.gatv2_att_grad(ctx, P, G_att)
report("gatv2_att_grad", f"rows={rows}", G_att=G_att)
