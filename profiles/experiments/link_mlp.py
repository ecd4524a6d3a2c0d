"""What the MLP link decoder costs, with R = 1, on two patterns: the Reddit-shaped stand-in
(synth_reddit_like(1.0, seed=1)) with P = the graph itself, and a uniform pattern of ogbl-collab's size (235 868 vertices,
2.4 M pairs).  At (d, hd) = (128, 128) and (64, 64): the three launches of mggcn_link_mlp_loss_f32 and the parameter-gradient
launch of mggcn_link_mlp_pairs_f32 on random embeddings, next to the dot decoder's three launches from the same run, and each
MLP launch's distance from the fp32 MFMA floor -- 2 d hd flops per product and pair, two products per pair in either kernel,
at the 157 TF that VERDICT.md quotes.  Device events after a warm-up, medians of SAMPLES samples.  A manual script, not a
test; not to be run under a profiler.
Usage: python profiles/experiments/link_mlp.py [--collab-only]"""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import __graft_entry__ as g

pkg = g.load_package()
ctx = pkg.context(0)
lib, ops, dn = ctx.lib, pkg.ops, pkg.dn_matrix
SAMPLES, PEAK = 7, 157e12


def sample(fn):
    ctx.record("exp-begin", 0)
    fn()
    ctx.record("exp-end", 0)
    ctx.sync()
    return float(lib.mggcn_event_elapsed_ms(ctx.events["exp-begin"], ctx.events["exp-end"]))


def timed(fn, pairs=0, d=0, hd=0):
    sample(fn)                                                   # warm-up: code objects, caches
    v = [sample(fn) for _ in range(SAMPLES)]
    med = statistics.median(v)
    floor = 1e3 * pairs * 2 * (2 * d * hd) / PEAK
    return f"{med:9.3f} ms (min {min(v):.3f}, max {max(v):.3f})" + (f"  floor {floor:7.3f} ms, x{med / floor:.1f}" if pairs else "")


class encoder_stub(pkg.gcn):
    """only what the heads' constructors read: a head is measured without an encoder"""

    def __init__(self, n, d):
        self.A, self._out_width, self.fused = type("rows", (), {"n": staticmethod(lambda: n)}), d, True


def graphs():
    n, deg = 235_868, 10
    ip, ix, dv = pkg.datasets.synth_uniform_csr(n, deg, seed=7)
    yield "collab-sized uniform", ip, ix, dv
    if "--collab-only" not in sys.argv:
        (ip, ix, dv), _, _ = pkg.datasets.synth_reddit_like(1.0, seed=1)
        yield "Reddit-shaped stand-in", ip, ix, dv


rng = np.random.default_rng(0)
for name, ip, ix, dv in graphs():
    n, M = ip.shape[0] - 1, int(ip[-1])
    print(f"[{name}] n {n}, M = nnz {M}, R 1", flush=True)
    for d, hd in ((128, 128), (64, 64)):
        P = pkg.csr_matrix(ip, ix, dv.copy(), n)
        head = pkg.mlp_link_predictor(encoder_stub(n, d), P, hidden=hd, neg_ratio=1, seed=1)
        H = dn.from_numpy((rng.standard_normal((n, d)) * d ** -0.25).astype(np.float32))
        head.loss_backward(ctx, H)
        ctx.sync()
        (keys, vals, ka, va), work = head._arrays
        r, (pp, px, _), (tp, tx, _), params = head._rows, P.device(ctx.device), head.P_T.device(ctx.device), head.params()
        w = 1.0 / M
        print(f" [d = {d}, hd = {hd}] loss {head.read()[0]:.4f}, acc {head.read()[1]:.4f}")
        launches = (("(a) P+neg", pp, px, 2 * M, dict(positive=True, weight=w, neg_ratio=1, neg_weight=w, seed=1, epoch=0,
                                                      row_loss=r["row_loss"], row_correct=r["row_correct"])),
                    ("(b) P^T  ", tp, tx, M, dict(positive=True, weight=w, beta=1.0)),
                    ("(c) NT   ", r["nt_indptr"], vals, M, dict(positive=False, weight=w, beta=1.0)))
        for tag, a, b, pairs, kw in launches:
            print(f"  mlp loss {tag} {timed(lambda: ops.link_mlp_loss(ctx, n, n, a, b, M, H, params, r['G'], **kw), pairs, d, hd)}")
            print(f"  dot loss {tag} {timed(lambda: ops.link_dot_loss(ctx, n, n, a, b, M, H, r['G'], **kw))}", flush=True)
        train = (head._head, px, M, 1, n, 1, 0)
        print(f"  mlp wgrad          {timed(lambda: ops.link_mlp_pairs(ctx, H, params, train=train, weight=w, neg_weight=w, grads=head._grads, partials=head._partials), 2 * M, d, hd)}")
        print(f"  whole mlp head     {timed(lambda: head.loss_backward(ctx, H))}", flush=True)
        del head, H
        import torch
        torch.cuda.empty_cache()
