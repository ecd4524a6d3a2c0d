"""What the bf16 MLP link decoder costs next to the fp32 one and the dot decoder, all three in one process and run
(DESIGN.md 3.15.7), with R = 1, on the two patterns of profiles/experiments/link_mlp.py: a uniform pattern of ogbl-collab's size
and the Reddit-shaped stand-in with P = the graph itself.  At (d, hd) = (128, 128) and (64, 64), per launch: the time of
mggcn_link_mlp_loss_bf16 / mggcn_link_mlp_pairs_bf16, its ratio to the fp32 decoder's launch, to the dot decoder's matching walk
(the gather floor a walk cannot beat) and to the bf16 MFMA floor -- 2 d hd flops per product and pair, two products per pair,
at 16 times the 157 TF of the fp32 instruction; then the two packing launches and the whole head of either dtype.  Device
events after a warm-up, medians of SAMPLES samples.  A manual script, not a test; not to be run under a profiler.
Usage: python profiles/experiments/link_mlp_bf16.py [--collab-only]"""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import __graft_entry__ as g

pkg = g.load_package()
ctx = pkg.context(0)
lib, ops, dn = ctx.lib, pkg.ops, pkg.dn_matrix
SAMPLES, PEAK16 = 7, 16 * 157e12


def sample(fn):
    ctx.record("exp-begin", 0)
    fn()
    ctx.record("exp-end", 0)
    ctx.sync()
    return float(lib.mggcn_event_elapsed_ms(ctx.events["exp-begin"], ctx.events["exp-end"]))


def timed(fn):
    sample(fn)                                                   # warm-up: code objects, caches
    v = [sample(fn) for _ in range(SAMPLES)]
    return statistics.median(v), min(v), max(v)


def show(tag, b16, f32=None, dot=None, pairs=0, d=0, hd=0):
    line = f"  {tag:18s} bf16 {b16[0]:9.3f} ms (min {b16[1]:.3f}, max {b16[2]:.3f})"
    if f32:
        line += f" | fp32 {f32[0]:9.3f} (min {f32[1]:.3f}, max {f32[2]:.3f}), bf16 / fp32 {b16[0] / f32[0]:.3f}"
    if dot:
        line += f" | dot {dot[0]:8.3f}, bf16 / dot x{b16[0] / dot[0]:.2f}"
    if pairs:
        floor = 1e3 * pairs * 2 * (2 * d * hd) / PEAK16
        line += f" | bf16 floor {floor:7.3f} ms, x{b16[0] / floor:.1f}"
    print(line, flush=True)


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
        heads = {dt: pkg.mlp_link_predictor(encoder_stub(n, d), P, hidden=hd, neg_ratio=1, seed=1, decoder_dtype=dt) for dt in ("f32", "bf16")}
        weights = heads["f32"].weights()
        for t, w_ in zip(heads["bf16"].params(), weights):
            t.init(w_)
        H = dn.from_numpy((rng.standard_normal((n, d)) * d ** -0.25).astype(np.float32))
        for head in heads.values():
            head.loss_backward(ctx, H)
            ctx.sync()
        f, b = heads["f32"], heads["bf16"]
        print(f" [d = {d}, hd = {hd}] loss fp32 {f.read()[0]:.4f} bf16 {b.read()[0]:.4f}, acc fp32 {f.read()[1]:.4f} bf16 {b.read()[1]:.4f}")
        (keys, vals, ka, va), work = f._arrays
        r, (pp, px, _), (tp, tx, _), params = f._rows, P.device(ctx.device), f.P_T.device(ctx.device), f.params()
        Hb, image = b._images
        packed = (image, b.b1, b.w2, b.b2)
        w = 1.0 / M
        launches = (("loss (a) P+neg", pp, px, 2 * M, dict(positive=True, weight=w, neg_ratio=1, neg_weight=w, seed=1, epoch=0,
                                                           row_loss=r["row_loss"], row_correct=r["row_correct"])),
                    ("loss (b) P^T", tp, tx, M, dict(positive=True, weight=w, beta=1.0)),
                    ("loss (c) NT", r["nt_indptr"], vals, M, dict(positive=False, weight=w, beta=1.0)))
        for tag, a_, b_, pairs, kw in launches:
            show(tag, timed(lambda: ops.link_mlp_loss_bf16(ctx, n, n, a_, b_, M, Hb, packed, r["G"], **kw)),
                 timed(lambda: ops.link_mlp_loss(ctx, n, n, a_, b_, M, H, params, r["G"], **kw)),
                 timed(lambda: ops.link_dot_loss(ctx, n, n, a_, b_, M, H, r["G"], **kw)), pairs, d, hd)
        train = (f._head, px, M, 1, n, 1, 0)
        wg = dict(train=train, weight=w, neg_weight=w, grads=f._grads, partials=f._partials)
        show("wgrad", timed(lambda: ops.link_mlp_pairs_bf16(ctx, Hb, packed, **wg)), timed(lambda: ops.link_mlp_pairs(ctx, H, params, **wg)),
             None, 2 * M, d, hd)
        show("pack H", timed(lambda: ops.convert_bf16(ctx, H, Hb)))
        show("pack W1", timed(lambda: ops.link_mlp_pack_bf16(ctx, b.W1, image)))
        show("whole mlp head", timed(lambda: b.loss_backward(ctx, H)), timed(lambda: f.loss_backward(ctx, H)))
        del heads, f, b, head, H, Hb, image, packed
        import torch
        torch.cuda.empty_cache()
