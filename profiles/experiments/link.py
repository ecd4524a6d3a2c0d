"""What the link head costs, on the Reddit-shaped stand-in (synth_reddit_like(1.0, seed=1)) with P = the
graph itself (every entry a positive pair) and R = 1, at d = 128 and d = 41:
  * draw / sort / bounds, the three launches of mggcn_link_dot_loss_f32 (P with inline negatives, P^T, NT), the sums and the
    whole head (link_predictor.loss_backward) on random embeddings;
  * next to each loss launch mggcn_gat_backward_dst_f32 at ONE head on the same pattern and width, from the same run: it
    also does one gather, one dot and one axpy-sized pass per entry (it sums a scalar where the link kernel sums a row);
  * the link epochs of gcn and sage(aggr="mean"), [608, 128, 128, d], next to their node-classification epochs.
Device events after a warm-up, medians of SAMPLES samples.  A manual script, not a test; not to be run under a profiler.
Usage: python profiles/experiments/link.py [--no-epochs]"""
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
SAMPLES = 7
ADAM = (1e-2, 0.9, 0.999, 5e-4, 1e-8)


def sample(fn):
    ctx.record("exp-begin", 0)
    fn()
    ctx.record("exp-end", 0)
    ctx.sync()
    return float(lib.mggcn_event_elapsed_ms(ctx.events["exp-begin"], ctx.events["exp-end"]))


def timed(fn):
    sample(fn)                                                   # warm-up: code objects, caches
    v = [sample(fn) for _ in range(SAMPLES)]
    return f"{statistics.median(v):8.3f} ms (min {min(v):.3f}, max {max(v):.3f})"


class encoder_stub(pkg.gcn):
    """only what link_predictor's constructor reads: the head is measured without an encoder"""

    def __init__(self, n, d):
        self.A, self._out_width = type("rows", (), {"n": staticmethod(lambda: n)}), d


t0 = time.time()
(ip, ix, dv), Xh, Yh = pkg.datasets.synth_reddit_like(1.0, seed=1)
n, M = ip.shape[0] - 1, int(ip[-1])
print(f"[graph] n {n}, M = nnz {M}, R 1; built in {time.time() - t0:.1f} s on the host", flush=True)
rng = np.random.default_rng(0)

for d in (128, 41):
    P = pkg.csr_matrix(ip, ix, dv.copy(), n)
    head = pkg.link_predictor(encoder_stub(n, d), P, neg_ratio=1, seed=1)
    H = dn.from_numpy((rng.standard_normal((n, d)) * d ** -0.25).astype(np.float32))      # scores of standard deviation 1
    head.loss_backward(ctx, H)
    ctx.sync()
    (keys, vals, ka, va), work = head._arrays
    r, (pp, px, _), (tp, tx, _) = head._rows, P.device(ctx.device), head.P_T.device(ctx.device)
    w = 1.0 / M
    print(f"[d = {d}] loss {head.read()[0]:.4f}, acc {head.read()[1]:.4f}")
    print(f"  draw          {timed(lambda: ops.link_neg_draw(ctx, n, pp, M, n, 1, 1, 0, keys, vals))}")
    print(f"  sort          {timed(lambda: ops.radix_sort_pairs(ctx, 1, M, keys, vals, ka, va, work, 0, head.sort_bits()))}")
    print(f"  bounds        {timed(lambda: ops.link_bounds(ctx, keys, M, n, r['nt_indptr']))}")
    launches = (("loss (a) P+neg", pp, px, dict(positive=True, weight=w, neg_ratio=1, neg_weight=w, seed=1, epoch=0,
                                                 row_loss=r["row_loss"], row_correct=r["row_correct"])),
                ("loss (b) P^T  ", tp, tx, dict(positive=True, weight=w, beta=1.0)),
                ("loss (c) NT   ", r["nt_indptr"], vals, dict(positive=False, weight=w, beta=1.0)))
    for name, a, b, kw in launches:
        print(f"  {name} {timed(lambda: ops.link_dot_loss(ctx, n, n, a, b, M, H, r['G'], **kw))}")
    print(f"  sums          {timed(lambda: ops.link_sums(ctx, r['row_loss'], r['row_correct'], n, r['sums']))}")
    print(f"  whole head    {timed(lambda: head.loss_backward(ctx, H))}")
    # the one-head attention backward over the rows of the same patterns (NT is this epoch's draw: the sampled_csr of the head)
    s1 = [dn.from_numpy(rng.standard_normal((n, 1)).astype(np.float32)) for _ in range(3)]
    D, ds, out = dn(n, 1), dn(n, 1), dn.from_numpy(rng.standard_normal((n, d)).astype(np.float32))
    for name, F in (("P  ", P), ("P^T", head.P_T)):
        print(f"  gat_backward_dst on {name} {timed(lambda: ops.gat_backward_dst(ctx, F, H, s1[0], s1[1], s1[2], out, out, D, ds, 1))}")
    del head, H, out
    import torch
    torch.cuda.empty_cache()

if "--no-epochs" not in sys.argv:
    X, Y = dn.from_numpy(Xh), dn.from_numpy(Yh.reshape(-1, 1).astype(np.int32))
    for name, make in (("gcn", pkg.gcn), ("sage(mean)", lambda A, s: pkg.sage(A, s, aggr="mean"))):
        for d in (128, 41):
            sizes = [Xh.shape[1], 128, 128, d]
            model = make(pkg.csr_matrix(ip, ix, dv.copy(), n), sizes)
            head = pkg.link_predictor(model, pkg.csr_matrix(ip, ix, dv.copy(), n))
            print(f"[epoch] {name} {sizes}: link {timed(lambda: head.train_step(ctx, X, *ADAM))}"
                  + (f"; node classification {timed(lambda: model.train_step(ctx, X, Y, *ADAM))}" if d == 41 else ""), flush=True)
            del model, head
            torch.cuda.empty_cache()
