"""What link_predictor.rank's kernels cost, all three decoders in one process at d = 128, hidden = 128 on
embeddings of the Reddit-shaped stand-in's size (n = 232 965):
  per-positive   m = 86 596 positives with K = 1000 tails each (ogbl-citation2's validation shape): the fused kernel next to what
                 a user composes today -- the pair kernel over the m (1 + K) explicit pairs, the copy of the scores to the host,
                 the counting in numpy -- and its distance from the gather floor m K d (4 or 2 bytes) at the 8.7 TB/s DESIGN.md
                 takes for random rows.  The counts of the two routes are compared, integer for integer.
  shared         m = 60 000 positives against m_neg = 100 000: scores, keys, sort and the two bisections.
Device events after a warm-up, medians of SAMPLES samples; the host's part of the composition is timed once with a wall clock.
A manual script, not a test; not to be run under a profiler.  Usage: python profiles/experiments/link_rank.py"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import __graft_entry__ as g

pkg = g.load_package()
ctx = pkg.context(0)
lib, ops = ctx.lib, pkg.ops
SAMPLES, RATE = 7, 8.7e12
N, D, HD, M, K = 232_965, 128, 128, 86_596, 1000


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


def fmt(t):
    return f"{t[0]:9.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


rng = np.random.default_rng(0)
H = pkg.dn_matrix.from_numpy((rng.standard_normal((N, D)) * D ** -0.25).astype(np.float32))
W1, b1, w2, b2 = (pkg.dn_matrix.from_numpy(a.astype(np.float32)) for a in (
    rng.standard_normal((D, HD)) / np.sqrt(D), rng.standard_normal((1, HD)) * 0.1, rng.standard_normal((1, HD)) / np.sqrt(HD),
    rng.standard_normal((1, 1)) * 0.1))
Hb = torch.empty((N, D), dtype=torch.bfloat16, device="cuda")
image = torch.empty(ops.link_mlp_image_halves(D, HD), dtype=torch.bfloat16, device="cuda")
ctx.sync()
ops.convert_bf16(ctx, H, Hb)
ops.link_mlp_pack_bf16(ctx, W1, image)

pos = rng.integers(0, N, (M, 2), dtype=np.int64).astype(np.uint32)
tails = rng.integers(0, N, (M, K), dtype=np.int64).astype(np.uint32)
tails[:, 0] = pos[:, 1]
src, dst, tl = dev(pos[:, 0]), dev(pos[:, 1]), dev(tails.reshape(-1))
flat_u = dev(np.repeat(pos[:, 0], 1 + K))
flat_v = dev(np.concatenate([pos[:, 1:2], tails], axis=1).reshape(-1))
counts = torch.empty(2 * M, dtype=torch.int32, device="cuda")
scores = torch.empty(M * (1 + K), device="cuda")
ctx.sync()
decoders = (
    ("dot", 4, lambda: ops.link_rank_dot(ctx, src, dst, M, tl, K, H, counts),
     lambda: ops.edge_dot(ctx, flat_u, flat_v, M * (1 + K), H, scores)),
    ("mlp fp32", 4, lambda: ops.link_rank_mlp(ctx, src, dst, M, tl, K, H, (W1, b1, w2, b2), counts),
     lambda: ops.link_mlp_pairs(ctx, H, (W1, b1, w2, b2), pairs=(flat_u, flat_v, M * (1 + K)), out=scores)),
    ("mlp bf16", 2, lambda: ops.link_rank_mlp_bf16(ctx, src, dst, M, tl, K, Hb, (image, b1, w2, b2), counts),
     lambda: ops.link_mlp_pairs_bf16(ctx, Hb, (image, b1, w2, b2), pairs=(flat_u, flat_v, M * (1 + K)), out=scores)),
)
print(f"[per-positive] n {N}, d {D}, hidden {HD}, m {M}, K {K}: {M * K / 1e6:.1f} M negatives", flush=True)
for name, elem, fused, flat in decoders:
    t_fused, t_flat = timed(fused), timed(flat)
    got = counts.cpu().numpy().reshape(M, 2)
    t0 = time.perf_counter()
    s = scores.cpu().numpy().reshape(M, 1 + K)
    t1 = time.perf_counter()
    want = np.stack([(s[:, 1:] > s[:, :1]).sum(1), (s[:, 1:] == s[:, :1]).sum(1)], axis=1)
    t2 = time.perf_counter()
    floor = 1e3 * M * K * D * elem / RATE
    print(f"  {name:9s} fused {fmt(t_fused)} | gather floor {floor:7.3f} ms, x{t_fused[0] / floor:.2f}", flush=True)
    print(f"  {'':9s} today: pair kernel {fmt(t_flat)} + copy back {1e3 * (t1 - t0):.0f} ms + numpy counts {1e3 * (t2 - t1):.0f} ms"
          f" = {t_flat[0] + 1e3 * (t2 - t0):.0f} ms, x{(t_flat[0] + 1e3 * (t2 - t0)) / t_fused[0]:.1f} of the fused kernel;"
          f" fused / pair kernel {t_fused[0] / t_flat[0]:.3f}; counts equal: {bool((got == want).all())}"
          f" ({int((got != want).any(axis=1).sum())} rows differ), ties beyond the planted one: {int(want[:, 1].sum()) - M}", flush=True)
del scores, flat_u, flat_v, tl
torch.cuda.empty_cache()

m, m_neg = 60_000, 100_000
pairs = rng.integers(0, N, (m + m_neg, 2), dtype=np.int64).astype(np.uint32)
u, v = dev(pairs[:, 0]), dev(pairs[:, 1])
out = torch.empty((m + m_neg, 1), device="cuda")
keys, vals, ka, va = (torch.empty(m_neg, dtype=torch.int32, device="cuda") for _ in range(4))
work = torch.empty(ops.radix_sort_work_bytes(1, m_neg) // 8 + 1, dtype=torch.int64, device="cuda")
zeros = torch.zeros((m_neg, 1), dtype=torch.int32, device="cuda")
cnt = torch.empty(2 * m, dtype=torch.int32, device="cuda")
ctx.sync()
print(f"[shared] m {m}, m_neg {m_neg}", flush=True)
stages = (("scores (edge_dot)", lambda: ops.edge_dot(ctx, u, v, m + m_neg, H, out.view(-1))),
          ("keys", lambda: ops.roc_auc_keys(ctx, out[m:], zeros, None, 0, 1, keys, vals)),
          ("sort", lambda: ops.radix_sort_pairs(ctx, 1, m_neg, keys, vals, ka, va, work)),
          ("two bisections", lambda: ops.link_rank_sorted(ctx, out.view(-1)[:m], m, keys, m_neg, cnt)))
for name, fn in stages:                                          # in order: each stage leaves the next one's input
    print(f"  {name:18s} {fmt(timed(fn))}", flush=True)
s = out.cpu().numpy().reshape(-1)
t0 = time.perf_counter()
order = np.sort(s[m:])
want = np.stack([m_neg - np.searchsorted(order, s[:m], "right"),
                 np.searchsorted(order, s[:m], "right") - np.searchsorted(order, s[:m], "left")], axis=1)
print(f"  numpy on the host  {1e3 * (time.perf_counter() - t0):.1f} ms after the copy; counts equal: "
      f"{bool((cnt.cpu().numpy().reshape(m, 2) == want).all())}", flush=True)
