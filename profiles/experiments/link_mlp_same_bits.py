"""Do two builds of libmggcn_hip.so give the MLP link decoder the same bits?  One process per library: it loads
DIR/libmggcn_hip.so, runs the walk, the pairs and the ranking kernels of both operand types on seeded inputs and prints one line
per output buffer with zlib.crc32 of its bytes.  Two runs' lines are compared with diff, or pasted side by side.
  shapes   (d, hd) in (32, 32), (96, 64), (128, 128), (32, 128), fp32 and bf16
  step     the pattern of tests/test_gpu_link_mlp.py's "edges" graph (rows of 0, 1, 31, 32, 33, 64 and 65 entries, then 0 .. 4),
           R = 2: draw -> sort -> bounds, the three walk launches (P with its negatives drawn, P^T, the negatives' transpose),
           the training-list pairs launch: G, the row sums and hits, the four parameter gradients
  lists    explicit lists of 1, 32, 33 and 1000 pairs: out
  rank     K in 1, 31, 32, 33, 70 tails for 37 positives: counts
No device is an error, not a fallback.  A manual script, not a test.
Usage: python profiles/experiments/link_mlp_same_bits.py DIR [> log]"""
import os
import sys
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import __graft_entry__ as g

if len(sys.argv) != 2 or not os.path.exists(os.path.join(sys.argv[1], "libmggcn_hip.so")):
    sys.exit(__doc__)
if not torch.cuda.is_available():
    sys.exit("link_mlp_same_bits: no device")
pkg = g.load_package()
pkg._lib.LIB_PATH = os.path.join(os.path.abspath(sys.argv[1]), "libmggcn_hip.so")
ctx = pkg.context(0)
ops = pkg.ops
SEED, EPOCH, R = 0x1234_5678_9ABC, 7, 2
SHAPES = ((32, 32), (96, 64), (128, 128), (32, 128))


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def crc(what, t):
    ctx.sync()
    print(f"{what:44s} {zlib.crc32(t.contiguous().cpu().numpy().tobytes()):08x}", flush=True)


def edges():
    n, rng = 70, np.random.default_rng(5)
    lens = rng.integers(0, 5, size=n)
    lens[:7] = (0, 1, 31, 32, 33, 64, 65)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    indices = rng.integers(0, n, size=int(indptr[-1])).astype(np.uint32)
    indices[int(indptr[2]) + 1] = indices[int(indptr[2])]
    return n, indptr, indices


def transpose(indptr, indices, n):
    heads = np.repeat(np.arange(n, dtype=np.uint32), np.diff(indptr.astype(np.int64)))
    order = np.argsort(indices, kind="stable")
    t_ip = np.concatenate([[0], np.cumsum(np.bincount(indices, minlength=n))]).astype(np.uint32)
    return heads, t_ip, heads[order]


n, indptr, indices = edges()
M = int(indptr[-1])
heads, t_ip, t_ix = transpose(indptr, indices, n)
ip, ix, tip, tix, hd_ = (dev(a) for a in (indptr, indices, t_ip, t_ix, heads))
keys, vals, ka, va = (torch.empty(M * R, dtype=torch.int32, device="cuda") for _ in range(4))
work = torch.empty(ops.radix_sort_work_bytes(1, M * R) // 8 + 1, dtype=torch.int64, device="cuda")
nt = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda")
ctx.sync()
ops.link_neg_draw(ctx, n, ip, M, n, R, SEED, EPOCH, keys, vals)
ops.radix_sort_pairs(ctx, 1, M * R, keys, vals, ka, va, work, 0, max(1, (n - 1).bit_length()))
ops.link_bounds(ctx, keys, M * R, n, nt)
ctx.sync()

for dtype in ("fp32", "bf16"):
    b16 = dtype == "bf16"
    loss, pairs_op, rank = ((ops.link_mlp_loss_bf16, ops.link_mlp_pairs_bf16, ops.link_rank_mlp_bf16) if b16 else
                            (ops.link_mlp_loss, ops.link_mlp_pairs, ops.link_rank_mlp))
    for d, hd in SHAPES:
        rng = np.random.default_rng(100 * d + hd)
        tag = f"{dtype} {d}x{hd}"
        H = dev((rng.standard_normal((1000, d)) * d ** -0.25).astype(np.float32))
        W1, b1, w2, b2 = (dev(a.astype(np.float32)) for a in (
            rng.standard_normal((d, hd)) / np.sqrt(d), rng.standard_normal(hd) * 0.1, rng.standard_normal(hd) / np.sqrt(hd),
            rng.standard_normal(1) * 0.1))
        ctx.sync()
        if b16:
            Hb = torch.empty((1000, d), dtype=torch.bfloat16, device="cuda")
            image = torch.empty(ops.link_mlp_image_halves(d, hd), dtype=torch.bfloat16, device="cuda")
            ctx.sync()
            ops.convert_bf16(ctx, H, Hb)
            ops.link_mlp_pack_bf16(ctx, W1, image)
            X, params = Hb, (image, b1, w2, b2)
        else:
            X, params = H, (W1, b1, w2, b2)
        # ---- a step on the first n rows
        G = torch.full((n, d), float("nan"), device="cuda")
        row_loss, row_correct = torch.empty(2 * n, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
        grads = torch.full((ops.link_mlp_grad_floats(d, hd),), float("nan"), device="cuda")
        partials = torch.full((ops.link_mlp_partial_floats(d, hd),), float("nan"), device="cuda")
        ctx.sync()
        loss(ctx, n, n, ip, ix, M, X[:n], params, G, True, 1.0 / M, R, 1.0 / (M * R), SEED, EPOCH, 0.0, row_loss, row_correct)
        crc(f"{tag} walk P: G", G)
        loss(ctx, n, n, tip, tix, M, X[:n], params, G, True, 1.0 / M, beta=1.0)
        crc(f"{tag} walk P^T: G", G)
        loss(ctx, n, n, nt, vals, M * R, X[:n], params, G, False, 1.0 / (M * R), beta=1.0)
        crc(f"{tag} walk negatives^T: G", G)
        crc(f"{tag} row sums", row_loss)
        crc(f"{tag} row hits", row_correct)
        pairs_op(ctx, X[:n], params, train=(hd_, ix, M, R, n, SEED, EPOCH), weight=1.0 / M, neg_weight=1.0 / (M * R),
                 grads=grads, partials=partials)
        cuts = np.cumsum([0, d * hd, hd, hd, 1])
        for name, lo, hi in zip(("G_W1", "G_b1", "G_w2", "G_b2"), cuts[:-1], cuts[1:]):
            crc(f"{tag} training list: {name}", grads[lo:hi])
        # ---- explicit lists
        for m in (1, 32, 33, 1000):
            src, dst = (dev(rng.integers(0, 1000, size=m).astype(np.uint32)) for _ in range(2))
            out = torch.full((m + 40,), float("nan"), device="cuda")
            ctx.sync()
            pairs_op(ctx, X, params, pairs=(src, dst, m), out=out)
            crc(f"{tag} list of {m}: out", out)
        # ---- ranking
        for K in (1, 31, 32, 33, 70):
            mp = 37
            src, dst = (dev(rng.integers(0, 1000, size=mp).astype(np.uint32)) for _ in range(2))
            tails = dev(rng.integers(0, 1000, size=mp * K).astype(np.uint32))
            counts = torch.full((2 * mp,), -1, dtype=torch.int32, device="cuda")
            ctx.sync()
            rank(ctx, src, dst, mp, tails, K, X, params, counts)
            crc(f"{tag} rank K={K}: counts", counts)
