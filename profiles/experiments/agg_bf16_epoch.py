"""Epochs of the default 3x128 model with agg_dtype="bf16" on the symmetric Reddit stand-in -- the target of a
rocprofv3 --kernel-trace --stats run (profiles/agg_bf16_epoch_kernel_stats.csv).
Usage: python profiles/experiments/agg_bf16_epoch.py [epochs] [f32|bf16]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import __graft_entry__ as ge  # noqa: E402

pkg = ge.load_package()
epochs = int(sys.argv[1]) if len(sys.argv) > 1 else 1
agg = sys.argv[2] if len(sys.argv) > 2 else "bf16"
(ip, ix, dv), X, Y = pkg.datasets.synth_reddit_like(1.0, seed=1, symmetric=True)
n = ip.shape[0] - 1
ctx = pkg.context(0)
G = pkg.gcn(pkg.csr_matrix(ip, ix, dv, n), [X.shape[1], 128, 128, 128, int(Y.max()) + 1], agg_dtype=agg)
Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
for e in range(epochs):
    print(agg, e, G.train_step(ctx, Xd, Yd, 1e-2, 0.9, 0.999, 5e-4, 1e-8), flush=True)
