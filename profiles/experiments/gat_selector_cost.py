"""What model_selector costs per epoch on the Reddit-shaped gat ([608, 128, 128, 128, 41], 4 heads, the stand-in of
profiles/experiments/gat.py at --scale, splits on), on the protocol of selector_cost.py: host wall time of an epoch
(train_step, which synchronises once) with the selector off, with clean=False (one stream-ordered copy of the parameters per
epoch: W, b and att of every layer) and with clean=True (one extra plain forward and loss-layer call per epoch).  One
process, one model object per form, the three forms alternating round by round so that clock and cache state drift hits them
alike; WARMUP epochs each first, then ROUNDS rounds of EPOCHS epochs; milliseconds per epoch as median / min / max over the
rounds, and each selector form's difference to the selector-off median of the same run.  One JSON line on stdout.
Usage: python profiles/experiments/gat_selector_cost.py [--scale 1.0] [--variant v1] [--rounds 5] [--epochs 5] [--warmup 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import __graft_entry__ as ge  # noqa: E402

ADAM = (1e-2, 0.9, 0.999, 5e-4, 1e-8)


def stats(x):
    x = np.asarray(x, dtype=np.float64)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--variant", default="v1")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    pkg = ge.load_package()
    ctx = pkg.context(0)
    (ip, ix, dv), X, Y = pkg.datasets.synth_reddit_like(args.scale, seed=1)
    n = ip.shape[0] - 1
    sizes = [X.shape[1], 128, 128, 128, int(Y.max()) + 1]
    S = np.random.default_rng(2).choice(3, size=n, p=(0.66, 0.10, 0.24)).astype(np.int32)
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    A = pkg.csr_matrix(ip, ix, dv, n)                            # gat neither uses nor changes the values: one matrix for all
    forms = {}
    for name in ("off", "clean_false", "clean_true"):
        G = pkg.gat(A, sizes, heads=4, variant=args.variant)
        G.set_splits(S)
        sel = None if name == "off" else pkg.model_selector(G, clean=(name == "clean_true"))
        step = (lambda G=G: G.train_step(ctx, Xd, Yd, *ADAM)) if sel is None else (lambda sel=sel: sel.step(ctx, Xd, Yd, *ADAM))
        for _ in range(args.warmup):
            step()
        forms[name] = step
    ms = {name: [] for name in forms}
    for _ in range(args.rounds):
        for name, step in forms.items():
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(args.epochs):
                step()
            ms[name].append((time.perf_counter() - t0) * 1e3 / args.epochs)
    parameters = int(sum(t.shape()[0] * t.shape()[1] for t in (getattr(o, p) for _, o, p, _, _ in pkg.checkpoint.model_params(G))))
    res = {"n": n, "nnz": int(ip[-1]), "sizes": sizes, "heads": G.heads, "variant": args.variant, "parameters": parameters,
           "rounds": args.rounds, "epochs_per_round": args.epochs, "epoch_ms": {k: stats(v) for k, v in ms.items()}}
    off = res["epoch_ms"]["off"]["median"]
    res["extra_ms_per_epoch"] = {k: res["epoch_ms"][k]["median"] - off for k in ("clean_false", "clean_true")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
