"""ROC-AUC on the device (metrics.roc_auc_evaluator: keys, the stable radix sort, the integer statistic) at two shapes:
the Reddit-shaped n = 232 968, C = 41 and the ogbn-proteins shape n = 132 534, C = 112.  One JSON line on stdout.

Per shape a gcn(loss="bce") is trained for a few epochs on a synthetic graph of that shape, so that the logits are a model's;
then, in the same process:
  keys / sort / stats   HIP events on the compute stream around each phase of one evaluator call (the evaluator's own
                        timers; the default workspace cap holds either shape in one group); the sort is four digit passes,
                        so a pass is a quarter of it.  Median, min and max over --reps calls.
  call                  a host clock around ev(ctx, logits, Y, S): the three phases, the synchronisation, the copy of
                        C x 15 integers and the Python arithmetic on them.
  model.roc_auc         the same with the plain forward in front.
  (a) host              the path it replaces: device-to-host copy of the logits plus the numpy restatement
                        (tests/auc_ref.py), timed once.  The integers of the two paths are compared: they must be equal.
  (b) epoch             train_step of the same gcn(loss="bce"), host clock, median over --reps.
  (c) floors            the bytes each phase must move over the HBM rate (--hbm-tbs, default the guide's achievable
                        6.3 TB/s): a sort pass reads and writes 16 B per pair and reads the 4-byte keys once more for the
                        histogram; keys reads 8 B (logit, target) and writes 8 B per pair; stats reads the values once
                        (count) and keys and values once (walk).
Usage: python profiles/experiments/roc_auc.py [--reps 7] [--epochs 3] [--hbm-tbs 6.3] [--shapes reddit,proteins]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
import auc_ref  # noqa: E402

ADAM = (1e-2, 0.9, 0.999, 5e-4, 1e-8)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def spread(x):
    x = np.asarray(x, dtype=np.float64)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max())}


def problem(pkg, name):
    """(csr, X, layer sizes) of the shape"""
    if name == "reddit":
        (ip, ix, dv), X, _ = pkg.datasets.synth_reddit_like(1.0, seed=1, symmetric=True)
        return (ip, ix, dv), X, [X.shape[1], 128, 128, 128, 41]
    n = 132_534                                                     # ogbn-proteins: 39.6 M undirected edges, 8 features
    ip, ix, dv = pkg.datasets.synth_symmetric_powerlaw_csr(n, 79_122_504 + n, 7_750, seed=3)
    X = np.random.default_rng(3).standard_normal((n, 8), dtype=np.float32)
    return (ip, ix, dv), X, [8, 128, 128, 128, 112]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--hbm-tbs", type=float, default=6.3)
    ap.add_argument("--shapes", default="reddit,proteins")
    args = ap.parse_args()
    pkg = ge.load_package()
    ctx = pkg.context(0)
    res = {"experiment": "roc_auc", "hbm_tbs": args.hbm_tbs, "tile": pkg.ops.RADIX_SORT_TILE, "chunk": pkg.ops.ROC_AUC_CHUNK}
    for name in args.shapes.split(","):
        t0 = time.perf_counter()
        csr, X, sizes = problem(pkg, name)
        n, C = X.shape[0], sizes[-1]
        rng = np.random.default_rng(1)
        Yh = (rng.random((n, C)) < 0.1).astype(np.int32)
        Sh = rng.choice(3, size=(n, 1), p=(0.66, 0.10, 0.24)).astype(np.int32)
        log(f"[{name}] n = {n}, C = {C}, nnz = {int(csr[0][-1])}: generated in {time.perf_counter() - t0:.1f} s")
        model = pkg.gcn(pkg.csr_matrix(*csr, n), sizes, loss="bce")
        model.set_splits(Sh)
        Xd, Yd, Sd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Yh), pkg.dn_matrix.from_numpy(Sh)
        for _ in range(args.epochs):                                # warm-up: plans, code objects
            loss = model.train_step(ctx, Xd, Yd, *ADAM)
        epoch = []
        for _ in range(args.reps):
            t = time.perf_counter()
            model.train_step(ctx, Xd, Yd, *ADAM)
            epoch.append((time.perf_counter() - t) * 1e3)
        logits = model(ctx, Xd)
        ctx.sync()
        ev = pkg.roc_auc_evaluator(n, C)
        assert ev.group == C
        got = ev(ctx, logits, Yd, Sd)                               # warm-up: allocation, code objects
        phases = {"keys": [], "sort": [], "stats": []}
        call, member = [], []
        for _ in range(args.reps):
            t = time.perf_counter()
            again = ev(ctx, logits, Yd, Sd)
            call.append((time.perf_counter() - t) * 1e3)
            for k in phases:
                phases[k].append(ctx.measure("roc-auc-" + k))
            assert again["stats"] == got["stats"]
        model.roc_auc(ctx, Xd, Yd)
        for _ in range(args.reps):
            t = time.perf_counter()
            model.roc_auc(ctx, Xd, Yd)
            member.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        host_logits = logits.numpy()
        copy_ms = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        want = auc_ref.stats(host_logits, Yh, Sh)
        numpy_ms = (time.perf_counter() - t) * 1e3
        assert got["stats"] == want, "the device integers differ from the host restatement"
        pairs = n * C
        floor_ms = {k: b * pairs / (args.hbm_tbs * 1e12) * 1e3 for k, b in (("keys", 16), ("sort_pass", 20), ("stats", 12))}
        out = {"n": n, "C": C, "pairs": pairs, "loss": float(loss[0]), "val_auc": got["val"], "test_auc": got["test"],
               "keys_ms": spread(phases["keys"]), "sort_ms": spread(phases["sort"]),
               "sort_pass_ms": spread(np.asarray(phases["sort"]) / 4), "stats_ms": spread(phases["stats"]),
               "call_ms": spread(call), "model_roc_auc_ms": spread(member),
               "host_copy_ms": copy_ms, "host_numpy_ms": numpy_ms, "epoch_ms": spread(epoch), "floor_ms": floor_ms,
               "workspace_bytes": ev.workspace_bytes(), "integers_equal_host": True}
        for k, f in (("keys", "keys"), ("sort_pass", "sort_pass"), ("stats", "stats")):
            out[f"{k}_over_floor"] = out[f"{k}_ms"]["median"] / floor_ms[f]
        res[name] = out
        log(f"[{name}] " + json.dumps(out))
        del model, ev, logits, Xd, Yd, Sd
    print(json.dumps(res))


if __name__ == "__main__":
    main()
