"""bf16 aggregation against fp32 on the symmetric Reddit stand-in and the products-shaped graph: one JSON line.

  * per call (HIP events on the compute stream, 3 warm-up + REPS timed calls, medians): the d = 128 forward matrix
    (A^T of the normalised graph), the d = 128 backward matrix (A), the d = 41 logits call (narrow plan) -- fp32 SpMM,
    bf16 SpMM alone, and the fp32 -> bf16 conversion pass it needs;
  * the default 3x128 model (gcn(fused=True)), fp32 and agg_dtype="bf16": epochs 0..19 from the same seed-99 init
    (loss, accuracy: the precision cost), epoch time = median of epochs 3..19 (HIP events around train_step);
  * the products-shaped d = 128 call, both ways.
Usage: python profiles/experiments/agg_bf16.py [--reps 20] [--no-products]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import __graft_entry__ as ge  # noqa: E402


def log(*a):
    print(*a, file=sys.stderr, flush=True)


class Timer:
    def __init__(self, ctx):
        self.ctx, self.lib = ctx, ctx.lib
        self.a, self.b = self.lib.mggcn_event_create(), self.lib.mggcn_event_create()

    def ms(self, fn, warmup=3, reps=20):
        for _ in range(warmup):
            fn()
        out = []
        for _ in range(reps):
            self.lib.mggcn_event_record(self.a, self.ctx.stream(0))
            fn()
            self.lib.mggcn_event_record(self.b, self.ctx.stream(0))
            self.lib.mggcn_event_synchronize(self.b)
            out.append(self.lib.mggcn_event_elapsed_ms(self.a, self.b))
        return float(np.median(out))


def call_times(pkg, ctx, timer, M, d, d_hint, reps):
    import torch
    n_cols = M.m()
    plan = pkg.ops.spmm_plan_for(ctx, M, max(d, 128), d_hint)
    g = torch.Generator(device="cuda").manual_seed(d)
    B = pkg.dn_matrix(n_cols, d, torch.randn(n_cols * d, device="cuda", generator=g))
    B16 = torch.empty((n_cols, d), dtype=torch.bfloat16, device="cuda")
    C = pkg.dn_matrix(M.n(), d)
    f32 = timer.ms(lambda: pkg.matmul(ctx, M, B, C, plan, 1.0, 0.0), reps=reps)
    conv = timer.ms(lambda: pkg.ops.convert_bf16(ctx, B, B16), reps=reps)
    b16 = timer.ms(lambda: pkg.ops.spmm_bf16(ctx, M, B16, C, plan, 1.0, 0.0), reps=reps)
    form = plan.describe().split(" form=")[1].split()[0]
    return {"f32_ms": round(f32, 4), "bf16_spmm_ms": round(b16, 4), "convert_ms": round(conv, 4),
            "bf16_ms": round(b16 + conv, 4), "form": form}


def train(pkg, ctx, timer, ip, ix, dv, n, X, Y, sizes, agg, epochs=20):
    G = pkg.gcn(pkg.csr_matrix(ip, ix, dv.copy(), n), sizes, fused=True, agg_dtype=agg)
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(Y)
    hist, ms = [], []
    for e in range(epochs):
        box = {}
        t = timer.ms(lambda: box.setdefault("r", G.train_step(ctx, Xd, Yd, 1e-2, 0.9, 0.999, 5e-4, 1e-8)), warmup=0, reps=1)
        hist.append([round(float(box["r"][0]), 6), round(float(box["r"][1]), 6)])
        if e >= 3:
            ms.append(t)
        log(f"{agg} epoch {e}: loss {hist[-1][0]} acc {hist[-1][1]} {t:.3f} ms")
    return G, hist, float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-products", action="store_true")
    args = ap.parse_args()
    pkg = ge.load_package()
    ctx = pkg.context(0)
    timer = Timer(ctx)
    t0 = time.time()
    (ip, ix, dv), X, Y = pkg.datasets.synth_reddit_like(1.0, seed=1, symmetric=True)
    n = ip.shape[0] - 1
    sizes = [X.shape[1], 128, 128, 128, int(Y.max()) + 1]
    log(f"stand-in: n {n} nnz {int(ip[-1])} sizes {sizes} ({time.time() - t0:.1f} s)")
    out = {"experiment": "agg_bf16", "graph": "reddit_like symmetric (synth_reddit_like(1.0, seed=1, symmetric=True))",
           "n": int(n), "nnz": int(ip[-1]), "sizes": sizes, "reps": args.reps, "stat": "median"}

    res = {}
    for agg in ("f32", "bf16"):
        G, hist, ms = train(pkg, ctx, timer, ip, ix, dv, n, X, Y, sizes, agg)
        res[agg] = (G, hist, ms)
    out["epoch_ms"] = {"f32": round(res["f32"][2], 3), "bf16": round(res["bf16"][2], 3),
                       "ratio": round(res["bf16"][2] / res["f32"][2], 3)}
    out["loss_acc_epochs_0_19"] = {"f32": res["f32"][1], "bf16": res["bf16"][1]}
    # the bf16 model's matrices (normalised A and A^T) for the per-call legs; fp32 and bf16 share the plans
    G = res["bf16"][0]
    del res
    out["calls"] = {
        "fwd_d128": call_times(pkg, ctx, timer, G.A_T, 128, 128, args.reps),
        "bwd_d128": call_times(pkg, ctx, timer, G.A, 128, 128, args.reps),
        "fwd_d41": call_times(pkg, ctx, timer, G.A_T, 41, 41, args.reps),
    }
    for k, v in out["calls"].items():
        v["ratio"] = round(v["bf16_ms"] / v["f32_ms"], 3)
        log(k, v)
    del G
    if not args.no_products:
        import torch
        torch.cuda.empty_cache()
        t0 = time.time()
        (pp, px, pv), _, _ = pkg.datasets.synth_products_like(1.0, seed=5, symmetric=True)
        pn = pp.shape[0] - 1
        P = pkg.csr_matrix(pp, px, pv, pn)
        P.normalize(True)
        log(f"products: n {pn} nnz {int(pp[-1])} ({time.time() - t0:.1f} s)")
        v = call_times(pkg, ctx, timer, P, 128, 128, max(10, args.reps // 2))
        v["ratio"] = round(v["bf16_ms"] / v["f32_ms"], 3)
        v["n"], v["nnz"] = int(pn), int(pp[-1])
        out["calls"]["products_d128"] = v
        log("products_d128", v)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
