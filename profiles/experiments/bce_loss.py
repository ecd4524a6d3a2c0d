"""The fused sigmoid-BCE loss (mggcn_sigmoid_bce_from_f32) against the split-aware softmax loss
(mggcn_softmax_xent_split_from_f32, the yardstick: unchanged) at the logits shapes of the multi-label graphs:
[716 847 x 100] (Yelp) and [132 534 x 112] (ogbn-proteins), splits on (66 % train / 10 % validation / 24 % test), out of
place.  One JSON line on stdout.

Same process, same logits; HIP events on the compute stream around a WINDOW of back-to-back calls (tens of milliseconds:
event resolution and launch gaps drop out), 3 warm-up windows, then REPS rounds that alternate the two; microseconds per call
(median over the windows, with min and max), algorithmic bytes -- 3 x 4 x n x m for the BCE pass (logits, targets,
gradient), 2 x 4 x n x m for the softmax pass (logits, gradient; the n labels and sets are left out of both) -- and GB/s.
Usage: python profiles/experiments/bce_loss.py [--reps 10] [--window-ms 30]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import __graft_entry__ as ge  # noqa: E402

SHAPES = {"yelp": (716_847, 100), "ogbn-proteins": (132_534, 112)}


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def stats(x):
    x = np.asarray(x, dtype=np.float64)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--window-ms", type=float, default=30.0)
    args = ap.parse_args()
    import torch
    pkg = ge.load_package()
    ctx = pkg.context(0)
    lib = ctx.lib
    a, b = lib.mggcn_event_create(), lib.mggcn_event_create()
    res = {}
    for name, (n, m) in SHAPES.items():
        rng = np.random.default_rng(0)
        S = rng.choice(3, size=n, p=(0.66, 0.10, 0.24)).astype(np.int32)
        H = torch.from_numpy(rng.standard_normal((n, m), dtype=np.float32) * np.float32(3.0)).cuda()
        T = torch.from_numpy((rng.random((n, m)) < 0.1).astype(np.int32)).cuda()
        Y = torch.from_numpy(rng.integers(0, m, n).astype(np.int32)).cuda()
        Sd = torch.from_numpy(S).cuda()
        G = torch.empty_like(H)
        sums = torch.zeros(16, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        n_train = int((S == 0).sum())
        gs_bce, gs_soft = float(np.float32(1.0 / (n_train * m))), float(np.float32(1.0 / n_train))

        def bce():
            lib.mggcn_sigmoid_bce_from_f32(ctx.stream(0), H.data_ptr(), G.data_ptr(), T.data_ptr(), Sd.data_ptr(), n, m, 0, gs_bce,
                                           sums.data_ptr())

        def soft():
            lib.mggcn_softmax_xent_split_from_f32(ctx.stream(0), H.data_ptr(), G.data_ptr(), Y.data_ptr(), Sd.data_ptr(), n, m, 0,
                                                  gs_soft, sums.data_ptr())

        def window(fn, calls):
            lib.mggcn_event_record(a, ctx.stream(0))
            for _ in range(calls):
                fn()
            lib.mggcn_event_record(b, ctx.stream(0))
            lib.mggcn_event_synchronize(b)
            return lib.mggcn_event_elapsed_ms(a, b) * 1e3 / calls

        calls = {}
        for what, fn in (("bce", bce), ("softmax", soft)):
            one = window(fn, 10)                                   # first look, also the first warm-up
            calls[what] = max(10, int(args.window_ms * 1e3 / max(one, 1.0)))
            for _ in range(3):
                window(fn, calls[what])
        t = {"bce": [], "softmax": []}
        for _ in range(args.reps):
            t["bce"].append(window(bce, calls["bce"]))
            t["softmax"].append(window(soft, calls["softmax"]))
        sb, ss = stats(t["bce"]), stats(t["softmax"])
        bytes_bce, bytes_soft = 3 * 4 * n * m, 2 * 4 * n * m
        res[name] = {"n": n, "m": m, "calls_per_window": calls, "bce_us": sb, "softmax_us": ss,
                     "bce_bytes": bytes_bce, "softmax_bytes": bytes_soft,
                     "bce_GBps": bytes_bce / sb["median"] / 1e3, "softmax_GBps": bytes_soft / ss["median"] / 1e3,
                     "bce_over_softmax": sb["median"] / ss["median"], "expected_from_bytes": bytes_bce / bytes_soft}
        log(f"{name} [{n} x {m}]: bce {sb['median']:.2f} us [{sb['min']:.2f}, {sb['max']:.2f}] {res[name]['bce_GBps']:.0f} GB/s "
            f"({calls['bce']} calls per window);  softmax split {ss['median']:.2f} us [{ss['min']:.2f}, {ss['max']:.2f}] "
            f"{res[name]['softmax_GBps']:.0f} GB/s ({calls['softmax']} calls per window);  ratio "
            f"{res[name]['bce_over_softmax']:.3f} (bytes: 1.5)")
        del H, T, Y, G
    print(json.dumps(res))


if __name__ == "__main__":
    main()
