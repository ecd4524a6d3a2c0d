"""The split-aware fused loss (mggcn_softmax_xent_split_from_f32) against the plain one (mggcn_softmax_xent_fused_from_f32,
the yardstick: unchanged), and one Reddit-shaped epoch with splits on and off.  One JSON line on stdout.

  * per call: same process, same logits, [232 968 x 41] and [232 968 x 48], S with the Reddit proportions (66 % train /
    10 % validation / 24 % test); HIP events on the compute stream, 5 warm-up calls, then REPS rounds that alternate
    plain / split; medians, and the spread (min, max, quartiles) of each -- the margin a difference has to beat.  Out of
    place (G != logits) and in place.
  * the epoch: gcn(fused=True) on the asymmetric Reddit stand-in, train_step timed by the host clock (it ends in a
    synchronise), blocks of epochs with set_splits(S) and set_splits(None) alternating; median per mode and spread.
Usage: python profiles/experiments/split_loss.py [--reps 20] [--no-epoch]"""
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


def stats(x):
    x = np.asarray(x, dtype=np.float64)
    q = np.percentile(x, [0, 25, 50, 75, 100])
    return {"median": float(q[2]), "min": float(q[0]), "q1": float(q[1]), "q3": float(q[3]), "max": float(q[4])}


def kernel_part(pkg, ctx, reps):
    import torch
    lib = ctx.lib
    a, b = lib.mggcn_event_create(), lib.mggcn_event_create()
    n = 232_968
    rng = np.random.default_rng(0)
    S = rng.choice(3, size=n, p=(0.66, 0.10, 0.24)).astype(np.int32)
    out = {}
    for m in (41, 48):
        H = torch.from_numpy(rng.standard_normal((n, m), dtype=np.float32) * np.float32(3.0)).cuda()
        Y = torch.from_numpy(rng.integers(0, 41, n).astype(np.int32)).cuda()
        Sd = torch.from_numpy(S).cuda()
        G = torch.empty_like(H)
        Hi = H.clone()
        sums = torch.zeros(8, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        gs = float(np.float32(1.0 / n))
        gs_t = float(np.float32(1.0 / int((S == 0).sum())))

        def timed(fn):
            lib.mggcn_event_record(a, ctx.stream(0))
            fn()
            lib.mggcn_event_record(b, ctx.stream(0))
            lib.mggcn_event_synchronize(b)
            return lib.mggcn_event_elapsed_ms(a, b) * 1e3

        for where, src, dst in (("out_of_place", H, G), ("in_place", Hi, Hi)):
            def plain():
                lib.mggcn_softmax_xent_fused_from_f32(ctx.stream(0), src.data_ptr(), dst.data_ptr(), Y.data_ptr(), n, m, gs,
                                                      sums.data_ptr())

            def split():
                lib.mggcn_softmax_xent_split_from_f32(ctx.stream(0), src.data_ptr(), dst.data_ptr(), Y.data_ptr(),
                                                      Sd.data_ptr(), n, m, 0, gs_t, sums.data_ptr())
            for _ in range(5):
                plain(); split()
            ctx.sync()
            tp, ts = [], []
            for _ in range(reps):
                tp.append(timed(plain))
                ts.append(timed(split))
            sp, ss = stats(tp), stats(ts)
            bytes_plain, bytes_split = n * (8 * m + 4), n * (8 * m + 8)
            out[f"m{m}_{where}"] = {
                "plain_us": sp, "split_us": ss, "split_over_plain": ss["median"] / sp["median"],
                "expected_from_bytes": bytes_split / bytes_plain,
                "plain_GBps": bytes_plain / sp["median"] / 1e3, "split_GBps": bytes_split / ss["median"] / 1e3}
            log(f"m={m} {where}: plain {sp['median']:.2f} us [{sp['min']:.2f}, {sp['max']:.2f}]  split {ss['median']:.2f} us "
                f"[{ss['min']:.2f}, {ss['max']:.2f}]  ratio {ss['median'] / sp['median']:.4f} (bytes: {bytes_split / bytes_plain:.4f})")
    return out


def epoch_part(pkg, ctx, reps):
    (ip, ix, dv), X, Y = pkg.datasets.synth_reddit_like(1.0, seed=1)
    n = ip.shape[0] - 1
    sizes = [X.shape[1], 128, 128, 128, 1 + int(Y.max())]
    G = pkg.gcn(pkg.csr_matrix(ip, ix, dv, n), sizes, fused=True)
    Xd, Yd = pkg.dn_matrix.from_numpy(X), pkg.dn_matrix.from_numpy(np.asarray(Y).reshape(-1, 1).astype(np.int32))
    S = np.random.default_rng(0).choice(3, size=n, p=(0.66, 0.10, 0.24)).astype(np.int32)
    Sd = pkg.dn_matrix.from_numpy(S.reshape(-1, 1))
    step = lambda: G.train_step(ctx, Xd, Yd, 1e-2, 0.9, 0.999, 5e-4, 1e-8)   # noqa: E731
    for _ in range(5):
        step()
    G.set_splits(Sd)
    for _ in range(3):
        step()
    t = {"off": [], "on": []}
    last = {}
    for block in range(4):
        for mode in ("off", "on"):
            G.set_splits(Sd if mode == "on" else None)
            step()
            for _ in range(max(reps // 4, 3)):
                t0 = time.perf_counter()
                last[mode] = step()
                t[mode].append((time.perf_counter() - t0) * 1e3)
    so, sn = stats(t["off"]), stats(t["on"])
    log(f"epoch: splits off {so['median']:.3f} ms [{so['min']:.3f}, {so['max']:.3f}]  on {sn['median']:.3f} ms "
        f"[{sn['min']:.3f}, {sn['max']:.3f}]; split metrics of the last epoch: {G.split_metrics()}")
    return {"n": int(n), "sizes": [int(x) for x in sizes], "off_ms": so, "on_ms": sn, "on_over_off": sn["median"] / so["median"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-epoch", action="store_true")
    args = ap.parse_args()
    pkg = ge.load_package()
    ctx = pkg.context(0)
    res = {"kernel": kernel_part(pkg, ctx, args.reps)}
    if not args.no_epoch:
        res["epoch"] = epoch_part(pkg, ctx, max(args.reps, 20))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
