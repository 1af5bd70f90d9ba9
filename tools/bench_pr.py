#!/usr/bin/env python3
"""Precision / recall reductions micro-benchmark (csrc/prstats.hip): milliseconds per call of ops.dist_stats (500 bins) and
ops.dist_median over Q = 200 000 (one evaluation's cloud) and Q = 10^7 squared distances, the achieved GB/s against the 4 Q bytes of
dist2 (dist_stats reads them once, dist_median four times: its figure is per 4 Q bytes as well, so a quarter of what its loads achieve),
and beside each the torch operators eval_recon.py used before on the same GPU: sqrt / mean / compare / histc, and the two kthvalue calls
of a median.

Method: seeded gamma-distributed distances (mean 4 cm, a tail beyond the 25 cm of the last bin); HIP events around `--calls` back-to-back
calls on the current stream, allocation of workspace and outputs included, divided by the number of calls; `--warmup` untimed rounds,
then `--repeats` timed ones, the median.  Launches per call are what the C entry points issue: dist_stats one memset + 2 kernels,
dist_median one memset + 5 kernels.  A record, not a criterion.
usage: python tools/bench_pr.py [--repeats 7] [--warmup 2] [--calls 20] [--json FILE]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from cut3r_slam_amd import ops

TAU, BIN_WIDTH, NBINS = 0.05, 5e-4, 500


def timed(fn, warmup, repeats, calls):
    ts, out = [], None
    for r in range(warmup + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            out = fn()
        e1.record()
        torch.cuda.synchronize()
        if r >= warmup:
            ts.append(e0.elapsed_time(e1) / calls)
    return statistics.median(ts), out


def torch_stats(d2):
    d = d2.double().sqrt()
    return d.mean(), (d < TAU).double().mean(), torch.histc(d, NBINS, 0.0, NBINS * BIN_WIDTH)


def torch_median(d2):
    n = d2.numel()
    return torch.stack([d2.kthvalue((n - 1) // 2 + 1).values, d2.kthvalue(n // 2 + 1).values])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--json", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pr needs a GPU")
    dev = "cuda:0"
    out = {"repeats": args.repeats, "warmup": args.warmup, "calls": args.calls, "launches": {"dist_stats": 3, "dist_median": 6}, "sizes": {}}
    for Q in (200000, 10 ** 7):
        g = torch.Generator().manual_seed(Q)
        u = 1 - torch.rand(2, Q, generator=g, dtype=torch.float64)                  # gamma(2) = -(ln u1 + ln u2)
        d2 = (-0.02 * u.log().sum(0)).square().float().to(dev).contiguous()
        res = {"mbytes": 4 * Q / 1e6}
        t, (counts, moments, hist) = timed(lambda: ops.dist_stats(d2, TAU, BIN_WIDTH, NBINS), args.warmup, args.repeats, args.calls)
        t_ref, (mean, share, _) = timed(lambda: torch_stats(d2), args.warmup, args.repeats, args.calls)
        same = abs(float(moments[0]) / Q - float(mean)) < 1e-9 and int(counts[1]) == round(float(share) * Q)
        res["dist_stats"] = {"hip_ms": t, "gbytes_per_s": 4 * Q / t / 1e6, "torch_ms": t_ref, "ratio": t_ref / t,
                             "share_in_bins": int(hist.sum()) / Q, "agrees_with_torch": bool(same)}
        t, med = timed(lambda: ops.dist_median(d2), args.warmup, args.repeats, args.calls)
        t_ref, med_ref = timed(lambda: torch_median(d2), args.warmup, args.repeats, max(1, args.calls // 4))
        res["dist_median"] = {"hip_ms": t, "gbytes_per_s": 4 * Q / t / 1e6, "torch_ms": t_ref, "ratio": t_ref / t,
                              "agrees_with_torch": bool(torch.equal(med, med_ref))}
        for k in ("dist_stats", "dist_median"):
            r = res[k]
            print(f"Q = {Q:>8d} {k:11s}: HIP {r['hip_ms']:.4f} ms ({out['launches'][k]} launches), {r['gbytes_per_s']:.0f} GB/s of the "
                  f"{res['mbytes']:.1f} MB of dist2; torch operators {r['torch_ms']:.3f} ms: {r['ratio']:.1f}x; same result: {r['agrees_with_torch']}")
        out["sizes"][str(Q)] = res
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w", encoding="utf-8") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
