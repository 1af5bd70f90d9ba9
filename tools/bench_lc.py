#!/usr/bin/env python3
"""Loop-closure optimiser (cut3r_lc_optimize: fused Adam over per-submap se(3) corrections, track_backend.py:256-299): iterations/s
and the fraction of the HBM roof for B submaps of N = 192 x 256 points.  Algorithmic traffic per iteration: 2 * B * N * 12
bytes (the last pointmap of submap b and the first of submap b+1), read once by the fused accumulate kernel.

--group sim3: the sim(3) optimisers (cut3r_lc_optimize_sim3 / cut3r_lc_optimize_terms_sim3) against the se(3) ones in the SAME process at
the production shape (12 submaps of 192 x 256, 2000 iterations): the chain form and the later-loop term list (12 submaps + 2 lc submaps:
11 + 2 + 2 terms), the two groups alternating, REPS timed calls each after a warm-up; median and min..max per group.  The accumulate launch
is the same code in both, so a difference beyond the se(3) spread is the Adam kernel's (one wave per transform: 7 instead of 6 dual
components through exp and matrix)."""
import argparse
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cut3r_slam_amd import ops

dev = "cuda:0"
h, w = 192, 256
N = h * w


def _maps(B, seed):
    g = torch.Generator().manual_seed(seed)
    sub = (torch.randn(B, 6, h, w, 3, generator=g) * 0.5 + 2.0).to(dev).contiguous()
    sub[1:, 0] = sub[:-1, 5] + 0.01 * torch.randn(B - 1, h, w, 3, generator=g).to(dev)       # consecutive submaps share a keyframe
    cur = sub[-1, 5].reshape(-1, 3).contiguous()
    cur_lc = (cur + 0.02).contiguous()
    return sub, cur, cur_lc, g


def _timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def roofline():
    iters = 1000
    for B in (20, 80, 200):
        sub, cur, cur_lc, _ = _maps(B, B)
        ops.lc_optimize(sub, None, cur, cur_lc, 10)
        torch.cuda.synchronize()
        ms = _timed(lambda: ops.lc_optimize(sub, None, cur, cur_lc, iters))
        byt = 2.0 * B * N * 12
        print(f"B={B:4d}: {iters} iterations in {ms:8.1f} ms = {iters / ms * 1e3:8.0f} iterations/s, {ms * 1e3 / iters:6.1f} us per iteration, "
              f"{byt / 1e6:6.1f} MB per iteration -> {byt * iters / ms / 1e9:6.2f} TB/s = {byt * iters / ms / 1e9 / 8.0:.3f} of 8 TB/s")


def compare_groups(iters, reps):
    B, Bc = 12, 2
    sub, cur, cur_lc, g = _maps(B, 12)
    sm, sc = [0, 1], [7, 11]
    lc_all = torch.stack([sub[m] + 0.002 * torch.randn(6, h, w, 3, generator=g).to(dev) for m in sm], 0).contiguous()
    pm_cur = torch.stack([sub[sc[0], 2], sub[sc[1], 4]], 0).contiguous()
    terms = [(sub[p, 5], p, sub[p + 1, 0], p + 1, 1.0 / (3 * (B - 1) * N), None) for p in range(B - 1)]
    terms += [(lc_all[k, 0], B + k, sub[sm[k], 0], sm[k], 1.0 / (3 * Bc * N), None) for k in range(Bc)]
    terms += [(pm_cur[k], sc[k], lc_all[k, 5], B + k, 1.0 / (3 * Bc * N), None) for k in range(Bc)]
    forms = {"chain": lambda grp: ops.lc_optimize(sub, None, cur, cur_lc, iters, group=grp),
             "later-loop terms": lambda grp: ops.lc_optimize_terms(terms, B + Bc, N, iters, group=grp)}
    for name, call in forms.items():
        for grp in ("se3", "sim3"):                                       # warm-up of both code objects at the timed shape
            call(grp)
        torch.cuda.synchronize()
        ms = {"se3": [], "sim3": []}
        for _ in range(reps):
            for grp in ("se3", "sim3"):
                ms[grp].append(_timed(lambda: call(grp)))
        med = {k: statistics.median(v) for k, v in ms.items()}
        for grp in ("se3", "sim3"):
            v = ms[grp]
            print(f"{name:17s} {grp:4s}: {iters} iterations, median {med[grp]:7.2f} ms = {med[grp] * 1e3 / iters:6.2f} us per iteration "
                  f"(min {min(v):7.2f}, max {max(v):7.2f} over {reps} calls)")
        print(f"{name:17s} sim3 / se3 = {med['sim3'] / med['se3']:.4f}; se3 spread (max - min) / median = "
              f"{(max(ms['se3']) - min(ms['se3'])) / med['se3']:.4f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--group", choices=("se3", "sim3"), default="se3", help="se3: the roofline table; sim3: sim(3) against se(3) at the production shape")
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_lc needs a GPU")
    if a.group == "sim3":
        compare_groups(a.iters, a.reps)
    else:
        roofline()
