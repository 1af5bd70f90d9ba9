#!/usr/bin/env python3
"""The nine-cell diagnostic panel (csrc/gs_panel.hip, ops.gs_panel: one range launch and one compose launch) at tracking resolution,
384 x 512, against the same composition written in torch tensor operations inside this tool (min / max reductions, the turbo gather,
the exposure product, the depth normal, the concatenations, the quantiser).  The parent commit has no panel to compare with.

Times: device events around synchronised work, after a warm-up; best and median of --reps.  With the kernel time the memory floor: the
fifteen fp32 input planes read twice at most (ranges + compose; 3 + 3 + 1 + 1 + 3 + 1 planes, the two depths and alpha also by the range
pass) and the 27 bytes a pixel of the panel written, at the measured 6.3 TB/s of the MI355X.  The torch composition must give the kernel's
bytes except where its own rounding (fused multiply-adds, reciprocal divisions) differs: the count of differing bytes is reported, not
asserted (tests/test_gs_panel_gpu.py pins the kernel to the numpy oracle instead).
usage: python tools/bench_panel.py [--size 384 512] [--reps 20] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from cut3r_slam_amd import ops

DEV = "cuda:0"
HBM_TBS = 6.3          # measured float4 copy rate of the MI355X


def timed(fn, reps):
    """(best, median) of reps in ms, by device events around fn (the stream is idle before and after), after one warm-up"""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return min(ts), statistics.median(ts)


def torch_panel(gt, render, A, b, gt_depth, depth, normal, alpha, fx, fy, cx, cy, table):
    """the panel in torch tensor operations, the reference's `viz` with the mapper's depth normal"""
    H, W = gt.shape[1:]

    def turbo(x):
        lo, hi = x.min(), x.max()
        den = (hi.double() - lo.double() + 1e-10).float()
        q = ((x - lo) / den).clamp(0, 1)
        return table[(q * 255).long()]                                    # [H,W,3] u8

    def colour(v):
        return torch.floor(v.double().clamp(0, 1) * 255 + 0.5).to(torch.uint8).permute(1, 2, 0)
    e = (render.permute(1, 2, 0) @ A + b).permute(2, 0, 1)
    y, x = torch.meshgrid(torch.arange(H, device=gt.device).float(), torch.arange(W, device=gt.device).float(), indexing="ij")
    pts = torch.stack([(x - cx) / fx, (y - cy) / fy, torch.ones_like(x)], 0) * depth
    dx = pts[:, 1:-1, 2:] - pts[:, 1:-1, :-2]
    dy = pts[:, 2:, 1:-1] - pts[:, :-2, 1:-1]
    n = torch.nn.functional.pad(torch.nn.functional.normalize(torch.cross(dx, dy, dim=0), dim=0), (1, 1, 1, 1))
    row0 = torch.cat([colour(gt), colour(render), colour((gt - e).abs() * 10)], 1)
    row1 = torch.cat([turbo(gt_depth), turbo(depth[0]), turbo((gt_depth - depth[0]).abs())], 1)
    row2 = torch.cat([colour((normal + 1) / 2), colour((n + 1) / 2), turbo((alpha[0] > 0.5).float())], 1)
    return torch.cat([row0, row1, row2], 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=[384, 512])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_panel needs a GPU: a time measured anywhere else says nothing")
    H, W = a.size
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.rand(*s, generator=g).to(DEV)
    gt, render, normal = r(3, H, W), r(3, H, W), 2 * r(3, H, W) - 1
    gt_depth, depth, alpha = 0.5 + 4 * r(H, W), 0.5 + 4 * r(1, H, W), r(1, H, W)
    A, b = (torch.eye(3) + 0.1 * torch.rand(3, 3, generator=g)).to(DEV), (0.05 * torch.rand(3, generator=g)).to(DEV)
    K = (0.9 * W, 0.9 * W, 0.5 * W, 0.5 * H)
    table = torch.from_numpy(ops.turbo_u8()).to(DEV)
    hip = lambda: ops.gs_panel(gt, render, A, b, gt_depth, depth, normal, alpha, *K)
    ref = lambda: torch_panel(gt, render, A, b, gt_depth, depth, normal, alpha, *K, table)
    differ = int((hip() != ref()).sum())
    k_best, k_med = timed(hip, a.reps)
    t_best, t_med = timed(ref, a.reps)
    nbytes = H * W * (4 * (12 + 3) + 27)
    out = {"H": H, "W": W, "reps": a.reps, "hip_ms_best": k_best, "hip_ms_median": k_med, "torch_ms_best": t_best, "torch_ms_median": t_med,
           "speedup_median": t_med / k_med, "bytes": nbytes, "floor_ms": nbytes / (HBM_TBS * 1e12) * 1e3, "bytes_differing_from_torch": differ,
           "panel_bytes": 27 * H * W}
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
