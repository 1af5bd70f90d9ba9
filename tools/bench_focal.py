#!/usr/bin/env python3
"""Focal-length estimators micro-benchmark (cut3r_slam_amd/self_calib.py, csrc/calib.hip): milliseconds per call of ops.focal_weiszfeld
(10 iterations) and ops.focal_median at 5 x 384 x 512 (one tracking window plus nothing: what a run without a calibration adds, once) and
140 x 384 x 512 (every keyframe of a long run), and beside each the same formula written with torch operators on the same GPU in the same
process.  The torch formulation is stated here (`torch_weiszfeld`, `torch_median`): whole-tensor elementwise operators, `mean` and
`nanmedian` per view.

Method: a seeded noisy pinhole scene; HIP events around each call on the current stream, workspace and output allocation included;
`--warmup` untimed calls, then `--repeats` timed ones, the median.  Launches per call are what the C entry points issue (csrc/calib.hip):
Weiszfeld iters + 2 kernels, median one memset + 5 kernels.
usage: python tools/bench_focal.py [--repeats 7] [--warmup 2] [--json FILE]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from cut3r_slam_amd import ops


def scene(B, H, W, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    f = 0.85 * W
    col = torch.arange(W, dtype=torch.float32)[None, None, :] - W / 2
    row = torch.arange(H, dtype=torch.float32)[None, :, None] - H / 2
    z = 1 + 3 * torch.rand(B, H, W, generator=g)
    pts = torch.stack([col * z / f, row * z / f, z], -1)
    pts = pts + 0.01 * z[..., None] * torch.randn(B, H, W, 3, generator=g)
    return pts.to(dev).contiguous(), torch.tensor([[W / 2, H / 2]] * B).to(dev)


def _uv(pts, pp):
    B, H, W, _ = pts.shape
    col = torch.arange(W, device=pts.device, dtype=torch.float32)[None, None, :] - pp[:, 0, None, None]
    row = torch.arange(H, device=pts.device, dtype=torch.float32)[None, :, None] - pp[:, 1, None, None]
    return col.expand(B, H, W).reshape(B, -1), row.expand(B, H, W).reshape(B, -1)


def torch_weiszfeld(pts, pp, iters=10):
    B = pts.shape[0]
    u, v = _uv(pts, pp)
    x, y, z = pts.reshape(B, -1, 3).unbind(-1)
    xz, yz = (x / z).nan_to_num(posinf=0, neginf=0), (y / z).nan_to_num(posinf=0, neginf=0)
    a, b = xz * u + yz * v, xz * xz + yz * yz
    f = a.mean(1) / b.mean(1)
    for _ in range(iters):
        du, dv = u - f[:, None] * xz, v - f[:, None] * yz
        w = 1.0 / torch.sqrt(du * du + dv * dv).clamp(min=1e-8)
        f = (w * a).mean(1) / (w * b).mean(1)
    return f


def torch_median(pts, pp):
    B = pts.shape[0]
    u, v = _uv(pts, pp)
    x, y, z = pts.reshape(B, -1, 3).unbind(-1)
    return torch.cat([(u * z) / x, (v * z) / y], 1).nanmedian(1).values


def timed(fn, warmup, repeats):
    ts, out = [], None
    for r in range(warmup + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        if r >= warmup:
            ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_focal needs a GPU")
    dev = "cuda:0"
    out = {"repeats": args.repeats, "warmup": args.warmup, "launches": {"weiszfeld": 12, "median": 6}, "sizes": {}}
    for B, H, W in ((5, 384, 512), (140, 384, 512)):
        pts, pp = scene(B, H, W, dev)
        res = {"mbytes_pts": pts.numel() * 4 / 1e6}
        for mode, hip, ref in (("weiszfeld", lambda: ops.focal_weiszfeld(pts, pp, iters=10), lambda: torch_weiszfeld(pts, pp)),
                               ("median", lambda: ops.focal_median(pts, pp), lambda: torch_median(pts, pp))):
            t_hip, f_hip = timed(hip, args.warmup, args.repeats)
            t_ref, f_ref = timed(ref, args.warmup, args.repeats)
            dev_rel = float(((f_hip - f_ref).abs() / f_ref.abs()).max())
            res[mode] = {"hip_ms": t_hip, "torch_ms": t_ref, "ratio": t_ref / t_hip, "max_rel_difference": dev_rel, "focal_view0": float(f_hip[0])}
            print(f"{B}x{H}x{W} {mode:9s}: HIP {t_hip:.3f} ms ({out['launches'][mode]} launches), torch operators {t_ref:.3f} ms: "
                  f"{t_ref / t_hip:.1f}x; largest relative difference of the two results {dev_rel:.2e}")
        out["sizes"][f"{B}x{H}x{W}"] = res
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w", encoding="utf-8") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
