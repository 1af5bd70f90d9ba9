#!/usr/bin/env python3
"""Trajectory filler micro-benchmark: milliseconds per `GSMapper.pose_estimator` iteration and per filled frame (one call of `--iters`
iterations, the reference runs 100) on the synthetic wall of tools/bench_gs.py's mapper leg (cut3r_slam_amd/synth.gs_wall_window, 512x384),
once with the three-call backward (pose_backward="chain": cut3r_gs_preprocess_backward + cut3r_gs_activate_backward) and once with
cut3r_gs_pose_backward ("fused"), in the same process on the same map.

Method: the map is built once; `--warmup` untimed calls per path (code objects, allocator, buffers), then `--repeats` timed calls per path,
the two paths alternating so that clock drift hits both alike; wall time around a synchronised call (a call ends with a host read of the
pose, as the filler uses it).  Reported: median, min and max over the repeats, and the bytes each backward moves per iteration as
counted from P.
usage: python tools/bench_fill.py [--iters 100] [--repeats 7] [--warmup 2] [--size 384 512]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from cut3r_slam_amd import gs_mapper as GM, synth

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--size", type=int, nargs=2, default=[384, 512])
args = ap.parse_args()
if args.repeats < 5:
    ap.error("--repeats must be at least 5")
DEV = "cuda:0"
H, W = args.size
packet, imgs, cfg = synth.gs_wall_window(H, W, device=DEV)
m = GM.GSMapper(cfg, 440.0, 440.0, W / 2, H / 2, downsample_ratio=2, device=DEV)
m.run(packet, iterations=5, init_iters=20, gba_per_view=1)
P = len(m.gaussians)
# a frame between keyframes 2 and 3: keyframe 3's image, started from keyframe 2's pose (5 cm and 0.6 degrees away)
start, frame = packet["poses"][2], imgs[3]
times = {"chain": [], "fused": []}
moved = {}
for r in range(args.warmup + args.repeats):
    for mode in ("chain", "fused"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pose = m.pose_estimator(start, frame, 3, iters=args.iters, pose_backward=mode)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if r >= args.warmup:
            times[mode].append(1e3 * dt)
        moved[mode] = float((pose - start).abs().max())
# floats per Gaussian and iteration after cut3r_gs_render_backward (4 bytes each).  Both: the activated Gaussian (means 3, scales 3,
# rotations 4, opacity 1), its geom and dgeom records (32 + 32), theta (14).  Chain only: the fill of the gradient block (17), its
# writes (d_means 3, d_scales 3, d_rots 4, d_opac 1, d_shs 3, d_means2D 3 = 17), the colour coefficients read (3) and d_means + d_rots read
# back (7).  Fused only: 16 floats per 256 Gaussians of partial rows, written and read once.
common = (11 + 64 + 14) * 4 * P
bytes_it = {"chain": common + (17 + 17 + 3 + 7) * 4 * P, "fused": common + 2 * 16 * 4 * ((P + 255) // 256)}
out = {"scene": f"synthetic wall {W}x{H}, {P} Gaussians, {len(m.viewpoints)} keyframes", "iters_per_frame": args.iters, "repeats": args.repeats,
       "warmup": args.warmup, "redone_for_capacity": m._fused_trainer().redone}
for mode in ("chain", "fused"):
    t = sorted(times[mode])
    out[mode] = {"ms_per_frame_median": statistics.median(t), "ms_per_frame_min": t[0], "ms_per_frame_max": t[-1],
                 "ms_per_iteration_median": statistics.median(t) / args.iters, "backward_bytes_per_iteration": bytes_it[mode],
                 "pose_moved": moved[mode]}
    print(f"pose_backward={mode:5s}: {statistics.median(t):8.2f} ms per filled frame (min {t[0]:.2f}, max {t[-1]:.2f}, {args.repeats} repeats) = "
          f"{statistics.median(t) / args.iters:.3f} ms per iteration; backward moves {bytes_it[mode] / 1e6:.2f} MB per iteration")
print(json.dumps(out))
