#!/usr/bin/env python3
"""Mesh clean-up (csrc/mesh_clean.hip) on the bench room of tools/bench_tsdf.py: the six-walled room fused from 300 views at 0.006 m (the
17.7 M-vertex mesh of DESIGN.md section 4c), then vertex clustering at cells 0.012 and 0.02 and min_faces=100 on the raw mesh, all on
device tensors (no host copy of the mesh).

Per configuration: the stages from HIP events on the stream (face check; keys + sort; remap; de-duplication; means; compaction;
labelling and its round count; filter), the end-to-end host clock of the call (allocations and the read-backs of the totals included),
and the output sizes; for context the extract_mesh time of the same run.  One warm-up call, then --reps calls; medians.
usage: python tools/bench_mesh_clean.py [--voxel 0.006] [--cells 0.012 0.02] [--min-faces 100] [--views 300] [--reps 5] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np
import torch

import bench_tsdf as BT
from cut3r_slam_amd import ops
from cut3r_slam_amd.tsdf import TSDFVolume

DEV = BT.DEV


def measure(fn, reps):
    """fn(timing) -> result; ({stage: median ms}, median host ms of the whole call, the last result)"""
    fn({})                                                   # warm-up: the allocator's blocks and hipcub's kernels
    stages, wall, out = {}, [], None
    for _ in range(reps):
        timing = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(timing)
        torch.cuda.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
        for k, v in timing.items():
            stages.setdefault(k, []).append(v)
    return {k: round(statistics.median(v), 3) for k, v in stages.items()}, round(statistics.median(wall), 3), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel", type=float, default=0.006)
    ap.add_argument("--cells", type=float, nargs="+", default=[0.012, 0.02])
    ap.add_argument("--min-faces", type=int, default=100)
    ap.add_argument("--views", type=int, default=300)
    ap.add_argument("--size", type=int, nargs=2, default=[384, 512])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_clean needs the GPU")
    H, W = args.size
    f = W / 2.0
    w2c_np, _ = BT.look_dirs(args.views, np.random.default_rng(0))
    depth, rgb = BT.render_room(w2c_np, H, W, f)
    w2c = torch.from_numpy(w2c_np).to(DEV)
    K = torch.tensor([[f, f, (W - 1) / 2, (H - 1) / 2]], dtype=torch.float32, device=DEV).expand(args.views, 4).contiguous()
    vol = TSDFVolume.from_bounds((0, 0, 0), BT.ROOM, args.voxel, pad=8 * args.voxel, max_voxels=2 ** 31 - 1, device=DEV)
    vol.integrate(depth, w2c, K, rgb=rgb)
    vol._extract(1.0)                                        # warm-up
    t_ext = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        verts, cols, faces = vol._extract(1.0)
        torch.cuda.synchronize()
        t_ext.append(1e3 * (time.perf_counter() - t0))
    del vol, depth, rgb
    torch.cuda.empty_cache()
    V, F = verts.shape[0], faces.shape[0]
    res = {"scene": f"six-walled room {BT.ROOM[0]} x {BT.ROOM[1]} x {BT.ROOM[2]} m, {args.views} views at {W}x{H}, voxel {args.voxel:g}",
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "vertices": V, "faces": F,
           "extract_mesh_device_ms": round(statistics.median(t_ext), 3), "results": []}
    print(json.dumps({k: v for k, v in res.items() if k != "results"}), flush=True)
    for cell in args.cells:
        stages, wall, r = measure(lambda t: ops.mesh_cluster(verts, cols, faces, cell, timing=t), args.reps)
        row = {"op": "simplify_vertex_clustering", "cell": cell, "stages_ms": stages, "stages_sum_ms": round(sum(stages.values()), 3),
               "call_ms_host_clock": wall, "vertices_out": r["vertices"].shape[0], "faces_out": r["faces"].shape[0],
               **{k: r[k] for k in ("clusters", "degenerate", "duplicate", "unreferenced")}}
        res["results"].append(row)
        print(json.dumps(row), flush=True)
        del r
    stages, wall, r = measure(lambda t: ops.mesh_components(verts, cols, faces, min_faces=args.min_faces, timing=t), args.reps)
    rounds = stages.pop("rounds")
    row = {"op": "remove_small_components", "min_faces": args.min_faces, "stages_ms": stages, "rounds": int(rounds),
           "stages_sum_ms": round(sum(stages.values()), 3), "call_ms_host_clock": wall, "vertices_out": r["vertices"].shape[0],
           "faces_out": r["faces"].shape[0], "components": r["n_components"], "components_kept": r["components"].shape[0]}
    res["results"].append(row)
    print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
