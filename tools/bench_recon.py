#!/usr/bin/env python3
"""Reconstruction metrics (csrc/recon.hip) on the room of tools/bench_tsdf.py: the room fused at each voxel size (default 0.02 m and
0.006 m) is the rec mesh, its six walls tessellated at ~2 cm the GT mesh.

Times (host clock around work that ends in a device synchronise, after a warm-up; best of --reps): face areas + fp64 scan + 200 k
samples; the grid over 200 k points and a query of 200 k points; full calc_3d_metric with and without alignment; one ICP iteration
(query + moments) at full vertex counts.  CPU baseline: scipy cKDTree(...).query(workers=16) on the same arrays (build and query).
Kernel-level split: run under `rocprofv3 --kernel-trace --stats`.
usage: python tools/bench_recon.py [--voxel 0.02 0.006] [--views 300] [--reps 3] [--json out.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cut3r_slam_amd import eval_recon as ER
from cut3r_slam_amd import ops
from cut3r_slam_amd.tsdf import Mesh, TSDFVolume
from tests import recon_oracle as O
from tools import bench_tsdf as BT

DEV = "cuda:0"


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return best * 1e3


def cpu_timed(fn, reps):
    best = float("inf")
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t)
    return best * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel", type=float, nargs="+", default=[0.02, 0.006])
    ap.add_argument("--views", type=int, default=300)
    ap.add_argument("--size", type=int, nargs=2, default=[384, 512])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from scipy.spatial import cKDTree
    H, W = a.size
    f = 0.5 * W
    w2c, _ = BT.look_dirs(a.views, np.random.default_rng(0))
    depth, rgb = BT.render_room(w2c, H, W, f)
    K = torch.tensor([f, f, (W - 1) / 2, (H - 1) / 2], device=DEV)
    gv, gf = O.box_room(BT.ROOM, 0.02)
    gt = Mesh(gv, np.zeros_like(gv, dtype=np.uint8), gf)
    out = {"gt_vertices": len(gv), "gt_faces": len(gf), "voxels": []}
    print(f"GT room {BT.ROOM}: {len(gv)} vertices, {len(gf)} faces")
    for voxel in a.voxel:
        vol = TSDFVolume.from_bounds((0, 0, 0), BT.ROOM, voxel, device=DEV)
        vol.integrate(depth, torch.from_numpy(w2c).to(DEV), K, rgb=rgb)
        rec = vol.extract_mesh(1.0)
        del vol
        torch.cuda.empty_cache()
        r = {"voxel": voxel, "rec_vertices": len(rec.vertices), "rec_faces": len(rec.faces)}
        v = torch.from_numpy(rec.vertices).to(DEV)
        fc = torch.from_numpy(rec.faces).to(DEV)
        n = ER.N_SAMPLES
        _, cdf = ops.mesh_area_cdf(v, fc)
        r["area_scan_ms"] = timed(lambda: ops.mesh_area_cdf(v, fc), a.reps)
        r["sample_200k_ms"] = timed(lambda: ops.mesh_sample(v, fc, cdf, n, 0, 1), a.reps)
        rec_pc = ops.mesh_sample(v, fc, cdf, n, 0, 1)
        gt_pc = ER.sample_surface(gt, n, stream=2)
        grid = ops.NNGrid(gt_pc, n)
        r["grid_build_200k_ms"] = timed(lambda: ops.NNGrid(gt_pc, n), a.reps)
        r["query_200k_ms"] = timed(lambda: grid.query(rec_pc), a.reps)
        # cKDTree on the same arrays, 16 workers
        gh, rh = gt_pc.cpu().numpy().astype(np.float64), rec_pc.cpu().numpy().astype(np.float64)
        r["ckdtree_build_200k_ms"] = cpu_timed(lambda: cKDTree(gh), a.reps)
        tree = cKDTree(gh)
        r["ckdtree_query_200k_ms"] = cpu_timed(lambda: tree.query(rh, workers=16), a.reps)
        r["calc_3d_metric_noalign_ms"] = timed(lambda: ER.calc_3d_metric(rec, gt, align=False), 1)
        t = time.perf_counter()
        res = ER.get_align_transformation(rec, gt)
        torch.cuda.synchronize()
        r["icp_ms"], r["icp_iterations"], r["icp_fitness"] = (time.perf_counter() - t) * 1e3, res.iterations, res.fitness
        r["calc_3d_metric_align_ms"] = timed(lambda: ER.calc_3d_metric(rec, gt, align=True), 1)
        r["metric"] = ER.calc_3d_metric(rec, gt, align=True)
        # one ICP iteration at full vertex counts: correspondences + moments (the grid over the GT vertices built once)
        src, dst = v.contiguous(), torch.from_numpy(gv).to(DEV)
        g2 = ops.NNGrid(dst, src.shape[0])
        M = np.eye(4)

        def icp_iter():
            d2, idx = g2.query(src, max_dist=0.1, transform=M)
            g2.moments(src, d2, idx, transform=M).cpu()
        r["icp_iteration_full_ms"] = timed(icp_iter, a.reps)
        r["nn_full_vertices_ms"] = timed(lambda: g2.query(src), a.reps)
        print(json.dumps(r))
        out["voxels"].append(r)
        del rec_pc, gt_pc, grid, g2
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
