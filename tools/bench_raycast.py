#!/usr/bin/env python3
"""Ray cast of the TSDF volumes (csrc/tsdf_raycast.hip) on the synthetic six-walled room of tools/bench_tsdf.py: the views are fused into
the dense grid and into the sparse brick volume, then 16 of them (a launch) are cast at 480 x 640.

Per store: ms per launch of 16 views (depth only, and with normals and colours), rays/s, the share of rays that hit, and the mean number
of samples a ray looks up in the store (the `samples` output: after the clipping to the grid and, in the brick pool, the skipping inside
unallocated bricks) against the samples of the plain march (t_max / step).  For the same views the route that existed before: the
marching-tetrahedra mesh (extract_mesh) and its rasterisation (mesh_render.render_depth), and how far the two depth images differ.
Host clock around work that ends in a device synchronise, after a warm-up of every shape; best of --reps.
usage: python tools/bench_raycast.py [--voxel 0.02] [--views 64] [--size 480 640] [--reps 3] [--json out.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cut3r_slam_amd import mesh_render
from cut3r_slam_amd.tsdf import SparseTSDFVolume, TSDFVolume
from tools.bench_tsdf import DEV, ROOM, look_dirs, render_room, timed


def bench_store(vol, w2c, K, H, W, reps):
    B = w2c.shape[0]
    full = lambda: vol.ray_cast(w2c, K, H, W)
    bare = lambda: vol.ray_cast(w2c, K, H, W, normals=False, colors=False)
    full(), bare()                                                       # warm-up
    t_full, t_bare = timed(full, reps), timed(bare, reps)
    rc, samples = vol.ray_cast(w2c, K, H, W, count=True)
    plain = int(np.floor(vol.depth_max / (0.5 * vol.voxel_size))) + 1
    return rc, {"launch_ms_depth_normal_color": round(1e3 * t_full, 3), "launch_ms_depth_only": round(1e3 * t_bare, 3),
                "rays_per_s": float(f"{B * H * W / t_full:.4g}"), "hit_share": round(float((rc.depth > 0).float().mean()), 4),
                "mean_samples_per_ray": round(float(samples.double().mean()), 1), "max_samples_per_ray": int(samples.max()),
                "plain_march_samples_per_ray": plain, "samples_per_s": float(f"{float(samples.double().sum()) / t_bare:.4g}")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--views", type=int, default=64, help="views fused into the volumes; the first 16 are cast")
    ap.add_argument("--size", type=int, nargs=2, default=[480, 640])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_raycast needs the GPU")
    H, W = args.size
    f = W / 2.0
    w2c_np, _ = look_dirs(args.views, np.random.default_rng(0))
    depth, rgb = render_room(w2c_np, H, W, f)
    w2c = torch.from_numpy(w2c_np).to(DEV)
    K = torch.tensor([[f, f, (W - 1) / 2, (H - 1) / 2]], dtype=torch.float32, device=DEV).expand(args.views, 4).contiguous()
    pad = 8 * args.voxel
    dense = TSDFVolume.from_bounds((0, 0, 0), ROOM, args.voxel, pad=pad, device=DEV).integrate(depth, w2c, K, rgb=rgb)
    sparse = SparseTSDFVolume(dense.origin, dense.voxel_size, dense.dims, device=DEV).integrate(depth, w2c, K, rgb=rgb)
    cast_w2c, cast_K = w2c_np[:16], K[:16]
    res = {"scene": f"six-walled room {ROOM[0]} x {ROOM[1]} x {ROOM[2]} m, {args.views} views fused, 16 cast at {W}x{H}, f = {f:g}, "
                    f"voxel {args.voxel:g}, grid {dense.dims}, step 0.5 voxel, depth_max {dense.depth_max:g}",
           "device": torch.cuda.get_device_name(0), "bricks": [sparse.n_bricks, sparse.table.numel()]}
    rd, res["dense"] = bench_store(dense, cast_w2c, cast_K, H, W, args.reps)
    rs, res["sparse"] = bench_store(sparse, cast_w2c, cast_K, H, W, args.reps)
    both = (rd.depth > 0) & (rs.depth > 0)
    res["sparse_vs_dense"] = {"dense_hits_sparse_misses": int(((rd.depth > 0) & ~(rs.depth > 0)).sum()),
                              "sparse_hits_dense_misses": int((~(rd.depth > 0) & (rs.depth > 0)).sum()),
                              "same_bits_where_both_hit": bool(torch.equal(rd.depth[both], rs.depth[both]))}
    # the route that existed before: the mesh, then its rasterisation at the same views
    c2w = np.linalg.inv(np.concatenate([cast_w2c.reshape(16, 3, 4).astype(np.float64), np.tile([[[0.0, 0.0, 0.0, 1.0]]], (16, 1, 1))], 1))
    mesh = dense.extract_mesh(1.0)
    raster = lambda: mesh_render.render_depth(mesh, c2w, cast_K.cpu().numpy(), H, W)
    md = raster()
    t_ext, t_ras = timed(lambda: dense.extract_mesh(1.0), args.reps), timed(raster, args.reps)
    m = (md > 0) & (rd.depth > 0)
    diff = (md - rd.depth)[m].abs() / dense.voxel_size
    res["mesh_route"] = {"faces": int(len(mesh.faces)), "extract_mesh_ms_incl_host_copy": round(1e3 * t_ext, 2),
                         "raster_16_views_ms_incl_upload": round(1e3 * t_ras, 2), "total_ms": round(1e3 * (t_ext + t_ras), 2),
                         "masks_differ_share": round(float(((md > 0) != (rd.depth > 0)).float().mean()), 5),
                         "median_abs_diff_voxels": round(float(diff.median()), 4), "share_over_half_voxel": round(float((diff > 0.5).float().mean()), 4)}
    print(json.dumps(res), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
