#!/usr/bin/env python3
"""Dense point-cloud evaluation (csrc/cloud.hip, cut3r_slam_amd/eval_dense.py) at the size of a 7-Scenes sequence: --gt-views (1000) GT
depth maps of 392 x 518 and --kf-views (150) keyframe depth maps of the room of tools/bench_tsdf.py, rendered from its ~2 cm wall mesh
by mesh_render.render_depth.

Times (device events around synchronised work, after a warm-up; best of --reps): the back-projection of the GT views at B = 1 and
B = 16 views per launch, the voxel downsample of the GT cloud at 0.05 m, one ICP iteration (query + moments) on the downsampled clouds,
the two Chamfer queries between the run's cloud and the cloud of the matched GT frames (one run each, no warm-up; the grid build is
part of the query), dense_metrics end to end (host clock: it reads results back).  With each kernel time the bytes the kernel must move
(inputs read once, outputs written once) and the rate that gives.  In the same process, alternating with the kernels (torch, kernel,
torch, kernel, ... after one warm-up run of each; best of --reps each), the torch statement of the same back-projection (fp64
meshgrid, mask, matmul, cast, cat) on the first 64 views and eval_recon.voxel_down_sample on the first 20 M points.
usage: python tools/bench_cloud.py [--gt-views 1000] [--kf-views 150] [--reps 3] [--json out.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cut3r_slam_amd import eval_dense as ED
from cut3r_slam_amd import eval_recon as ER
from cut3r_slam_amd import mesh_render as MR
from cut3r_slam_amd import ops
from cut3r_slam_amd.tsdf import Mesh
from tests import recon_oracle as O
from tools import bench_tsdf as BT

DEV = "cuda:0"
TRUNC = 4.5


def timed(fn, reps, warm=True):
    """best of reps, ms, by device events around fn (the stream is idle before and after)"""
    if warm:
        fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def timed_pair(fa, fb, reps):
    """best of reps of each, ms, the two alternating (a, b, a, b, ...) after one warm-up run of each"""
    fa()
    fb()
    best = [float("inf"), float("inf")]
    for _ in range(reps):
        for k, fn in enumerate((fa, fb)):
            best[k] = min(best[k], timed(fn, 1, warm=False))
    return best


def torch_backproject(depth, c2w, K, trunc):
    """the torch statement of ops.depth_cloud: per view fp64 pixel grid, mask, affine, fp32, then one cat"""
    B, H, W = depth.shape
    dev = depth.device
    T = torch.as_tensor(c2w, dtype=torch.float64, device=dev).reshape(B, 3, 4)
    K = torch.as_tensor(K, dtype=torch.float64, device=dev).reshape(-1, 4).expand(B, 4)
    v, u = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    out = []
    for b in range(B):
        d = depth[b]
        ok = torch.isfinite(d) & (d > 0) & (d < trunc)
        z = d[ok].double()
        pc = torch.stack([(u[ok] - K[b, 2]) * z / K[b, 0], (v[ok] - K[b, 3]) * z / K[b, 1], z], 1)
        out.append((pc @ T[b, :, :3].T + T[b, :, 3]).float())
    return torch.cat(out)


def emit_batched(depth, c2w, K, per_launch):
    """ops.depth_cloud restricted to `per_launch` views a launch (B = 1: one view a launch)"""
    return [ops.depth_cloud(depth[b:b + per_launch], c2w[b:b + per_launch], K, TRUNC)[0] for b in range(0, depth.shape[0], per_launch)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gt-views", type=int, default=1000)
    ap.add_argument("--kf-views", type=int, default=150)
    ap.add_argument("--size", type=int, nargs=2, default=[392, 518])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    H, W = a.size
    f = 0.5 * W
    K = np.array([f, f, (W - 1) / 2, (H - 1) / 2])
    gv, gf = O.box_room(BT.ROOM, 0.02)
    room = Mesh(gv, np.zeros_like(gv, dtype=np.uint8), gf)
    w2c, _ = BT.look_dirs(a.gt_views, np.random.default_rng(0))
    w = np.tile(np.eye(4), (a.gt_views, 1, 1))
    w[:, :3] = w2c.astype(np.float64).reshape(-1, 3, 4)
    c2w = np.linalg.inv(w)
    depth = MR.render_depth(room, c2w, K, H, W)
    kf = np.linspace(0, a.gt_views - 1, a.kf_views).round().astype(int)
    # the run: the keyframes' own depths with 1 % multiplicative noise, the trajectory under a similarity
    g = torch.Generator(device=DEV).manual_seed(0)
    kf_depth = (depth[torch.from_numpy(kf).to(DEV)] * (1 + 0.01 * torch.randn(len(kf), H, W, device=DEV, generator=g))).contiguous() / 1.3
    S = np.eye(4)
    S[:3, :3] = O.rot([0.1, 0.2, 0.9], 0.4) / 1.3
    S[:3, 3] = [1.0, -2.0, 0.5]
    kf_c2w = S @ c2w[kf]
    kf_c2w[:, :3, :3] *= 1.3                                          # poses stay rigid: only the positions and the depths carry the scale
    torch.cuda.synchronize()
    r = {"gt_views": a.gt_views, "kf_views": a.kf_views, "H": H, "W": W}

    def stage(name):
        print(f"[bench_cloud] {name}: " + json.dumps({k: v for k, v in r.items() if k != "result"}), file=sys.stderr, flush=True)
    c2w12 = c2w[:, :3].reshape(-1, 12)
    pts, _, counts = ops.depth_cloud(depth, c2w12, K, TRUNC)
    N = pts.shape[0]
    r["gt_points"] = N
    # bytes a back-projection must move: every depth read twice (count, emit), 12 B written per point
    bp_bytes = 2 * 4 * depth.numel() + 12 * N
    del pts
    for per in (16, 1):
        ms = timed(lambda: emit_batched(depth, c2w12, K, per), a.reps)
        r[f"backproject_B{per}_ms"], r[f"backproject_B{per}_GBs"] = ms, bp_bytes / ms / 1e6
    ms = timed(lambda: ops.depth_cloud(depth, c2w12, K, TRUNC), a.reps)
    r["backproject_all_ms"], r["backproject_all_GBs"], r["backproject_bytes"] = ms, bp_bytes / ms / 1e6, bp_bytes
    n_t = min(a.gt_views, 64)                                             # the torch path at full size needs several full-size temporaries
    t_ms, k_ms = timed_pair(lambda: torch_backproject(depth[:n_t], c2w12[:n_t], K, TRUNC),
                            lambda: ops.depth_cloud(depth[:n_t], c2w12[:n_t], K, TRUNC), a.reps)
    r["torch_backproject_views"], r["torch_backproject_ms"], r["kernel_backproject_same_views_ms"] = n_t, t_ms, k_ms
    stage("back-projection")
    pts, _, _ = ops.depth_cloud(depth, c2w12, K, TRUNC)
    # downsample: the points read for the bounds, the keys and the means (12 B each), key + index pairs written, sorted in 8 radix passes
    # of 12 B read + 12 B written, read again for the heads; outputs are small
    ds_bytes = N * (3 * 12 + 12 + 8 * 24 + 2 * 8 + 4)
    ms = timed(lambda: ops.voxel_downsample(pts, 0.05), a.reps)
    gt_down = ops.voxel_downsample(pts, 0.05)[0]
    r["downsample_ms"], r["downsample_GBs"], r["downsample_bytes"], r["gt_voxels"] = ms, ds_bytes / ms / 1e6, ds_bytes, gt_down.shape[0]
    n_t = min(N, 20_000_000)                                              # torch.unique(dim=0) over [N,3] int64 keys: kept to 20 M points
    sub = pts[:n_t].contiguous()
    r["torch_downsample_points"] = n_t
    r["torch_downsample_ms"], r["kernel_downsample_same_points_ms"] = timed_pair(lambda: ER.voxel_down_sample(sub, 0.05),
                                                                                 lambda: ops.voxel_downsample(sub, 0.05), a.reps)
    del sub
    stage("downsample")
    # the run's cloud under the true alignment (what dense_metrics arrives at): S^-1 . pose, an affine with the scale 1.3
    est_pts, _, _ = ops.depth_cloud(kf_depth, (np.linalg.inv(S) @ kf_c2w)[:, :3].reshape(-1, 12), K, TRUNC)
    est_down = ops.voxel_downsample(est_pts, 0.05)[0]
    r["est_points"], r["est_voxels"] = est_pts.shape[0], est_down.shape[0]
    grid = ops.NNGrid(gt_down, est_down.shape[0])
    I4 = np.eye(4)

    def icp_iter():
        d2, idx = grid.query(est_down, max_dist=0.1, transform=I4)
        grid.moments(est_down, d2, idx, transform=I4)
    r["icp_iteration_ms"] = timed(icp_iter, a.reps)
    del grid
    stage("icp iteration")
    # the Chamfer queries at the size dense_metrics runs them: the GT cloud is the GT frames matched to a keyframe, not all of them
    del pts
    gt_m, _, _ = ops.depth_cloud(depth[torch.from_numpy(kf).to(DEV)].contiguous(), c2w12[kf], K, TRUNC)
    r["matched_gt_points"] = gt_m.shape[0]
    r["chamfer_est_to_gt_ms"] = timed(lambda: ops.nn_query(gt_m, est_pts, max_dist=0.5), 1, warm=False)
    r["chamfer_gt_to_est_ms"] = timed(lambda: ops.nn_query(est_pts, gt_m, max_dist=0.5), 1, warm=False)
    stage("chamfer queries")
    del gt_m, est_pts
    torch.cuda.empty_cache()
    stamps = np.arange(a.gt_views, dtype=np.float64)
    gt = ED.DepthViews(depth, c2w, K, stamps)
    est = ED.DepthViews(kf_depth, kf_c2w, K, stamps[kf])
    t = time.perf_counter()
    res = ED.dense_metrics(est, gt)
    torch.cuda.synchronize()
    r["dense_metrics_s"] = time.perf_counter() - t
    r["result"] = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in res.items()}
    print(json.dumps(r))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(r, fh, indent=1)


if __name__ == "__main__":
    main()
