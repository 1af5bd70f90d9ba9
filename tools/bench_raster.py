#!/usr/bin/env python3
"""Mesh depth rasteriser (csrc/raster.hip) and the 2-D depth-L1 metric on the room of tools/bench_tsdf.py: the room fused at each voxel
size (default 0.02 m and 0.006 m) is the rec mesh, its six walls tessellated at ~2 cm the GT mesh.  Cameras: the metric's own
(eval_recon.sample_views in the box of get_cam_position), 500 x 500 pixels at focal 300 as the reference renders.

Times (host clock around work that ends in a device synchronise, after a warm-up; best of --reps): mesh_raster of the rec mesh at B = 1
(mean over 4 views) and B = 16, per view, and the triangle-views per second they amount to; the share of the pixels with a hit; depth_l1
of 16 views; calc_2d_metric end to end (uploads, both meshes rendered, no alignment, cameras given / sampled) at 10 and 1000 views.
Kernel-level split: run under `rocprofv3 --kernel-trace --stats`.
usage: python tools/bench_raster.py [--voxel 0.02 0.006] [--views 300] [--reps 3] [--n-imgs 10 1000] [--json out.json]"""
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
from tools.bench_recon import timed

DEV = "cuda:0"
H = W = 500
FOCAL = 300.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel", type=float, nargs="+", default=[0.02, 0.006])
    ap.add_argument("--views", type=int, default=300, help="views fused into the room")
    ap.add_argument("--size", type=int, nargs=2, default=[384, 512])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n-imgs", type=int, nargs="+", default=[10, 1000])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    fh, fw = a.size
    f = 0.5 * fw
    w2c_fuse, _ = BT.look_dirs(a.views, np.random.default_rng(0))
    depth, rgb = BT.render_room(w2c_fuse, fh, fw, f)
    Kf = torch.tensor([f, f, (fw - 1) / 2, (fh - 1) / 2], device=DEV)
    gv, gf = O.box_room(BT.ROOM, 0.02)
    gt = Mesh(gv, np.zeros_like(gv, dtype=np.uint8), gf)
    K = [FOCAL, FOCAL, W / 2.0 - 0.5, H / 2.0 - 0.5]
    extents, transform = ER.get_cam_position(gt)
    cams = ER.sample_views(extents, transform, max(a.n_imgs + [16]), seed=0)
    w2c = np.linalg.inv(cams)[:, :3]
    out = {"gt_vertices": len(gv), "gt_faces": len(gf), "image": [H, W], "focal": FOCAL, "voxels": []}
    print(f"GT room {BT.ROOM}: {len(gv)} vertices, {len(gf)} faces; {len(cams)} cameras of sample_views")
    gvd, gfd = ER._gpu_mesh(gt)
    out["gt_raster_b16_ms_per_view"] = timed(lambda: ops.mesh_raster(gvd, gfd, w2c[:16], K, H, W), a.reps) / 16
    print(f"GT mesh: B = 16 {out['gt_raster_b16_ms_per_view']:.3f} ms per view", flush=True)
    for voxel in a.voxel:
        vol = TSDFVolume.from_bounds((0, 0, 0), BT.ROOM, voxel, device=DEV)
        vol.integrate(depth, torch.from_numpy(w2c_fuse).to(DEV), Kf, rgb=rgb)
        rec = vol.extract_mesh(1.0)
        del vol
        torch.cuda.empty_cache()
        F = len(rec.faces)
        r = {"voxel": voxel, "rec_vertices": len(rec.vertices), "rec_faces": F}
        v, fc = ER._gpu_mesh(rec)
        b1 = np.mean([timed(lambda k=k: ops.mesh_raster(v, fc, w2c[k:k + 1], K, H, W), a.reps) for k in range(4)])
        b16 = timed(lambda: ops.mesh_raster(v, fc, w2c[:16], K, H, W), a.reps)
        r["raster_b1_ms_per_view"], r["raster_b16_ms_per_view"] = float(b1), b16 / 16
        print(f"voxel {voxel}: {F} faces, B = 1 {b1:.3f} ms, B = 16 {b16 / 16:.3f} ms per view", flush=True)
        r["raster_b16_face_id_ms_per_view"] = timed(lambda: ops.mesh_raster(v, fc, w2c[:16], K, H, W, face_id=True), a.reps) / 16
        r["triangle_views_per_s_b1"], r["triangle_views_per_s_b16"] = F / (b1 * 1e-3), 16 * F / (b16 * 1e-3)
        d = ops.mesh_raster(v, fc, w2c[:16], K, H, W)
        g = ops.mesh_raster(gvd, gfd, w2c[:16], K, H, W)
        r["pixels_hit_share"] = float((d > 0).double().mean())
        r["depth_l1_16_views_ms"] = timed(lambda: ops.depth_l1(g, d), a.reps)
        for n in a.n_imgs:
            t = time.perf_counter()
            res = ER.calc_2d_metric(rec, gt, align=False, views=cams[:n])
            torch.cuda.synchronize()
            r[f"calc_2d_metric_{n}_views_ms"] = (time.perf_counter() - t) * 1e3
            r[f"depth_l1_cm_{n}_views"] = res["depth l1"]
            print(f"voxel {voxel}: calc_2d_metric {n} views {r[f'calc_2d_metric_{n}_views_ms']:.1f} ms", flush=True)
        t = time.perf_counter()
        ER.calc_2d_metric(rec, gt, align=False, n_imgs=a.n_imgs[0])
        torch.cuda.synchronize()
        r[f"calc_2d_metric_{a.n_imgs[0]}_sampled_views_ms"] = (time.perf_counter() - t) * 1e3
        print(json.dumps(r), flush=True)
        out["voxels"].append(r)
        del v, fc, d, g
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as fh_:
            json.dump(out, fh_, indent=1)


if __name__ == "__main__":
    main()
