"""Render a saved Gaussian map along a trajectory: the offline stand-in for the reference's viewer (hislam2's GUI is not built).

    python -m cut3r_slam_amd.gs_view MAP.ply --traj TRAJ.txt --calib "fx fy cx cy"|FILE --size H W --out DIR
                                     [--every N] [--layers rgb depth normal] [--depth-range NEAR FAR]

MAP.ply is a standard 3DGS file of SH degree 0..3 (gs_ply.py: the mapper's 3dgs_final.ply, or another trainer's); TRAJ the TUM rows of
traj_kf.txt / traj_full.txt (`t tx ty tz qx qy qz qw`, camera to world; poses through views.py); the calibration holds at the size given.
Frames are lossless PNGs {i:05d}_{layer}.png, i the row of TRAJ, composed on the GPU by cut3r_gs_frame (csrc/gs_panel.hip): rgb, depth in
turbo over the frame's own range (or --depth-range), the rendered normal map as (n + 1) / 2.

render_cloud calls the rasteriser with the WORLD-frame view matrix and the true camera position.  gs_mapper.render() instead moves the
Gaussians into the camera frame and sets campos = 0, which is right only at SH degree 0 (no view dependence); with the world-frame call
files of degree 1..3 render with the view dependence their trainer gave them."""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from . import ops, views
from .gaussian_rasterizer import GaussianRasterizationSettings, GaussianRasterizer

LAYERS = ("rgb", "depth", "normal")
_SOURCE = {"rgb": "render", "depth": "depth", "normal": "normal"}


def camera_matrices(w2c, K, H, W):
    """(viewmatrix, projmatrix, campos) on the host in the rasteriser's transposed convention, for a world->camera [4,4] and K = fx fy cx cy:
    viewmatrix = w2c^T, projmatrix = (P w2c)^T with P the projection gs_mapper.Camera builds (getProjectionMatrix2, znear 0.01, zfar 100),
    campos = -R^T t; formed in fp64, rounded once"""
    from .gs_mapper import Camera
    M = np.asarray(w2c.detach().cpu() if isinstance(w2c, torch.Tensor) else w2c, np.float64).reshape(4, 4)
    fx, fy, cx, cy = (float(v) for v in np.asarray(K.detach().cpu() if isinstance(K, torch.Tensor) else K, np.float64).reshape(-1)[:4])
    znear, zfar = 0.01, 100.0
    hp = 1.0 if Camera.half_pixel_center else 0.0
    P = np.zeros((4, 4))
    P[0, 0], P[1, 1] = 2 * fx / W, 2 * fy / H
    P[0, 2], P[1, 2] = (2 * cx + hp) / W - 1, (2 * cy + hp) / H - 1
    P[3, 2], P[2, 2], P[2, 3] = 1.0, zfar / (zfar - znear), -(zfar * znear) / (zfar - znear)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    return f32(M.T), f32((P @ M).T), f32(-(M[:3, :3].T @ M[:3, 3]))


@torch.no_grad()
def render_cloud(cloud, w2c, K, H, W, bg=(0, 0, 0)):
    """rasterise a gs_ply.GaussianCloud (any SH degree) from the camera w2c [4,4] (world->camera), K = fx fy cx cy, at H x W -> the dict
    of gs_mapper.render()"""
    H, W = int(H), int(W)
    fx, fy = (float(v) for v in torch.as_tensor(K).reshape(-1)[:2])
    view, proj, campos = camera_matrices(w2c, K, H, W)
    st = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=math.tan(2 * math.atan(W / (2 * fx)) * 0.5),      # (as Camera's FoVx)
                                       tanfovy=math.tan(2 * math.atan(H / (2 * fy)) * 0.5), kernel_size=0.0,
                                       bg=torch.tensor([float(v) for v in bg]), scale_modifier=1.0, viewmatrix=view, projmatrix=proj,
                                       sh_degree=cloud.sh_degree, campos=campos, prefiltered=False, require_coord=True, require_depth=True,
                                       debug=False)
    means2D = torch.zeros_like(cloud.get_xyz)
    color, radii, coord, mcoord, depth, mdepth, alpha, normal = GaussianRasterizer(st)(
        means3D=cloud.get_xyz, means2D=means2D, opacities=cloud.get_opacity, shs=cloud.get_features, scales=cloud.get_scaling,
        rotations=cloud.get_rotation)
    return {"render": color, "mask": alpha, "expected_coord": coord, "median_coord": mcoord, "depth": depth, "median_depth": mdepth,
            "viewspace_points": means2D, "visibility_filter": radii > 0, "radii": radii, "normal": normal, "n_touched": None}


def render_frames(cloud, w2c, K, H, W, layers=LAYERS, depth_range=None, bg=(0, 0, 0)):
    """{layer: uint8 [H,W,3] device tensor} of one camera (render_cloud, then ops.gs_frame per layer)"""
    for name in layers:
        if name not in LAYERS:
            raise ValueError(f"layer {name!r}: one of {LAYERS}")
    pkg = render_cloud(cloud, w2c, K, H, W, bg)
    return {name: ops.gs_frame(pkg[_SOURCE[name]].contiguous(), name, depth_range if name == "depth" else None) for name in layers}


def read_calib(text):
    """fx fy cx cy from a string of four numbers or from a file whose first four numbers they are"""
    try:
        vals = [float(v) for v in text.split()]
    except ValueError:
        vals = []
    if len(vals) != 4:
        if not os.path.isfile(text):
            raise ValueError(f"--calib: four numbers `fx fy cx cy` or a file, got {text!r}")
        vals = [float(v) for v in np.loadtxt(text).reshape(-1)[:4]]
        if len(vals) != 4:
            raise ValueError(f"{text}: fewer than four numbers")
    if not (all(math.isfinite(v) for v in vals) and vals[0] > 0 and vals[1] > 0):
        raise ValueError(f"--calib: finite values with fx, fy > 0, got {vals}")
    return vals


def main(argv=None):
    import argparse

    from PIL import Image

    from .gs_ply import GaussianCloud
    p = argparse.ArgumentParser(prog="python -m cut3r_slam_amd.gs_view", description=__doc__.split("\n\n")[0])
    p.add_argument("map", help="a standard 3DGS .ply (3dgs_final.ply)")
    p.add_argument("--traj", required=True, help="TUM rows `t tx ty tz qx qy qz qw`, camera to world (traj_kf.txt / traj_full.txt)")
    p.add_argument("--calib", required=True, help='"fx fy cx cy" or a file that starts with them, at the size of --size')
    p.add_argument("--size", type=int, nargs=2, required=True, metavar=("H", "W"))
    p.add_argument("--out", required=True)
    p.add_argument("--every", type=int, default=1)
    p.add_argument("--layers", nargs="+", default=["rgb"], choices=LAYERS)
    p.add_argument("--depth-range", type=float, nargs=2, default=None, metavar=("NEAR", "FAR"), help="default: every frame's own range")
    p.add_argument("--device", default="cuda:0")
    args = p.parse_args(argv)
    H, W = args.size
    if H < 1 or W < 1 or args.every < 1:
        p.error("--size and --every must be >= 1")
    K = read_calib(args.calib)
    rows = np.loadtxt(args.traj, ndmin=2)
    w2c = views.inverse44(views.tum_matrices(rows))
    cloud = GaussianCloud.from_ply(args.map, args.device)
    os.makedirs(args.out, exist_ok=True)
    n = 0
    for i in range(0, len(w2c), args.every):
        frames = render_frames(cloud, w2c[i], K, H, W, args.layers, args.depth_range)
        for name, img in frames.items():
            Image.fromarray(img.cpu().numpy()).save(os.path.join(args.out, f"{i:05d}_{name}.png"))
        n += 1
    print(f"{n} views x {len(args.layers)} layers of {len(cloud)} Gaussians (SH degree {cloud.sh_degree}) -> {args.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
