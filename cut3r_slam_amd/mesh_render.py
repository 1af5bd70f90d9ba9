"""Depth images of a triangle mesh and what follows from them, on the gfx950 rasteriser of csrc/raster.hip.

  render_depth        depth [B,H,W] (and the face seen) of a mesh from B cameras
  visible_vertices    which vertices a set of cameras sees
  cull_mesh           the part of a mesh a trajectory saw
  unseen_points       surface samples of the part it did not see

The reference's 2-D metric (scripts/eval_recon.py:151-154) reads two files it never makes: a GT mesh culled to what the camera
trajectory saw (data/Replica/gt_mesh_culled/*.ply) and a point cloud of the rest (*_pc_unseen.npy), both produced by an outside
culling script that the reference does not ship.  The visibility rule here and its eps are therefore OURS, not a port: a vertex is seen
when in some view it projects inside the image, lies within (0, z_far] and is at most eps behind the mesh's own rendered depth at its
nearest pixel; a face is kept when one of its vertices is seen.

CLI: python -m cut3r_slam_amd.mesh_render cull GT.ply TRAJ_TUM.txt --calib "fx fy cx cy" --size H W --out DIR
     -> DIR/<name>_culled.ply, DIR/<name>_pc_unseen.npy
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

from . import ops, views
from .eval_ate import load_tum
from .eval_recon import _gpu_mesh, as_mesh, sample_surface
from .tsdf import Mesh, write_ply
from .views import tum_matrices as tum_to_c2w          # [n,4,4] camera-to-world from TUM rows (t x y z qx qy qz qw)

EPS = 0.03                         # metres a vertex may lie behind the rendered surface and still count as seen
UNSEEN_POINTS = 200000
STREAM_UNSEEN = 3                  # sample stream of unseen_points (1 and 2 are the metric's two meshes)


def render_depth(mesh, c2w, K, H, W, z_near=0.0, z_far=20.0, face_id=False):
    """depth [B,H,W] fp32 on the GPU (0 = nothing hit) of a tsdf.Mesh or PLY path from the cameras c2w [B,4,4] (OpenCV axes), K = fx fy cx
    cy (one row, or one per view); with face_id=True also the int32 index of the face seen (-1 = nothing).  See ops.mesh_raster."""
    v, f = _gpu_mesh(as_mesh(mesh))
    return ops.mesh_raster(v, f, views.inverse44(c2w)[:, :3], K, H, W, z_near=z_near, z_far=z_far, face_id=face_id)


def visible_vertices(mesh, w2c, K, H, W, eps=EPS, z_far=20.0) -> np.ndarray:
    """bool [V]: the vertices seen by one of the cameras w2c [B,3,4] / [B,4,4] (any B: 16 views are rendered and tested per launch, the
    flags OR-ed across the batches)"""
    v, f = _gpu_mesh(as_mesh(mesh))
    w2c = views.pose_rows(w2c)
    K = views.intrinsics(K, len(w2c))
    flags = torch.zeros(v.shape[0], dtype=torch.uint8, device=v.device)
    for b0 in range(0, len(w2c), ops.RASTER_MAX_VIEWS):
        w, k = w2c[b0:b0 + ops.RASTER_MAX_VIEWS], K[b0:b0 + ops.RASTER_MAX_VIEWS]
        depth = ops.mesh_raster(v, f, w, k, H, W, z_far=z_far)
        ops.mesh_vertex_visible(v, depth, w, k, eps=eps, z_far=z_far, flags=flags)
    return flags.cpu().numpy().astype(bool)


def _split(mesh, seen):
    """bool [F]: the faces with at least one seen vertex"""
    return seen[mesh.faces].any(1)


def cull_mesh(mesh, w2c, K, H, W, eps=EPS, z_far=20.0) -> Mesh:
    """the faces with at least one seen vertex, their vertices re-indexed in the original order"""
    mesh = as_mesh(mesh)
    keep = _split(mesh, visible_vertices(mesh, w2c, K, H, W, eps=eps, z_far=z_far))
    return _submesh(mesh, keep)


def _submesh(mesh, keep) -> Mesh:
    faces = mesh.faces[keep]
    used = np.zeros(len(mesh.vertices), bool)
    used[faces.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return Mesh(mesh.vertices[used], mesh.colors[used], remap[faces].astype(np.int32).reshape(-1, 3))


def unseen_points(mesh, w2c, K, H, W, count=UNSEEN_POINTS, seed=0, eps=EPS, z_far=20.0) -> np.ndarray:
    """[count,3] fp32 surface samples (eval_recon.sample_surface) of the faces cull_mesh removes: the *_pc_unseen.npy of the 2-D metric;
    [0,3] when every face is seen"""
    mesh = as_mesh(mesh)
    keep = _split(mesh, visible_vertices(mesh, w2c, K, H, W, eps=eps, z_far=z_far))
    rest = _submesh(mesh, ~keep)
    if len(rest.faces) == 0:
        return np.zeros((0, 3), np.float32)
    return sample_surface(rest, count, seed=seed, stream=STREAM_UNSEEN).cpu().numpy()


def main(argv=None):
    p = argparse.ArgumentParser(description="what a camera trajectory saw of a mesh (the culling rule is this project's, see the module text)")
    sub = p.add_subparsers(dest="cmd", required=True)
    c = sub.add_parser("cull", help="write <name>_culled.ply and <name>_pc_unseen.npy")
    c.add_argument("mesh", type=str, help="mesh (binary PLY)")
    c.add_argument("traj", type=str, help="TUM trajectory of camera-to-world poses")
    c.add_argument("--calib", type=str, required=True, help='"fx fy cx cy"')
    c.add_argument("--size", type=int, nargs=2, required=True, metavar=("H", "W"))
    c.add_argument("--out", type=str, required=True)
    c.add_argument("--eps", type=float, default=EPS)
    c.add_argument("--z-far", type=float, default=20.0)
    c.add_argument("--count", type=int, default=UNSEEN_POINTS, help="points of the unseen cloud")
    c.add_argument("--seed", type=int, default=0)
    a = p.parse_args(argv)
    K = [float(x) for x in a.calib.replace(",", " ").split()]
    if len(K) != 4:
        p.error("--calib takes four numbers")
    H, W = a.size
    mesh = as_mesh(a.mesh)
    w2c = views.inverse44(tum_to_c2w(load_tum(a.traj)))[:, :3]
    keep = _split(mesh, visible_vertices(mesh, w2c, K, H, W, eps=a.eps, z_far=a.z_far))
    os.makedirs(a.out, exist_ok=True)
    name = os.path.splitext(os.path.basename(a.mesh))[0]
    write_ply(os.path.join(a.out, f"{name}_culled.ply"), _submesh(mesh, keep))
    rest = _submesh(mesh, ~keep)
    pts = sample_surface(rest, a.count, seed=a.seed, stream=STREAM_UNSEEN).cpu().numpy() if len(rest.faces) else np.zeros((0, 3), np.float32)
    np.save(os.path.join(a.out, f"{name}_pc_unseen.npy"), pts)
    print(f"{len(w2c)} views: {int(keep.sum())} of {len(keep)} faces seen -> {a.out}/{name}_culled.ply, {len(pts)} unseen points")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
