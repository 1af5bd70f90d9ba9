"""Reconstruction metrics of a mesh against a ground-truth mesh on the gfx950 kernels of csrc/recon.hip: the 3-D half of the reference's
scripts/eval_recon.py (accuracy, completion, completion ratio over 200 000 surface samples per mesh, after a point-to-point ICP of the
mesh vertices onto the GT vertices) and the clipped Chamfer distances of geometry_eval_utils.py:79-110.

  sample_surface         area-weighted uniform samples (trimesh.sample.sample_surface), counter-based: sample i depends on (seed, stream, i)
  accuracy / completion / completion_ratio     mean distance rec -> GT, GT -> rec, share of GT samples closer than dist_th (strict <)
  get_align_transformation                     Open3D registration_icp point-to-point with its defaults, as eval_recon.py:44-58 calls it
  calc_3d_metric / eval_recon                  eval_recon.py:92-116 (cm and %)
  chamfer_distance / chamfer_distance_RMSE     geometry_eval_utils.py:79-110
  voxel_down_sample                            Open3D's PointCloud.voxel_down_sample (eval7_scenes_dense.py:238-250), output sorted by voxel
  sim3_from_trajectories                       the Sim(3) that run_replica.py:45-46 applies to the mesh before it is scored

Every nearest-neighbour distance is the fp64 sqrt of the kernel's exact fp32 squared distance; means are fp64.  Inputs: a tsdf.Mesh, a PLY
path (tsdf.read_ply) or, for point sets, an [N,3] array or tensor.  CLI: python -m cut3r_slam_amd.eval_recon REC.ply GT.ply.
"""
from __future__ import annotations

import argparse
import math
import os
from typing import NamedTuple

import numpy as np
import torch

from . import ops
from .eval_ate import associate, load_tum, umeyama
from .tsdf import Mesh, read_ply

N_SAMPLES = 200000                 # eval_recon.py:104-107
STREAM_REC, STREAM_GT = 1, 2       # independent sample streams of the two meshes


def _device():
    return torch.device("cuda", torch.cuda.current_device())


def as_mesh(m) -> Mesh:
    if isinstance(m, Mesh):
        return m
    if isinstance(m, (str, os.PathLike)):
        return read_ply(m)
    raise TypeError(f"expected a tsdf.Mesh or a PLY path, got {type(m).__name__}")


def as_points(x) -> torch.Tensor:
    """[N,3] fp32 contiguous on the current GPU from a tensor, an array, a Mesh (its vertices) or a PLY path"""
    if isinstance(x, (Mesh, str, os.PathLike)):
        x = as_mesh(x).vertices
    t = torch.as_tensor(x)
    return t.to(_device(), torch.float32).reshape(-1, 3).contiguous()


def apply_transform(mesh, M) -> Mesh:
    """the mesh with vertices M[:3,:3] v + M[:3,3] (fp64, then fp32), as trimesh's apply_transform / Open3D's transform"""
    mesh = as_mesh(mesh)
    M = np.asarray(M, np.float64).reshape(4, 4)
    v = mesh.vertices.astype(np.float64) @ M[:3, :3].T + M[:3, 3]
    return Mesh(v.astype(np.float32), mesh.colors, mesh.faces)


def sample_surface(mesh, count, seed=0, stream=0) -> torch.Tensor:
    """count points [count,3] fp32 on the GPU, uniform over the mesh surface (trimesh.sample.sample_surface)"""
    mesh = as_mesh(mesh)
    v = as_points(mesh.vertices)
    f = torch.as_tensor(np.ascontiguousarray(mesh.faces, np.int32)).to(v.device).reshape(-1, 3).contiguous()
    _, cdf = ops.mesh_area_cdf(v, f)
    return ops.mesh_sample(v, f, cdf, count, seed=seed, stream_id=stream)


def _nn_dist(ref, query, max_dist=None) -> torch.Tensor:
    """fp64 distance of every query point to its nearest reference point (+inf beyond max_dist)"""
    d2, _ = ops.nn_query(as_points(ref), as_points(query), max_dist=max_dist)
    return d2.double().sqrt()


def completion_ratio(gt_points, rec_points, dist_th=0.05):
    return float((_nn_dist(rec_points, gt_points) < dist_th).double().mean())


def accuracy(gt_points, rec_points):
    return float(_nn_dist(gt_points, rec_points).mean())


def completion(gt_points, rec_points):
    return float(_nn_dist(rec_points, gt_points).mean())


# ---------------------------------------------------------------------------------------------------------------------------- ICP
class ICPResult(NamedTuple):
    transformation: np.ndarray     # fp64 [4,4], source -> target
    fitness: float                 # correspondences / source points
    inlier_rmse: float             # sqrt(mean d2) over the correspondences (0 without any)
    iterations: int


def rigid_from_moments(m) -> np.ndarray:
    """the least-squares rigid motion src -> dst from the fp64 moments of NNGrid.moments (eval_ate.umeyama with with_scale=False,
    restated on sums: cov = sum(dst src^T) / n - mu_dst mu_src^T); identity without correspondences (Open3D's behaviour)"""
    m = np.asarray(m, np.float64)
    n = m[0]
    T = np.eye(4)
    if n <= 0:
        return T
    mu_s, mu_d = m[2:5] / n, m[5:8] / n
    cov = m[8:17].reshape(3, 3).T / n - np.outer(mu_d, mu_s)
    U, _, Vt = np.linalg.svd(cov)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1
    R = U @ S @ Vt
    T[:3, :3] = R
    T[:3, 3] = mu_d - R @ mu_s
    return T


def icp_point_to_point(source, target, threshold, init=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6) -> ICPResult:
    """Open3D registration_icp with TransformationEstimationPointToPoint and ICPConvergenceCriteria's defaults: correspondences (d2 <=
    threshold^2), update, T = update @ T, correspondences again, stop when fitness and inlier RMSE both moved by less than the criteria.
    The source is never rewritten: the kernel applies fp32(T) to each source point as it loads it."""
    src, dst = as_points(source), as_points(target)
    grid = ops.NNGrid(dst, src.shape[0])
    T = np.eye(4) if init is None else np.asarray(init, np.float64).reshape(4, 4).copy()

    def evaluate(T):
        d2, idx = grid.query(src, max_dist=threshold, transform=T)
        m = grid.moments(src, d2, idx, transform=T).cpu().numpy()
        n = m[0]
        return m, n / src.shape[0], (math.sqrt(m[1] / n) if n > 0 else 0.0)

    m, fitness, rmse = evaluate(T)
    it = 0
    for i in range(max_iteration):
        T = rigid_from_moments(m) @ T
        prev_fitness, prev_rmse = fitness, rmse
        m, fitness, rmse = evaluate(T)
        it = i + 1
        if abs(prev_fitness - fitness) < relative_fitness and abs(prev_rmse - rmse) < relative_rmse:
            break
    return ICPResult(T, float(fitness), float(rmse), it)


def get_align_transformation(rec_mesh, gt_mesh) -> ICPResult:
    """eval_recon.py:44-58: ICP of the rec mesh's vertices onto the GT mesh's vertices, threshold 0.1, identity start"""
    return icp_point_to_point(as_mesh(rec_mesh).vertices, as_mesh(gt_mesh).vertices, 0.1, np.eye(4))


def calc_3d_metric(rec_mesh, gt_mesh, align=True, samples=N_SAMPLES, seed=0):
    """eval_recon.py:92-116: {'accuracy' (cm), 'completion' (cm), 'completion_ratio' (%, at 5 cm)}"""
    rec, gt = as_mesh(rec_mesh), as_mesh(gt_mesh)
    if align:
        rec = apply_transform(rec, get_align_transformation(rec, gt).transformation)
    rec_pc = sample_surface(rec, samples, seed=seed, stream=STREAM_REC)
    gt_pc = sample_surface(gt, samples, seed=seed, stream=STREAM_GT)
    acc = accuracy(gt_pc, rec_pc)
    d = _nn_dist(rec_pc, gt_pc)                                   # completion and completion_ratio share the GT -> rec search
    comp, ratio = float(d.mean()), float((d < 0.05).double().mean())
    return {"accuracy": acc * 100, "completion": comp * 100, "completion_ratio": ratio * 100}


def eval_recon(rec_mesh, gt_mesh, eval_3d=True, align=True, samples=N_SAMPLES, seed=0):
    """eval_recon.py:226-250 without the 2-D depth metric and the external run_evaluation"""
    result = {}
    if eval_3d:
        result.update(calc_3d_metric(rec_mesh, gt_mesh, align=align, samples=samples, seed=seed))
    return result


# ----------------------------------------------------------------------------------------------------------------------- Chamfer
def _clipped(ref, est, max_error):
    # a limit just above max_error: every distance the clip keeps is found, the rest come back +inf and clip to max_error
    lim = float(max_error) * (1 + 1e-6)
    d1 = _nn_dist(ref, est, lim).clamp(0, max_error)               # kdtree_ref.query(est)
    d2 = _nn_dist(est, ref, lim).clamp(0, max_error)               # kdtree_est.query(ref)
    return d1, d2


def chamfer_distance(pcd_ref, pcd_est, max_error):
    """geometry_eval_utils.py:79-93 -> (chamfer, dist1, dist2)"""
    d1, d2 = _clipped(pcd_ref, pcd_est, max_error)
    cd = 0.5 * float(d1.mean()) + 0.5 * float(d2.mean())
    return cd, d1.cpu().numpy(), d2.cpu().numpy()


def chamfer_distance_RMSE(pcd_ref, pcd_est, max_error):
    """geometry_eval_utils.py:96-110 -> (chamfer, rmse_dist1, rmse_dist2, dist1, dist2)"""
    d1, d2 = _clipped(pcd_ref, pcd_est, max_error)
    r1, r2 = math.sqrt(float((d1 * d1).mean())), math.sqrt(float((d2 * d2).mean()))
    return 0.5 * r1 + 0.5 * r2, r1, r2, d1.cpu().numpy(), d2.cpu().numpy()


def voxel_down_sample(points, voxel):
    """Open3D PointCloud.voxel_down_sample: voxel index floor((p - (min - voxel / 2)) / voxel) in fp64, one output point per occupied
    voxel = the mean of its points, sorted by (ix, iy, iz).  fp64 [M,3] on the input's device."""
    p = torch.as_tensor(points).to(torch.float64).reshape(-1, 3)
    if not voxel > 0:
        raise ValueError("voxel must be > 0")
    if p.shape[0] == 0:
        return p
    lo = p.min(0).values - voxel * 0.5
    key = torch.floor((p - lo) / voxel).long()
    uniq, inv = torch.unique(key, dim=0, return_inverse=True)
    acc = torch.zeros(uniq.shape[0], 3, dtype=torch.float64, device=p.device).index_add_(0, inv, p)
    cnt = torch.zeros(uniq.shape[0], dtype=torch.float64, device=p.device).index_add_(0, inv, torch.ones_like(p[:, 0]))
    return acc / cnt[:, None]


# --------------------------------------------------------------------------------------------------------------------- Sim(3)
def sim3_from_trajectories(est_tum, gt_tum, max_diff=0.01) -> np.ndarray:
    """the 4x4 Sim(3) (s R | t) aligning the estimated keyframe positions to the ground truth (evo -as, run_replica.py:45-46): a monocular
    mesh has no metric scale and rigid ICP cannot fix it.  est_tum / gt_tum: TUM files or [n,8] arrays."""
    est = load_tum(est_tum) if isinstance(est_tum, (str, os.PathLike)) else np.asarray(est_tum, np.float64)
    gt = load_tum(gt_tum) if isinstance(gt_tum, (str, os.PathLike)) else np.asarray(gt_tum, np.float64)
    ie, ig = associate(est, gt, max_diff)
    if len(ie) < 3:
        raise ValueError(f"only {len(ie)} associated poses (max_diff {max_diff})")
    s, R, t = umeyama(est[ie, 1:4], gt[ig, 1:4], with_scale=True)
    M = np.eye(4)
    M[:3, :3] = s * R
    M[:3, 3] = t
    return M


# ------------------------------------------------------------------------------------------------------------------------- CLI
def parse_args(argv=None):
    p = argparse.ArgumentParser(description="3-D reconstruction metrics of a mesh against a ground-truth mesh (scripts/eval_recon.py)")
    p.add_argument("rec_mesh", type=str, help="reconstructed mesh (binary PLY)")
    p.add_argument("gt_mesh", type=str, help="ground-truth mesh (binary PLY)")
    p.add_argument("--eval_3d", action="store_true", help="accepted for compatibility: the 3-D metric is the only one built")
    p.add_argument("--save", type=str, default=None, help="write the result dict as f'{result}' (ast.literal_eval reads it back)")
    p.add_argument("--no-align", action="store_true", help="skip the ICP alignment of the rec mesh onto the GT mesh")
    p.add_argument("--transform", type=str, default=None, help="4x4 .npy applied to the rec mesh first")
    p.add_argument("--traj-est", type=str, default=None, help="TUM trajectory of the run (with --traj-gt: Sim(3) applied to the rec mesh)")
    p.add_argument("--traj-gt", type=str, default=None, help="TUM ground-truth trajectory")
    p.add_argument("--samples", type=int, default=N_SAMPLES, help="surface samples per mesh")
    p.add_argument("--seed", type=int, default=0)
    a = p.parse_args(argv)
    if (a.traj_est is None) != (a.traj_gt is None):
        p.error("--traj-est and --traj-gt go together")
    if a.samples <= 0:
        p.error("--samples must be > 0")
    return a


def main(argv=None):
    a = parse_args(argv)
    rec = read_ply(a.rec_mesh)
    if a.transform is not None:
        rec = apply_transform(rec, np.load(a.transform))
    if a.traj_est is not None:
        rec = apply_transform(rec, sim3_from_trajectories(a.traj_est, a.traj_gt))
    result = eval_recon(rec, a.gt_mesh, eval_3d=True, align=not a.no_align, samples=a.samples, seed=a.seed)
    print(result)
    if a.save:
        with open(a.save, "w") as fh:
            fh.write(f"{result}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
