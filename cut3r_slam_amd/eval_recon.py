"""Reconstruction metrics of a mesh against a ground-truth mesh on the gfx950 kernels of csrc/recon.hip and csrc/raster.hip: the 3-D half
of the reference's scripts/eval_recon.py (accuracy, completion, completion ratio over 200 000 surface samples per mesh, after a
point-to-point ICP of the mesh vertices onto the GT vertices), its 2-D half (the depth L1 between renders of the two meshes from random
viewpoints inside the room) and the clipped Chamfer distances of geometry_eval_utils.py:79-110.

  sample_surface         area-weighted uniform samples (trimesh.sample.sample_surface), counter-based: sample i depends on (seed, stream, i)
  accuracy / completion / completion_ratio     mean distance rec -> GT, GT -> rec, share of GT samples closer than dist_th (strict <)
  get_align_transformation                     Open3D registration_icp point-to-point with its defaults, as eval_recon.py:44-58 calls it
  calc_3d_metric / eval_recon                  eval_recon.py:92-116 (cm and %)
  check_proj / get_cam_position / sample_views / calc_2d_metric     eval_recon.py:60-89, 118-223 ('depth l1' in cm)
  chamfer_distance / chamfer_distance_RMSE     geometry_eval_utils.py:79-110
  voxel_down_sample                            Open3D's PointCloud.voxel_down_sample (eval7_scenes_dense.py:238-250), output sorted by voxel
  sim3_from_trajectories                       the Sim(3) that run_replica.py:45-46 applies to the mesh before it is scored
  run_evaluation / precision_recall / align_coarse_to_fine     evaluate_3d_reconstruction.run_evaluation (eval_recon.py:232-235): the keys
                                               run_replica.py:54-57 reads; written from the published Tanks-and-Temples evaluation

The evaluation against ground-truth DEPTH MAPS instead of a mesh (scripts/eval7_scenes_dense.py) is cut3r_slam_amd/eval_dense.py; it uses
icp_point_to_point and chamfer_distance_RMSE from here and the GPU voxel downsample ops.voxel_downsample.

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


def sim3_from_moments(m) -> np.ndarray:
    """the least-squares similarity src -> dst, 4x4 (s R | t), from the fp64 moments of NNGrid.moments_scaled (eval_ate.umeyama with
    with_scale=True restated on sums: the variance of src = sum |src|^2 / n - |mu_src|^2, s = trace(D S) / variance); identity without
    correspondences, and the rigid motion (s = 1) when the source points coincide (variance <= 1e-12 of the mean |src|^2)"""
    m = np.asarray(m, np.float64)
    n = m[0]
    T = np.eye(4)
    if n <= 0:
        return T
    mu_s, mu_d = m[2:5] / n, m[5:8] / n
    cov = m[8:17].reshape(3, 3).T / n - np.outer(mu_d, mu_s)
    var = m[17] / n - mu_s @ mu_s
    U, D, Vt = np.linalg.svd(cov)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1
    R = U @ S @ Vt
    s = float(np.trace(np.diag(D) @ S) / var) if var > 1e-12 * m[17] / n else 1.0       # below: the rounding of the subtraction
    T[:3, :3] = s * R
    T[:3, 3] = mu_d - s * R @ mu_s
    return T


def icp_point_to_point(source, target, threshold, init=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6,
                       with_scaling=False) -> ICPResult:
    """Open3D registration_icp with TransformationEstimationPointToPoint and ICPConvergenceCriteria's defaults: correspondences (d2 <=
    threshold^2), update, T = update @ T, correspondences again, stop when fitness and inlier RMSE both moved by less than the criteria.
    The source is never rewritten: the kernel applies fp32(T) to each source point as it loads it.  with_scaling: the update is the
    similarity of sim3_from_moments (TransformationEstimationPointToPoint(with_scaling=True)), T = [s R | t] @ T."""
    src, dst = as_points(source), as_points(target)
    grid = ops.NNGrid(dst, src.shape[0])
    T = np.eye(4) if init is None else np.asarray(init, np.float64).reshape(4, 4).copy()
    moments, update = (grid.moments_scaled, sim3_from_moments) if with_scaling else (grid.moments, rigid_from_moments)

    def evaluate(T):
        d2, idx = grid.query(src, max_dist=threshold, transform=T)
        m = moments(src, d2, idx, transform=T).cpu().numpy()
        n = m[0]
        return m, n / src.shape[0], (math.sqrt(m[1] / n) if n > 0 else 0.0)

    m, fitness, rmse = evaluate(T)
    it = 0
    for i in range(max_iteration):
        T = update(m) @ T
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


def eval_recon(rec_mesh, gt_mesh, eval_3d=True, align=True, samples=N_SAMPLES, seed=0, eval_2d=False, n_imgs=10, unseen=None, pr=False,
               pr_thresh=0.05, pr_scale=False, pr_out=None):
    """eval_recon.py:226-250; the 2-D depth metric (n_imgs views, 10 as eval_recon.py:238) only with eval_2d, the keys of the external
    run_evaluation (eval_recon.py:232-235: precision, recall, F-score) only with pr"""
    result = {}
    if eval_3d:
        result.update(calc_3d_metric(rec_mesh, gt_mesh, align=align, samples=samples, seed=seed))
    if pr:
        result.update(run_evaluation(rec_mesh, gt_mesh, distance_thresh=pr_thresh, icp_align=align, with_scaling=pr_scale, samples=samples,
                                     seed=seed, out_dir=pr_out))
    if eval_2d:
        result.update(calc_2d_metric(rec_mesh, gt_mesh, align=align, n_imgs=n_imgs, unseen=unseen, seed=seed))
    return result


# ------------------------------------------------------------------------------------------------- precision, recall, F-score
# evaluate_3d_reconstruction.run_evaluation (eval_recon.py:9,232-235) is the Tanks-and-Temples evaluation; its library is not available
# here, so what follows is written from the published evaluation and PARITY WITH THE LIBRARY IS UNPINNED.  What is pinned is the rule
# stated here, against tests/pr_oracle.py.
class PRResult(NamedTuple):
    precision: float               # share of the rec points closer than tau to the GT cloud (strict <)
    recall: float                  # share of the GT points closer than tau to the rec cloud
    fscore: float                  # 2 p r / (p + r), 0 when both are 0
    mean_rec: float                # rec -> GT distances: mean, median (the mean of the two middle ranks), population std, min, max
    median_rec: float
    std_rec: float
    min_rec: float
    max_rec: float
    mean_gt: float                 # GT -> rec distances
    median_gt: float
    std_gt: float
    min_gt: float
    max_gt: float
    edges: np.ndarray              # fp64 [nbins + 1] = arange(nbins + 1) * tau / bins_per_tau, nbins = stretch * bins_per_tau
    cum_rec: np.ndarray            # fp64 [nbins]: share of the rec points with d < edges[k + 1] (precision as a function of the threshold)
    cum_gt: np.ndarray             # fp64 [nbins]: the same for the GT points (recall)
    dist2_rec: torch.Tensor        # fp32 [n_rec] squared distance of every rec point to the GT cloud, on the GPU
    dist2_gt: torch.Tensor         # fp32 [n_gt]
    rec_points: torch.Tensor       # fp32 [n_rec,3] the (downsampled) clouds the distances belong to, on the GPU
    gt_points: torch.Tensor        # fp32 [n_gt,3]


def _one_way(dist2, tau, w, nbins):
    counts, moments, hist = ops.dist_stats(dist2, tau, w, nbins)
    med = ops.dist_median(dist2)
    counts, moments, hist, med = counts.cpu().numpy(), moments.cpu().numpy(), hist.cpu().numpy(), med.cpu().numpy().astype(np.float64)
    good, below, bad = (int(c) for c in counts)
    if bad:
        raise ValueError(f"{bad} of {len(dist2)} nearest-neighbour distances are NaN, negative or infinite")
    mean = moments[0] / good
    std = math.sqrt(max(moments[1] / good - mean * mean, 0.0))
    median = 0.5 * (math.sqrt(med[0]) + math.sqrt(med[1]))
    return below / good, (float(mean), float(median), std, float(moments[2]), float(moments[3])), np.cumsum(hist).astype(np.float64) / good


def precision_recall(rec_pts, gt_pts, tau=0.05, voxel=None, stretch=5, bins_per_tau=100) -> PRResult:
    """the two clouds are voxel-downsampled (ops.voxel_downsample; voxel=None: tau / 2, voxel=0: not at all), the exact nearest neighbour
    is searched both ways, and ops.dist_stats / ops.dist_median reduce the two sets of distances on the GPU.  The histograms have
    bins_per_tau bins per tau out to stretch * tau (at most 4096 bins); a distance beyond it counts in the means but in no bin."""
    tau = float(tau)
    nbins = int(stretch) * int(bins_per_tau)
    if not (tau > 0 and 0 < nbins <= ops.DIST_STATS_MAX_BINS):
        raise ValueError(f"tau must be > 0 and stretch * bins_per_tau in 1 .. {ops.DIST_STATS_MAX_BINS}")
    voxel = 0.5 * tau if voxel is None else float(voxel)
    rec, gt = as_points(rec_pts), as_points(gt_pts)
    if voxel > 0:
        rec, gt = ops.voxel_downsample(rec, voxel)[0], ops.voxel_downsample(gt, voxel)[0]
    w = tau / int(bins_per_tau)
    d2_rec, _ = ops.nn_query(gt, rec)
    d2_gt, _ = ops.nn_query(rec, gt)
    p, s_rec, cum_rec = _one_way(d2_rec, tau, w, nbins)
    r, s_gt, cum_gt = _one_way(d2_gt, tau, w, nbins)
    f = 2 * p * r / (p + r) if p + r > 0 else 0.0
    return PRResult(p, r, f, *s_rec, *s_gt, np.arange(nbins + 1, dtype=np.float64) * w, cum_rec, cum_gt, d2_rec, d2_gt, rec, gt)


def align_coarse_to_fine(rec_pts, gt_pts, tau, with_scaling=False) -> np.ndarray:
    """the published registration schedule, rec -> GT, 4x4: ICP on the clouds downsampled at voxel tau with threshold 80 tau, on the clouds
    at voxel tau / 2 with threshold 20 tau, and on those again with threshold 2 tau; 20 iterations each, each from the result before.  The
    clouds are downsampled once, as they come (the library downsamples the source after moving it by the running estimate)."""
    tau = float(tau)
    rec, gt = as_points(rec_pts), as_points(gt_pts)
    coarse = ops.voxel_downsample(rec, tau)[0], ops.voxel_downsample(gt, tau)[0]
    fine = ops.voxel_downsample(rec, 0.5 * tau)[0], ops.voxel_downsample(gt, 0.5 * tau)[0]
    T = np.eye(4)
    for (src, dst), threshold in ((coarse, 80 * tau), (fine, 20 * tau), (fine, 2 * tau)):
        T = icp_point_to_point(src, dst, threshold, T, max_iteration=20, with_scaling=with_scaling).transformation
    return T


def transform_points(points, M) -> torch.Tensor:
    """fp32 [N,3]: ((M00 x + M01 y) + M02 z) + M03 per row in fp64, every product and sum rounded on its own, then rounded to fp32"""
    p = as_points(points).double()
    M = np.asarray(M, np.float64).reshape(4, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return torch.stack([((x * M[r, 0] + y * M[r, 1]) + z * M[r, 2]) + M[r, 3] for r in range(3)], 1).float().contiguous()


HOT_R = ((0.0, (1.0, 1.0, 1.0)), (1 - 0.746032, (1.0, 1.0, 0.0)), (1 - 0.365079, (1.0, 0.0, 0.0)), (1.0, (0.0416, 0.0, 0.0)))


def error_colors(dist, tau) -> torch.Tensor:
    """uint8 [N,3]: x = min(d, 3 tau) / (3 tau) through matplotlib's "hot" reversed, i.e. linear between white at x = 0, (1, 1, 0) at
    1 - 0.746032, (1, 0, 0) at 1 - 0.365079 and (0.0416, 0, 0) at x = 1 (hot's breakpoints; matplotlib's 256-entry table is not
    reproduced), each channel floor(255 c + 0.5)"""
    d = torch.as_tensor(dist, dtype=torch.float64)
    x = torch.clamp(d, max=3 * float(tau)) / (3 * float(tau))
    c = torch.zeros(x.shape + (3,), dtype=torch.float64, device=x.device)
    for (x0, c0), (x1, c1) in zip(HOT_R[:-1], HOT_R[1:]):
        inside = ((x >= x0) & (x <= x1))[..., None]
        u = ((x - x0) / (x1 - x0))[..., None]
        c = torch.where(inside, torch.tensor(c0, dtype=torch.float64, device=x.device) * (1 - u)
                        + torch.tensor(c1, dtype=torch.float64, device=x.device) * u, c)
    return torch.floor(255 * c + 0.5).to(torch.uint8)


def evaluate_points(rec_pts, gt_pts, tau=0.05, icp_align=True, with_scaling=False):
    """(PRResult, 4x4 applied to rec_pts): align_coarse_to_fine (identity without icp_align), then precision_recall at voxel tau / 2"""
    T = align_coarse_to_fine(rec_pts, gt_pts, tau, with_scaling) if icp_align else np.eye(4)
    moved = transform_points(rec_pts, T) if icp_align else as_points(rec_pts)
    return precision_recall(moved, gt_pts, tau), T


def pr_dict(res: PRResult) -> dict:
    """the keys of run_evaluation that the reference's scripts read: shares in %, distances in cm"""
    return {"precision": res.precision * 100, "recall": res.recall * 100, "f-score": res.fscore * 100,
            "mean precision": res.mean_rec * 100, "mean recall": res.mean_gt * 100,
            "median precision": res.median_rec * 100, "median recall": res.median_gt * 100}


def run_evaluation(rec_mesh, gt_mesh, distance_thresh=0.05, icp_align=True, with_scaling=False, samples=N_SAMPLES, seed=0, out_dir=None):
    """evaluate_3d_reconstruction.run_evaluation as eval_recon.py:232-235 calls it: `samples` surface samples per mesh (the streams of
    calc_3d_metric), the coarse-to-fine alignment of the rec samples onto the GT samples, precision / recall / F-score at distance_thresh
    over the clouds downsampled at half of it.  Returns plain floats: 'precision', 'recall', 'f-score' (%), 'mean precision', 'mean
    recall', 'median precision', 'median recall' (cm; "precision" distances run rec -> GT, "recall" distances GT -> rec).  out_dir:
    precision.ply / recall.ply (the downsampled rec / GT cloud coloured by error_colors) and pr_curve.txt (threshold, precision and
    recall up to it, one line per histogram edge); no plot."""
    rec_pc = sample_surface(rec_mesh, samples, seed=seed, stream=STREAM_REC)
    gt_pc = sample_surface(gt_mesh, samples, seed=seed, stream=STREAM_GT)
    res, _ = evaluate_points(rec_pc, gt_pc, distance_thresh, icp_align, with_scaling)
    if out_dir is not None:
        from .tsdf import write_ply
        os.makedirs(out_dir, exist_ok=True)
        for name, pts, d2 in (("precision", res.rec_points, res.dist2_rec), ("recall", res.gt_points, res.dist2_gt)):
            col = error_colors(d2.double().sqrt(), distance_thresh)
            write_ply(os.path.join(out_dir, f"{name}.ply"), Mesh(pts.cpu().numpy(), col.cpu().numpy(), np.zeros((0, 3), np.int32)))
        with open(os.path.join(out_dir, "pr_curve.txt"), "w") as fh:
            fh.write("# threshold precision recall\n")
            for e, p, r in zip(res.edges[1:], res.cum_rec, res.cum_gt):
                fh.write(f"{e:.9g} {p:.9g} {r:.9g}\n")
    return pr_dict(res)


# ------------------------------------------------------------------------------------------------------------------- 2-D metric
EDGE = 10                          # eval_recon.py:86
_M64 = (1 << 64) - 1


def _splitmix64(z):
    z = np.asarray(z, np.uint64) + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _uniform(seed, views, attempts, ncomp):
    """fp64 [len(views), ncomp] in [0, 1): the project's counter-based splitmix64 (csrc/recon.hip) with stream = view and counter =
    8 * try + component, 53 bits each"""
    with np.errstate(over="ignore"):
        key = _splitmix64(_splitmix64(np.array([int(seed) & _M64], np.uint64)) ^ np.asarray(views, np.uint64))
        ctr = np.uint64(8) * np.asarray(attempts, np.uint64)[:, None] + np.arange(ncomp, dtype=np.uint64)[None]
        h = _splitmix64(key[:, None] ^ ctr)
    return (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def check_proj(points, W, H, fx, fy, cx, cy, c2w) -> bool:
    """eval_recon.py:60-89: does the camera c2w see one of the points inside the image shrunk by 10 pixels.

    The reference negates the y and z columns of c2w, inverts, negates the camera x, multiplies by K, adds 1e-5 to the third component
    and tests `0 <= -z`.  With (x, y, z) the point in the plain OpenCV camera inv(c2w), its camera coordinates are (-x, -y, -z), K maps
    them to (-(fx x + cx z), -(fy y + cy z), -z), and the signs cancel in the division: u = (fx x + cx z) / z', v = (fy y + cy z) / z'
    with z' = z - 1e-5, tested as 0 <= z', 10 < u < W - 10, 10 < v < H - 10.  That is what cut3r_points_in_view evaluates (fp32)."""
    w2c = np.linalg.inv(np.asarray(c2w, np.float64).reshape(4, 4))[None, :3]
    return bool(int(ops.points_in_view(as_points(points), w2c, [fx, fy, cx, cy], H, W, EDGE)[0]) > 0)


def get_cam_position(gt_mesh):
    """(extents [3], transform [4,4]) of the box camera positions are drawn from (eval_recon.py:118-126).  DEVIATION: the reference takes
    trimesh's minimum-volume oriented box of the GT mesh; trimesh is not available here, so this is the axis-aligned box of the GT
    vertices, with the reference's three factors applied as 0.3 on the shortest axis and 0.7 on the other two and the centre raised by
    0.4 along world z.  For a room whose walls are not axis-aligned the two differ, and nobody has compared them: pass your own box to
    sample_views where it matters."""
    v = np.asarray(as_mesh(gt_mesh).vertices, np.float64)
    lo, hi = v.min(0), v.max(0)
    fac = np.full(3, 0.7)
    fac[np.argmin(hi - lo)] = 0.3
    T = np.eye(4)
    T[:3, 3] = 0.5 * (lo + hi)
    T[2, 3] += 0.4
    return (hi - lo) * fac, T


def viewmatrix(z, up, pos) -> np.ndarray:
    """eval_recon.py:129-135 as a 4x4 c2w: columns normalize(up x z), z x that, normalize(z), pos"""
    unit = lambda x: x / np.linalg.norm(x)
    v2 = unit(np.asarray(z, np.float64))
    v0 = unit(np.cross(up, v2))
    v1 = unit(np.cross(v2, v0))
    m = np.eye(4)
    m[:3] = np.stack([v0, v1, v2, np.asarray(pos, np.float64)], 1)
    return m


def sample_views(extents, transform, n, unseen=None, seed=0, max_tries=1000, W=500, H=500, focal=300.0) -> np.ndarray:
    """n camera poses c2w [n,4,4] (eval_recon.py:166-187): position uniform in the box (extents, transform), looking at a target uniform
    in [-10000, 10000]^3 rounded to 2 decimals, up (0, 0, -1); a candidate that sees one of the `unseen` points (check_proj) is redrawn.
    Candidate `try` of view k is a function of (seed, k, try) only, so view k does not depend on n.  The reference loops for ever when no
    candidate qualifies; here max_tries rejections in a row raise RuntimeError.  The candidates of one round are tested in one batch."""
    extents, transform = np.asarray(extents, np.float64).reshape(3), np.asarray(transform, np.float64).reshape(4, 4)
    out = np.zeros((int(n), 4, 4))
    pts = None if unseen is None or len(unseen) == 0 else as_points(unseen)
    K = [focal, focal, W / 2.0 - 0.5, H / 2.0 - 0.5]
    todo = np.arange(int(n))
    for attempt in range(int(max_tries)):
        if len(todo) == 0:
            break
        u = _uniform(seed, todo, np.full(len(todo), attempt), 6)
        pos = ((u[:, :3] - 0.5) * extents) @ transform[:3, :3].T + transform[:3, 3]
        target = np.array([[round(-10000.0 + 20000.0 * x, 2) for x in row] for row in u[:, 3:]]).reshape(-1, 3)
        c2w = np.stack([viewmatrix(t - p, np.array([0.0, 0.0, -1.0]), p) for t, p in zip(target, pos)]) if len(todo) else np.zeros((0, 4, 4))
        out[todo] = c2w
        if pts is None:
            todo = todo[:0]
            break
        seen = ops.points_in_view(pts, np.linalg.inv(c2w)[:, :3], K, H, W, EDGE).cpu().numpy() > 0
        todo = todo[seen]
    if len(todo):
        raise RuntimeError(f"view {int(todo[0])}: {max_tries} candidates in a row see the unseen region")
    return out


def _unseen_next_to(gt_mesh):
    if isinstance(gt_mesh, (str, os.PathLike)):
        path = os.path.splitext(os.fspath(gt_mesh))[0] + "_pc_unseen.npy"
        if os.path.isfile(path):
            return np.load(path)
    return None


def _gpu_mesh(mesh):
    v = as_points(mesh.vertices)
    return v, torch.as_tensor(np.ascontiguousarray(mesh.faces, np.int32)).to(v.device).reshape(-1, 3).contiguous()


def calc_2d_metric(rec_mesh, gt_mesh, align=True, n_imgs=1000, unseen=None, views=None, seed=0, H=500, W=500, focal=300):
    """eval_recon.py:138-223: {'depth l1' (cm)}.  Both meshes are rendered by cut3r_mesh_raster (z_far 20 as set_constant_z_far) from the
    same cameras: `views` [n,4,4] c2w when given, else n_imgs poses of sample_views in the box of get_cam_position(gt_mesh), redrawn
    while they see a point of `unseen` (an [N,3] array; None: <gt stem>_pc_unseen.npy next to a GT path, and no rejection when there is
    none).  Per view the mean |gt - ours| over the pixels with ours > 0 (a pixel where only the GT is empty counts with gt = 0); views
    where the reconstruction is empty are skipped; the mean over the others times 100, nan when none is left."""
    if unseen is None:
        unseen = _unseen_next_to(gt_mesh)
    rec, gt = as_mesh(rec_mesh), as_mesh(gt_mesh)
    if align:
        rec = apply_transform(rec, get_align_transformation(rec, gt).transformation)
    if views is None:
        extents, transform = get_cam_position(gt)
        views = sample_views(extents, transform, n_imgs, unseen=unseen, seed=seed, W=W, H=H, focal=focal)
    views = np.asarray(views, np.float64).reshape(-1, 4, 4)
    if len(views) == 0:
        return {"depth l1": float("nan")}
    w2c = np.linalg.inv(views)[:, :3]
    K = [focal, focal, W / 2.0 - 0.5, H / 2.0 - 0.5]
    gv, gf = _gpu_mesh(gt)
    rv, rf = _gpu_mesh(rec)
    sums = []
    for b0 in range(0, len(w2c), ops.RASTER_MAX_VIEWS):
        w = w2c[b0:b0 + ops.RASTER_MAX_VIEWS]
        sums.append(ops.depth_l1(ops.mesh_raster(gv, gf, w, K, H, W), ops.mesh_raster(rv, rf, w, K, H, W)))
    s = torch.cat(sums).cpu().numpy()
    ok = s[:, 0] > 0
    errors = s[ok, 1] / s[ok, 0]
    return {"depth l1": float(errors.mean() * 100) if len(errors) else float("nan")}


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
    p = argparse.ArgumentParser(description="reconstruction metrics of a mesh against a ground-truth mesh (scripts/eval_recon.py)")
    p.add_argument("rec_mesh", type=str, help="reconstructed mesh (binary PLY)")
    p.add_argument("gt_mesh", type=str, help="ground-truth mesh (binary PLY)")
    p.add_argument("--eval_3d", action="store_true", help="accepted for compatibility: the 3-D metric is always computed")
    p.add_argument("--eval_2d", action="store_true", help="also the 2-D metric: depth L1 of renders from random viewpoints inside the room")
    p.add_argument("--n-imgs", type=int, default=10, help="views of the 2-D metric (the reference's eval_recon uses 10, its tables 1000)")
    p.add_argument("--unseen", type=str, default=None, help="[N,3] .npy of GT points no sampled view may see (default: "
                   "<gt stem>_pc_unseen.npy when it exists)")
    p.add_argument("--save", type=str, default=None, help="write the result dict as f'{result}' (ast.literal_eval reads it back)")
    p.add_argument("--no-align", action="store_true", help="skip the ICP alignment of the rec mesh onto the GT mesh")
    p.add_argument("--transform", type=str, default=None, help="4x4 .npy applied to the rec mesh first")
    p.add_argument("--traj-est", type=str, default=None, help="TUM trajectory of the run (with --traj-gt: Sim(3) applied to the rec mesh)")
    p.add_argument("--traj-gt", type=str, default=None, help="TUM ground-truth trajectory")
    p.add_argument("--samples", type=int, default=N_SAMPLES, help="surface samples per mesh")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--pr", action="store_true", help="also precision, recall and F-score (the reference's external run_evaluation): the keys "
                   "'precision', 'recall', 'f-score' (%%), 'mean precision', 'mean recall', 'median precision', 'median recall' (cm)")
    p.add_argument("--pr-thresh", type=float, default=0.05, help="distance threshold of --pr, metres")
    p.add_argument("--pr-scale", action="store_true", help="the alignment of --pr also estimates a scale")
    p.add_argument("--pr-out", type=str, default=None, metavar="DIR", help="write precision.ply, recall.ply and pr_curve.txt of --pr here")
    a = p.parse_args(argv)
    if not a.pr and (a.pr_scale or a.pr_out is not None):
        p.error("--pr-scale and --pr-out belong to --pr")
    if not 0 < a.pr_thresh < float("inf"):
        p.error("--pr-thresh must be > 0 and finite")
    if (a.traj_est is None) != (a.traj_gt is None):
        p.error("--traj-est and --traj-gt go together")
    if a.samples <= 0:
        p.error("--samples must be > 0")
    if a.n_imgs <= 0:
        p.error("--n-imgs must be > 0")
    return a


def main(argv=None):
    a = parse_args(argv)
    rec = read_ply(a.rec_mesh)
    if a.transform is not None:
        rec = apply_transform(rec, np.load(a.transform))
    if a.traj_est is not None:
        rec = apply_transform(rec, sim3_from_trajectories(a.traj_est, a.traj_gt))
    extra = dict(eval_2d=True, n_imgs=a.n_imgs, unseen=None if a.unseen is None else np.load(a.unseen)) if a.eval_2d else {}
    if a.pr:
        extra.update(pr=True, pr_thresh=a.pr_thresh, pr_scale=a.pr_scale, pr_out=a.pr_out)
    result = eval_recon(rec, a.gt_mesh, eval_3d=True, align=not a.no_align, samples=a.samples, seed=a.seed, **extra)
    print(result)
    if a.save:
        with open(a.save, "w") as fh:
            fh.write(f"{result}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
