"""Dense point-cloud evaluation of a run's depth maps against ground-truth depth maps on the gfx950 kernels of csrc/cloud.hip and
csrc/recon.hip: the reference's scripts/eval7_scenes_dense.py:172-289, for the datasets that ship GT depth and poses but no GT mesh (TUM,
ScanNet, 7-Scenes).

  DepthViews                 a set of posed depth maps: depth [n,H,W] fp32 metres, c2w, K, stamps, optional rgb
  dense_metrics              associate stamps -> Sim(3) of the trajectories -> both clouds -> ICP on 5 cm voxel-downsampled clouds -> the
                             run's cloud re-emitted under ICP . Sim(3) . pose -> RMSE_acc, RMSE_comp, Chamfer_distance (clip 0.5 m)
  from_keyframes / from_mapper / load_depth_dir      the sources: the tracker's store, the Gaussian map's keyframe renders, a directory
                             of 16-bit depth PNGs with a TUM trajectory
  write_results              3D_eval_results.txt in the reference's `key: value` lines, optionally the two clouds as vertex-only PLY

Deviations from the reference, all stated in DESIGN.md section 4f: the clouds are fp32 (Open3D keeps doubles; every point is computed in
fp64 and rounded once); the nearest-neighbour resampling rule is the exact floor (ops.depth_cloud); the transforms are composed on the
host in fp64 and applied in one pass, where the reference transforms the stored cloud twice; the trajectory alignment is the exact
identity where the identity fits at least as well as umeyama's answer (trajectory_sim3).

CLI: python -m cut3r_slam_amd.eval_dense --est-depthdir D --est-traj traj_kf.txt --est-calib C --gtdepthdir G --gt-traj gt.txt --gt-calib C
"""
from __future__ import annotations

import argparse
import os
import re
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import ops
from .eval_ate import associate, load_tum, umeyama
from .eval_recon import chamfer_distance_RMSE, icp_point_to_point
from .stream import load_calib, natsorted
from .views import intrinsics, inverse44, pose_matrices, run_views

KEYS = ("RMSE_acc", "RMSE_comp", "Chamfer_distance")
DEPTH_SCALE = 6553.5               # the run's depth PNGs (eval7_scenes_dense.py:203)


class DepthViews(NamedTuple):
    depth: object                  # [n,H,W] fp32 metres (tensor or array)
    c2w: object                    # [n,4,4] / [n,3,4] camera-to-world, or TUM rows [n,8] (stamp t q_xyzw) / [n,7] (t q_xyzw)
    K: object                      # [4] or [n,4] fx fy cx cy of the H x W depth maps
    stamps: object                 # [n]
    rgb: Optional[object] = None   # u8 [n,3,H,W]


def _device():
    return torch.device("cuda", torch.cuda.current_device())


def grid_intrinsics(K, n, shape, size) -> np.ndarray:
    """fp64 [n,4]: the intrinsics of the H x W maps carried to the H1 x W1 sampling grid as vggt_resize does (eval7_scenes_dense.py:66-70):
    fx W1 / W, fy H1 / H, cx W1 / W, cy H1 / H"""
    K = intrinsics(K, n)
    if size is not None:
        (H, W), (H1, W1) = shape, size
        K[:, [0, 2]] = K[:, [0, 2]] / (W / W1)
        K[:, [1, 3]] = K[:, [1, 3]] / (H / H1)
    return K


def _views(v, name):
    v = DepthViews(*v)
    depth = torch.as_tensor(v.depth)
    if depth.dim() != 3 or depth.shape[0] == 0:
        raise ValueError(f"{name}: depth [n,H,W]")
    n = depth.shape[0]
    poses = pose_matrices(v.c2w)
    stamps = np.asarray(v.stamps.detach().cpu() if isinstance(v.stamps, torch.Tensor) else v.stamps, np.float64).reshape(-1)
    if len(poses) != n or len(stamps) != n:
        raise ValueError(f"{name}: {n} depth maps, {len(poses)} poses, {len(stamps)} stamps")
    rgb = None if v.rgb is None else torch.as_tensor(v.rgb)
    return depth, poses, v.K, stamps, rgb


def trajectory_sim3(src, dst):
    """(s, R, t) of the least-squares similarity dst ~ s R src + t of paired camera positions [n,3]: eval_ate.umeyama, except that the
    identity is returned where it fits at least as well.  umeyama reaches the minimum only up to the rounding of its SVD, so for
    trajectories that are already aligned (a run scored in the GT's frame, a cloud against itself) it gives the identity perturbed in
    the last bits, and that perturbation flips the fp32 rounding of a few points in a million; the identity's residual is then the
    smaller one, and it is the answer."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    s, R, t = umeyama(src, dst, with_scale=True)
    if float(((src - dst) ** 2).sum()) <= float((((s * (R @ src.T)).T + t - dst) ** 2).sum()):
        return 1.0, np.eye(3), np.zeros(3)
    return s, R, t


def _cloud(depth, rgb, idx, poses, K, trunc, size):
    dev = _device()
    sel = torch.as_tensor(np.asarray(idx), dtype=torch.long)
    d = depth[sel.to(depth.device)].to(dev, torch.float32).contiguous()
    c = None if rgb is None else rgb[sel.to(rgb.device)].to(dev, torch.uint8).contiguous()
    return ops.depth_cloud(d, poses, K, trunc, size=size, rgb=c)


def dense_metrics(est, gt, *, depth_trunc=4.5, est_depth_trunc=None, size=None, voxel=0.05, icp_threshold=0.1, max_error=0.5, max_diff=0.01,
                  icp=True, return_clouds=False):
    """eval7_scenes_dense.py:172-289 for two DepthViews -> {"RMSE_acc", "RMSE_comp", "Chamfer_distance", n_gt, n_est, pairs, scale,
    icp_fitness, icp_rmse, icp_iterations, transformation (the ICP's 4x4), sim3 (the trajectory alignment's 4x4)}.

    1. stamps are associated (eval_ate.associate, max_diff); fewer than 3 pairs: ValueError.  2. M = the Sim(3) of the run's camera
    positions onto the GT's over the pairs (trajectory_sim3).  3. GT cloud: the matched GT frames in ascending GT index, depths in
    (0, depth_trunc).  4. the run's cloud: the matched keyframes under M . c2w (composed in fp64), depths in (0, est_depth_trunc) in the
    run's own units, before the Sim(3) (default depth_trunc, as the reference's depth2point).  5. ICP (point to point, icp_threshold,
    from the identity) of the two clouds voxel-downsampled at `voxel`.  6. the run's cloud emitted again under T_icp . M . c2w: one rounding per point.  7. the clipped
    RMSE Chamfer distances of geometry_eval_utils.chamfer_distance_RMSE(gt, est, max_error).  size=(H1, W1): both sets are sampled on
    that nearest-neighbour grid first (the reference's vggt_resize, 392 x 518), the intrinsics scaled with it."""
    e_depth, e_pose, e_K, e_stamp, e_rgb = _views(est, "est")
    g_depth, g_pose, g_K, g_stamp, g_rgb = _views(gt, "gt")
    ie, ig = associate(e_stamp[:, None], g_stamp[:, None], max_diff)
    if len(ie) < 3:
        raise ValueError(f"only {len(ie)} associated frames (max_diff {max_diff})")
    s, R, t = trajectory_sim3(e_pose[ie, :3, 3], g_pose[ig, :3, 3])
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = s * R, t
    ig_sorted = np.sort(ig)
    e_trunc = depth_trunc if est_depth_trunc is None else est_depth_trunc
    gK = grid_intrinsics(g_K, len(g_pose), g_depth.shape[1:], size)[ig_sorted]
    eK = grid_intrinsics(e_K, len(e_pose), e_depth.shape[1:], size)[ie]
    gt_pts, gt_col, _ = _cloud(g_depth, g_rgb, ig_sorted, g_pose[ig_sorted], gK, depth_trunc, size)
    emit = lambda T: _cloud(e_depth, e_rgb, ie, T @ e_pose[ie], eK, e_trunc, size)
    est_pts, est_col, _ = emit(M)
    if gt_pts.shape[0] == 0 or est_pts.shape[0] == 0:
        raise ValueError(f"empty cloud: {gt_pts.shape[0]} GT points, {est_pts.shape[0]} estimated points")
    T_icp, fitness, rmse, iters = np.eye(4), float("nan"), float("nan"), 0
    if icp:
        reg = icp_point_to_point(ops.voxel_downsample(est_pts, voxel)[0], ops.voxel_downsample(gt_pts, voxel)[0], icp_threshold)
        T_icp, fitness, rmse, iters = reg.transformation, reg.fitness, reg.inlier_rmse, reg.iterations
        del est_pts, est_col
        est_pts, est_col, _ = emit(T_icp @ M)
    cd, r_acc, r_comp, _, _ = chamfer_distance_RMSE(gt_pts, est_pts, max_error)
    out = {"RMSE_acc": r_acc, "RMSE_comp": r_comp, "Chamfer_distance": cd, "n_gt": int(gt_pts.shape[0]), "n_est": int(est_pts.shape[0]),
           "pairs": int(len(ie)), "scale": float(s), "icp_fitness": float(fitness), "icp_rmse": float(rmse), "icp_iterations": int(iters),
           "transformation": T_icp, "sim3": M}
    if return_clouds:
        out["clouds"] = {"est": (est_pts, est_col), "gt": (gt_pts, gt_col)}
    return out


# ------------------------------------------------------------------------------------------------------------------------ sources
def filter_views(views, consistency, return_keep=False):
    """the DepthViews with its depth maps cross-checked between neighbouring views (depth_consistency.ConsistencyOptions) and the rejected
    pixels zeroed, which the clouds skip; every finite positive depth takes part, whatever the evaluation truncates later.  This is for
    the RUN's depths: ground truth is never filtered."""
    from . import depth_consistency
    depth, poses, K, _, _ = _views(views, "views")
    out, keep = depth_consistency.apply(depth.to(_device(), torch.float32), inverse44(poses)[:, :3], intrinsics(K, len(poses)), consistency,
                                        float("inf"))
    v = DepthViews(*views)._replace(depth=out)
    return (v, keep) if return_keep else v


def _filtered(views, consistency) -> DepthViews:
    return views if consistency is None else filter_views(views, consistency)


def from_keyframes(keyframes, n, stamps=None, consistency=None) -> DepthViews:
    """the tracker's keyframes 0..n-1 (the same ones as the trajectory): depth, pose (c2w [t, q xyzw]), intrinsic, tstamp, image.  stamps:
    replaces the store's frame indices (demo.py passes the file stamps that traj_kf.txt carries).  consistency: filter_views' options
    (None: the depth maps as they are)."""
    n = int(n)
    if n <= 0:
        raise ValueError("no tracked keyframes")
    kf = keyframes
    stamps = kf.tstamp[:n].double().numpy() if stamps is None else np.asarray(stamps, np.float64).reshape(-1)[:n]
    return _filtered(DepthViews(kf.depth[:n], kf.pose[:n].double().numpy(), kf.intrinsic[:n].double().numpy(), stamps, kf.image[:n]), consistency)


def _mapper_frame_indices(mapper):
    """the frame index (Camera.tstamp) of every mapper keyframe in key order.  A view added without one (add_new_view's default) is
    refused: its key is a keyframe index, and taken for a stamp it would pair the view with the wrong GT frame."""
    vp = mapper.viewpoints
    missing = [k for k in sorted(vp) if vp[k].tstamp is None]
    if missing:
        raise ValueError(f"mapper keyframes {missing[:5]} carry no tstamp: pass stamps explicitly")
    return [vp[k].tstamp for k in sorted(vp)]


@torch.no_grad()
def from_mapper(mapper, stamps=None, consistency=None) -> DepthViews:
    """every mapper keyframe rendered from the Gaussian map at its refined pose (tsdf.render_mapper_views: the depth quantised as the
    reference's renders_kf/depth_after_opt PNGs).  stamps: one per keyframe in key order; default the keyframes' frame indices.
    consistency: filter_views' options (None: the depth maps as they are)."""
    from .tsdf import render_mapper_views
    if not mapper.viewpoints:
        raise ValueError("the mapper has no keyframes")
    if stamps is None:
        stamps = _mapper_frame_indices(mapper)
    depth, rgb, w2c, K = render_mapper_views(mapper)
    return _filtered(DepthViews(depth, inverse44(pose_matrices(w2c)), K.double().cpu().numpy(), np.asarray(stamps, np.float64), rgb), consistency)


def cast_views(volume, views, **cast):
    """tsdf.RayCast of a fused volume (tsdf.TSDFVolume / SparseTSDFVolume) at the poses and intrinsics of `views` and the size of its
    depth maps: world->camera = the fp64 inverse of each c2w.  cast: the options of the volume's ray_cast."""
    depth, poses, K, _, _ = _views(views, "views")
    n, (H, W) = depth.shape[0], depth.shape[1:]
    w2c = inverse44(poses)[:, :3].reshape(n, 12).astype(np.float32)
    return volume.ray_cast(torch.from_numpy(w2c), torch.from_numpy(intrinsics(K, n).astype(np.float32)), H, W, **cast)


def from_volume(volume, views, **cast) -> DepthViews:
    """the fused model's own depth maps: `volume` ray-cast (csrc/tsdf_raycast.hip) at every pose of `views`, with their intrinsics, size
    and stamps; 0 where a ray misses, which the clouds skip.  The colours are the volume's."""
    rc = cast_views(volume, views, normals=False, **cast)
    v = DepthViews(*views)
    return DepthViews(rc.depth, v.c2w, v.K, v.stamps, rc.color)


def from_slam(slam, source="auto", stamps_full=None, consistency=None, volume=None, fuse=None) -> DepthViews:
    """the keyframes views.run_views picks for `source` ("mapper", "tracker", "auto"), as Cut3rSlam.fuse / --mesh-source do.
    "fused": the run's TSDF volume ray-cast at each keyframe's pose and intrinsics (from_volume) -- `volume` when given, else
    slam.fuse(**fuse), fuse = its arguments (voxel_size at least); the keyframes are those of fuse's source (default auto).
    stamps_full: the per-frame stamps (stream.frame_timestamps) that map the store's frame indices to the stamps of traj_kf.txt.
    consistency: filter_views' options (None: the depth maps as they are)."""
    if source == "fused":
        fuse = dict(fuse or {})
        if volume is None:
            if "voxel_size" not in fuse:
                raise ValueError("source='fused' needs a volume, or fuse={'voxel_size': ...} to make one")
            volume = slam.fuse(**fuse)
        return _filtered(from_volume(volume, from_slam(slam, fuse.get("source", "auto"), stamps_full)), consistency)
    kind, n = run_views(slam, source)
    full = None if stamps_full is None else np.asarray(stamps_full, np.float64).reshape(-1)
    lookup = (lambda idx: None) if full is None else (lambda idx: full[np.asarray(idx, np.float64).astype(int)])
    if kind == "mapper":
        return from_mapper(slam.mapper, lookup(_mapper_frame_indices(slam.mapper)), consistency)
    return from_keyframes(slam.keyframes, n, lookup(slam.keyframes.tstamp[:max(n, 0)].numpy()), consistency)


def read_depth_png(path, scale) -> np.ndarray:
    """fp32 [H,W] metres of a 16-bit depth PNG: raw 65535 (7-Scenes' invalid marker, eval7_scenes_dense.py:73) -> 0, float32(raw) /
    float32(scale)"""
    from PIL import Image
    with Image.open(path) as im:
        raw = np.asarray(im)
    if raw.ndim != 2:
        raise ValueError(f"{path}: a single-channel 16-bit depth image is expected, got shape {raw.shape}")
    raw = raw.astype(np.int64)
    if raw.min() < 0 or raw.max() > 65535:
        raise ValueError(f"{path}: values outside 0..65535")
    raw[raw == 65535] = 0
    return raw.astype(np.float32) / np.float32(scale)


def load_depth_dir(depthdir, scale, traj_tum, calib) -> DepthViews:
    """a directory of 16-bit depth PNGs (natural sort; the stamp of a file is the last number in its name, the rule of
    stream.frame_timestamps) with a TUM trajectory (a path or [m,8] rows) and a calibration (a path or fx fy cx cy ...).  A file is used
    when the trajectory has a pose at its stamp (within 1e-6), so a directory of all frames goes with a keyframe trajectory."""
    names = [f for f in natsorted(os.listdir(depthdir)) if f.lower().endswith(".png")]
    if not names:
        raise ValueError(f"{depthdir}: no PNG files")
    stamps = np.array([float(re.findall(r"[+]?(?:\d*\.\d+|\d+)", x)[-1]) for x in names])
    traj = load_tum(traj_tum) if isinstance(traj_tum, (str, os.PathLike)) else np.asarray(traj_tum, np.float64).reshape(-1, 8)
    K = np.asarray(load_calib(calib) if isinstance(calib, (str, os.PathLike)) else calib, np.float64).reshape(-1)[:4]
    i_file, i_pose = associate(stamps[:, None], traj, 1e-6)
    if len(i_file) == 0:
        raise ValueError(f"{depthdir}: no file stamp has a pose in the trajectory")
    depth = np.stack([read_depth_png(os.path.join(depthdir, names[i]), scale) for i in i_file])
    return DepthViews(torch.from_numpy(depth), traj[i_pose], K, stamps[i_file], None)


# ------------------------------------------------------------------------------------------------------------------------- output
def write_results(outdir, result, clouds=None) -> str:
    """<outdir>/3D_eval_results.txt: the three metrics as `key: value` lines (eval7_scenes_dense.py:282-289); clouds = {"est": (points,
    colors), "gt": (points, colors)}: also pcd_est_aligned.ply and pcd_gt.ply (:265-266), vertex-only"""
    os.makedirs(outdir, exist_ok=True)
    path = os.path.join(outdir, "3D_eval_results.txt")
    with open(path, "w") as fh:
        for k in KEYS:
            fh.write(f"{k}: {result[k]}\n")
    if clouds is not None:
        from .tsdf import Mesh, write_ply
        for name, key in (("pcd_est_aligned.ply", "est"), ("pcd_gt.ply", "gt")):
            pts, col = clouds[key]
            write_ply(os.path.join(outdir, name), Mesh(pts.cpu().numpy(), None if col is None else col.cpu().numpy(), np.zeros((0, 3), np.int32)))
    return path


def read_results(path) -> dict:
    out = {}
    with open(path) as fh:
        for line in fh:
            k, _, v = line.partition(":")
            if v.strip():
                out[k.strip()] = float(v)
    return out


# ---------------------------------------------------------------------------------------------------------------------------- CLI
def parse_args(argv=None):
    p = argparse.ArgumentParser(description="dense point-cloud evaluation of depth maps against GT depth maps (scripts/eval7_scenes_dense.py)")
    p.add_argument("--est-depthdir", required=True, help="the run's 16-bit depth PNGs, one per pose of --est-traj (stamp = last number in the name)")
    p.add_argument("--est-traj", required=True, help="the run's TUM trajectory (traj_kf.txt)")
    p.add_argument("--est-calib", required=True, help="fx fy cx cy of the run's depth maps")
    p.add_argument("--gtdepthdir", required=True, help="ground-truth 16-bit depth PNGs")
    p.add_argument("--gt-traj", required=True, help="ground-truth TUM trajectory")
    p.add_argument("--gt-calib", required=True, help="fx fy cx cy of the GT depth maps")
    p.add_argument("--gt-depth-scale", type=float, default=1000.0, help="GT raw units per metre (7-Scenes, ScanNet: 1000; TUM: 5000)")
    p.add_argument("--est-depth-scale", type=float, default=DEPTH_SCALE, help="the run's raw units per metre")
    p.add_argument("--depth-trunc", type=float, default=4.5, help="depths at or beyond this are dropped (Kinect range, :72-76)")
    p.add_argument("--est-depth-trunc", type=float, default=None, help="the same for the run, in its own units (default --depth-trunc)")
    p.add_argument("--resize", type=int, nargs=2, default=None, metavar=("H", "W"), help="nearest-neighbour sampling grid (the reference: 392 518)")
    p.add_argument("--voxel", type=float, default=0.05)
    p.add_argument("--icp-threshold", type=float, default=0.1)
    p.add_argument("--max-error", type=float, default=0.5)
    p.add_argument("--max-diff", type=float, default=0.01, help="largest stamp difference of an associated pair")
    p.add_argument("--no-icp", action="store_true")
    p.add_argument("--save", type=str, default=None, help="directory for 3D_eval_results.txt, pcd_est_aligned.ply and pcd_gt.ply")
    a = p.parse_args(argv)
    for name in ("gt_depth_scale", "est_depth_scale", "depth_trunc", "voxel", "icp_threshold", "max_error"):
        if not getattr(a, name) > 0:
            p.error(f"--{name.replace('_', '-')} must be > 0")
    if a.est_depth_trunc is not None and not a.est_depth_trunc > 0:
        p.error("--est-depth-trunc must be > 0")
    if a.max_diff < 0:
        p.error("--max-diff must be >= 0")
    if a.resize is not None and min(a.resize) <= 0:
        p.error("--resize H W must be > 0")
    return a


def main(argv=None):
    a = parse_args(argv)
    est = load_depth_dir(a.est_depthdir, a.est_depth_scale, a.est_traj, a.est_calib)
    gt = load_depth_dir(a.gtdepthdir, a.gt_depth_scale, a.gt_traj, a.gt_calib)
    res = dense_metrics(est, gt, depth_trunc=a.depth_trunc, est_depth_trunc=a.est_depth_trunc, size=None if a.resize is None else tuple(a.resize),
                        voxel=a.voxel, icp_threshold=a.icp_threshold, max_error=a.max_error, max_diff=a.max_diff, icp=not a.no_icp,
                        return_clouds=a.save is not None)
    clouds = res.pop("clouds", None)
    print({k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in res.items()})
    if a.save:
        write_results(a.save, res, clouds)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
