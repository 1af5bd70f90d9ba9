"""Camera poses, intrinsics and the run's view source for the host code in front of the kernels (ops, tsdf, depth_consistency, eval_dense,
mesh_render, Cut3rSlam, demo.py): numpy and torch, no GPU call.  The three inverses round differently and are kept apart, each with the
arithmetic its consumers are pinned to: inverse44 (eval_dense, mesh_render, demo.py), inverse_affine (tsdf: the c2w rows of the ray cast and
of the sparse volume's mark kernel), inverse_rigid (depth_consistency.relative_rows)."""
from __future__ import annotations

import numpy as np
import torch


def _cast(x, dtype):
    """x as a tensor on its device (a torch dtype) or an array (a numpy dtype), converted in one step"""
    if isinstance(dtype, torch.dtype):
        return torch.as_tensor(x).detach().to(dtype)
    return np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype)


def pose_rows(p, dtype=np.float64, single=False):
    """[n,3,4] of poses [n,12], [n,16], [n,3,4] or [n,4,4] (a fourth row is dropped unread): a tensor for a torch dtype, an array for a
    numpy one.  single: a lone [3,4] or [4,4] is one pose; without it that is n rows of width 4 and refused like every other shape."""
    p = _cast(p, dtype)
    s = tuple(p.shape)
    if single and s in ((3, 4), (4, 4)):
        p, s = p[None], (1,) + s
    if (len(s) == 2 and s[1] in (12, 16)) or (len(s) == 3 and s[1:] in ((3, 4), (4, 4))):
        return p.reshape(s[0], s[-1] // 4 if len(s) == 2 else s[1], 4)[:, :3]
    raise ValueError(f"poses: [n,12], [n,16], [n,3,4] or [n,4,4], got {list(s)}")


def intrinsics(K, n, dtype=np.float64):
    """[n,4] fx fy cx cy of K [4], [1,4] or [n,4], a contiguous copy: a tensor for a torch dtype, an array for a numpy one"""
    K = _cast(K, dtype)
    if tuple(K.shape) not in ((4,), (1, 4), (n, 4)):
        raise ValueError(f"intrinsics: [4], [1,4] or [{n},4] fx fy cx cy, got {list(K.shape)}")
    K = K.reshape(-1, 4)
    return K.expand(n, 4).contiguous() if isinstance(K, torch.Tensor) else np.array(np.broadcast_to(K, (n, 4)))


def tum_matrices(rows) -> np.ndarray:
    """fp64 [n,4,4] from TUM rows [n,8] (stamp first) or [n,7]: t, q = (x, y, z, w), normalised here"""
    p = _cast(rows, np.float64)
    if p.ndim != 2 or p.shape[1] not in (7, 8):
        raise ValueError(f"TUM rows: [n,8] or [n,7], got {list(p.shape)}")
    p = p[:, -7:]
    t, q = p[:, :3], p[:, 3:]
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    out = np.tile(np.eye(4), (len(p), 1, 1))
    out[:, :3, :3], out[:, :3, 3] = R, t
    return out


def pose_matrices(p) -> np.ndarray:
    """fp64 [n,4,4] (last row 0 0 0 1) from any layout of pose_rows or from TUM rows ([n,8] with the stamp first, [n,7] without)"""
    p = _cast(p, np.float64)
    if p.ndim == 2 and p.shape[1] in (7, 8):
        return tum_matrices(p)
    rows = pose_rows(p)
    out = np.tile(np.eye(4), (len(rows), 1, 1))
    out[:, :3] = rows
    return out


def inverse44(T) -> np.ndarray:
    """fp64 [n,4,4]: np.linalg.inv of 4x4 matrices [n,4,4] (or one [4,4])"""
    return np.linalg.inv(np.asarray(T, np.float64).reshape(-1, 4, 4))


def inverse_affine(rows) -> np.ndarray:
    """fp32 [n,12]: the inverse of each 3x4 affine map of rows [n,12], in fp64 and rounded once (a rigid map gives R^T, -R^T t)"""
    w = np.asarray(rows, np.float64).reshape(-1, 3, 4)
    Ri = np.linalg.inv(w[:, :, :3])
    ti = -(Ri @ w[:, :, 3:])
    return np.ascontiguousarray(np.concatenate([Ri, ti], 2).reshape(-1, 12), dtype=np.float32)


def inverse_rigid(rows):
    """(R^T [n,3,3], -R^T t [n,3]) of rigid rows [R | t] fp64 [n,3,4]: no matrix is inverted"""
    Ri = rows[:, :, :3].transpose(0, 2, 1)
    return Ri, -np.einsum("nij,nj->ni", Ri, rows[:, :, 3])


def run_views(slam, source="auto"):
    """which keyframes are the run -> ("mapper", its keyframe count) or ("tracker", n): "auto" is the mapper when one with keyframes is
    attached; the tracker's are 0 .. counter - 2, capped by tracker.t1 when only the tracked ones count (n <= 0: the consumers refuse)"""
    if source not in ("auto", "tracker", "mapper"):
        raise ValueError(f"source must be auto, tracker or mapper, not {source!r}")
    has_mapper = slam.mapper is not None and bool(getattr(slam.mapper, "viewpoints", None))
    if source == "mapper" or (source == "auto" and has_mapper):
        if not has_mapper:
            raise ValueError("source='mapper' needs a Gaussian mapper with keyframes")
        return "mapper", len(slam.mapper.viewpoints)
    n = slam.keyframes.counter.value - 1
    if slam.tracked_only:
        n = min(n, slam.tracker.t1)
    return "tracker", n
