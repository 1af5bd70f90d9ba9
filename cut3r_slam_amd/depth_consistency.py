"""Multi-view depth consistency filtering ahead of TSDF fusion and the dense clouds, on the gfx950 kernel of csrc/consistency.hip.

Pointmap networks leave flying pixels at depth discontinuities and now and then a floating blob; fused as they are, only the TSDF weight
threshold removes them, and only when no second view repeats them.  Here every keyframe depth map is cross-checked against its neighbours
first, as MVSNet's fusion, Gipuma and COLMAP do.  The reference has no such step: nothing here reproduces a file of it.

The rule per reference pixel and source view (include/cut3r_hip.h states the arithmetic and its order, tests/consistency_oracle.py restates
it; depths are valid when finite and in (0, depth_max]):

  no observation   the point projects behind the source (Z <= z_min), outside its image, or onto a 2x2 neighbourhood with an invalid depth
  violation        the point is nearer to the source than ALL FOUR depths around its projection by more than `rel`: the source sees through
                   the place where the reference put a surface (free space).  All four must agree because the source's own map may have
                   a discontinuity there, and a depth interpolated across one means nothing
  support          the source's interpolated depth, carried back into the reference, lands within `pix` pixels of the pixel and within
                   `rel` (relative) of its depth.  A violating source never supports; a point hidden behind the source's surface is neither

  neighbour_table  the sources of view i: i - window .. i + window
  relative_rows    the rigid rows reference -> source and back, composed on the host in fp64
  consistency      (support, violation[, depth_avg]) of every view of a stack
  filter_depths    the stack with the rejected pixels set to 0 (every consumer skips 0), and the mask
  ConsistencyOptions / apply   what tsdf.fuse_*, Cut3rSlam.fuse / reconstruct and eval_dense.from_* take as `consistency=`

pix = 1, rel = 0.01, min_support = 2 and window = 2 are user parameters.  The defaults are the ones of MVSNet's fusion (one pixel, one per
cent, photo-consistent in several views); they are NOT tuned on real data here.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import ops, views


class ConsistencyOptions(NamedTuple):
    window: int = 2                # sources of view i: i - window .. i + window
    min_support: int = 2           # a pixel stays when at least this many sources support it ...
    max_violation: int = 0         # ... and at most this many see through it
    pix: float = 1.0               # reprojection distance of a supporting source, pixels
    rel: float = 0.01              # relative depth difference of a supporting source, and the margin of the free-space test
    average: bool = False          # kept pixels take the mean of their own and the supporting depths


def neighbour_table(n, window) -> np.ndarray:
    """int32 [n, 2 window]: row i holds i - window .. i + window without i, clipped to [0, n), ascending, padded with -1"""
    n, window = int(n), int(window)
    if n < 1 or window < 1:
        raise ValueError("neighbour_table: n >= 1 and window >= 1")
    out = np.full((n, 2 * window), -1, np.int32)
    for i in range(n):
        s = [j for j in range(i - window, i + window + 1) if j != i and 0 <= j < n]
        out[i, :len(s)] = s
    return out


def _tables(n, ref, src):
    ref = np.asarray(ref)
    src = np.asarray(src)
    if ref.ndim != 1 or src.ndim != 2 or src.shape[0] != ref.shape[0] or ref.dtype.kind not in "iu" or src.dtype.kind not in "iu":
        raise ValueError("ref: integers [R], src: integers [R,S]")
    if src.shape[1] < 1 or src.shape[1] > ops.CONSISTENCY_MAX_SOURCES:
        raise ValueError(f"src: 1 .. {ops.CONSISTENCY_MAX_SOURCES} sources a view, got {src.shape[1]}")
    if ((ref < 0) | (ref >= n)).any() or ((src < -1) | (src >= n)).any():
        raise ValueError(f"ref / src: index outside the {n} views (-1: no source)")
    if (src == ref[:, None]).any():
        raise ValueError("src: a view cannot be its own source")
    return ref.astype(np.int32), src.astype(np.int32)


def relative_rows(w2c, ref, src):
    """(fwd, bwd) fp64 [R,S,12]: fwd[r,k] = W_s . W_r^-1 carries camera coordinates of view ref[r] into view src[r,k], bwd the other way;
    the inverse of a rigid [R | t] is formed as [R^T | -R^T t].  Rows of a missing source (-1) are 0.  Refused: src == ref, an index
    outside the views, more than 16 sources."""
    W = np.ascontiguousarray(views.pose_rows(w2c))
    ref, src = _tables(len(W), ref, src)
    Rm, t = W[:, :, :3], W[:, :, 3]
    Ri, ti = views.inverse_rigid(W)

    def compose(a, b):             # W_a . W_b^-1 for index arrays a, b of one shape
        Rab = np.einsum("...ij,...jk->...ik", Rm[a], Ri[b])
        tab = np.einsum("...ij,...j->...i", Rm[a], ti[b]) + t[a]
        return np.concatenate([Rab, tab[..., None]], -1).reshape(a.shape + (12,))
    s = np.where(src >= 0, src, 0)
    r = np.broadcast_to(ref[:, None], src.shape)
    used = (src >= 0)[..., None]
    return np.where(used, compose(s, r), 0.0), np.where(used, compose(r, s), 0.0)


def consistency(depth, w2c, K, src=None, window=2, depth_max=5.0, pix=1.0, rel=0.01, z_min=1e-3, average=False,
                chunk=ops.CONSISTENCY_MAX_REFS):
    """(support u8 [N,H,W], violation u8 [N,H,W][, depth_avg fp32 [N,H,W]]) of all N views of depth fp32 [N,H,W] (GPU): how many of its
    sources support each pixel and how many see through it.  w2c [N,12] / [N,3,4] / [N,4,4] rigid world->camera (used in fp64), K [4] or
    [N,4] fx fy cx cy.  src: int [N,S] table of source views (-1: none, S <= 16), default neighbour_table(N, window).  pix, rel, window
    are user parameters whose defaults (MVSNet's) are not tuned on real data.  The views go through the kernel `chunk` at a time."""
    depth = torch.as_tensor(depth)
    if depth.dim() != 3 or depth.shape[0] == 0:
        raise ValueError("depth: [N,H,W]")
    depth = depth.to(torch.float32).contiguous()
    N = depth.shape[0]
    if src is None:
        if 2 * int(window) > ops.CONSISTENCY_MAX_SOURCES:
            raise ValueError(f"window {window}: more than {ops.CONSISTENCY_MAX_SOURCES} sources a view")
        src = neighbour_table(N, window)
    ref = np.arange(N, dtype=np.int32)
    fwd, bwd = relative_rows(w2c, ref, src)
    src = np.asarray(src, np.int32)
    K = views.intrinsics(K, N, torch.float32).to(depth.device)
    chunk = int(chunk)
    if not 1 <= chunk <= ops.CONSISTENCY_MAX_REFS:
        raise ValueError(f"chunk: 1 .. {ops.CONSISTENCY_MAX_REFS}")
    parts = [ops.depth_consistency(depth, K, ref[a:a + chunk], src[a:a + chunk], fwd[a:a + chunk], bwd[a:a + chunk], depth_max, pix=pix,
                                   rel=rel, z_min=z_min, average=average) for a in range(0, N, chunk)]
    out = tuple(p[0] if len(parts) == 1 else torch.cat(p) for p in zip(*parts) if p[0] is not None)
    return out


def filter_depths(depth, w2c, K, min_support=2, max_violation=0, **kw):
    """(depth_filtered fp32 [N,H,W], keep bool [N,H,W]): keep = the depth is valid (finite, in (0, depth_max]), at least min_support
    sources support it and at most max_violation see through it; every other pixel becomes 0, which every consumer skips.  With
    average=True the kept pixels take depth_avg, the mean of their own depth and the supporting sources' depths carried into the view.
    **kw: consistency()'s.  min_support (like pix, rel, window) is a user parameter; its default is not tuned on real data."""
    depth = torch.as_tensor(depth).to(torch.float32)
    out = consistency(depth, w2c, K, **kw)
    support, violation = out[0], out[1]
    depth_max = float(kw.get("depth_max", 5.0))
    top = np.float32(depth_max)                                        # the largest fp32 <= depth_max: the kernel compares in fp64
    if float(top) > depth_max:
        top = np.nextafter(top, np.float32(-np.inf))
    keep = torch.isfinite(depth) & (depth > 0) & (depth <= float(top)) & (support >= int(min_support)) & (violation <= int(max_violation))
    value = out[2] if kw.get("average", False) else depth
    return torch.where(keep, value, torch.zeros_like(value)), keep


def apply(depth, w2c, K, options, depth_max):
    """filter_depths under a ConsistencyOptions (or a tuple / dict of its fields)"""
    o = ConsistencyOptions(**options) if isinstance(options, dict) else ConsistencyOptions(*options)
    return filter_depths(depth, w2c, K, min_support=o.min_support, max_violation=o.max_violation, window=o.window, pix=o.pix, rel=o.rel,
                         average=o.average, depth_max=depth_max)
