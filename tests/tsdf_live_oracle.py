"""numpy restatement of csrc/tsdf_live.hip: the integer accumulators of the live TSDF volume and the planes resolved from them, bit for bit.

Built per view on the dense oracle (tests/tsdf_oracle.py), which restates the gates the live kernel shares with tsdf_fuse_voxel: ONE view
fused into a FRESH volume leaves tsdf == t exactly on the voxels it updates ((1 * 0 + t) / 1 is exact), weight == 1 there and nowhere
else, and color == the pixel's u8 values.  So q = rint(t * 32768) per view, and the accumulators are plain integer sums."""
from __future__ import annotations

import numpy as np

from tests import tsdf_oracle as O
from tests import tsdf_sparse_oracle as S

f32 = np.float32
Q = 32768


def new_acc(dims):
    X, Y, Z = dims
    return np.zeros((5, Z, Y, X), np.int32)


def integrate(acc, origin, voxel, depth, w2c, K, trunc, depth_max, rgb=None, conf=None, conf_ds=1, conf_min=None, sign=1, offset=(0, 0, 0)):
    """in place on acc int32 [5,Z,Y,X] (sum_q, count, sum_r, sum_g, sum_b): the views of depth [B,H,W] put in (sign = 1) or taken out
    (sign = -1).  offset: acc is the window of the lattice (origin, voxel) that starts at this integer voxel position."""
    depth = np.asarray(depth, f32)
    B = depth.shape[0]
    w2c = np.asarray(w2c, f32).reshape(B, 12)
    K = np.broadcast_to(np.asarray(K, f32).reshape(-1, 4), (B, 4))
    Z, Y, X = acc.shape[1:]
    for b in range(B):
        one = O.new_volume((X, Y, Z))
        S.integrate_window(one, origin, voxel, offset, depth[b:b + 1], w2c[b:b + 1], K[b:b + 1], trunc, depth_max,
                           rgb=None if rgb is None else rgb[b:b + 1], conf=None if conf is None else conf[b:b + 1], conf_ds=conf_ds,
                           conf_min=conf_min)
        m = one[1] == 1
        assert np.all(one[1][~m] == 0)
        q = np.rint(one[0][m] * f32(Q))
        assert np.all(np.abs(q) <= Q)
        acc[0][m] += sign * q.astype(np.int32)
        acc[1][m] += sign
        if rgb is not None:
            for c in range(3):
                acc[2 + c][m] += sign * one[2][c][m].astype(np.int32)
    return acc


def resolve(acc):
    """(tsdf, weight, color [3]) fp32 of the accumulators: one fp64 division and one rounding to fp32 each; count == 0 -> (1, 0, 0)"""
    n = acc[1].astype(np.float64)
    some = acc[1] != 0
    d = np.where(some, n, 1.0)
    tsdf = np.where(some, (acc[0].astype(np.float64) / (d * float(Q))).astype(f32), f32(1))
    color = np.where(some[None], (acc[2:].astype(np.float64) / d[None]).astype(f32), f32(0))
    return tsdf, acc[1].astype(f32), color
