"""Writes tests/golden/focal.npz: seeded pointmaps and what the reference's own `estimate_focal_knowing_depth`
(src/dust3r/post_process.py:12-64, pure torch, on the CPU) returns for them.

Run only where the reference tree is present (CUT3R_REFERENCE, default /root/reference); the tests read the .npz alone.  Per case `name`:
    {name}_pts fp32 [B,H,W,3], {name}_pp fp32 [B,2],
    {name}_median, {name}_weiszfeld fp32 [B]   the reference on the fp32 inputs (its default clip to [0, inf) included)
    {name}_weiszfeld64 fp64 [B]                the same function on .double() inputs
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("CUT3R_REFERENCE", "/root/reference")


def pinhole(rng, B, H, W, f, pp, noise):
    """points of a pinhole camera with focal f and principal points pp [B,2] at random depths, plus relative noise"""
    col = np.arange(W, dtype=np.float64)[None, None, :]
    row = np.arange(H, dtype=np.float64)[None, :, None]
    z = rng.uniform(1.0, 4.0, size=(B, H, W))
    x = (col - pp[:, 0, None, None]) * z / f
    y = (row - pp[:, 1, None, None]) * z / f
    pts = np.stack([x, y, z], -1)
    pts = pts + noise * z[..., None] * rng.standard_normal(pts.shape)
    return pts.astype(np.float32)


def cases():
    rng = np.random.default_rng(20240607)
    out = {}
    # noisy pinhole with an outlier patch, one z = 0 and one x = 0 pixel
    B, H, W = 3, 24, 32
    pp = np.tile(np.float32([W / 2, H / 2]), (B, 1))
    pts = pinhole(rng, B, H, W, 29.0, pp.astype(np.float64), 0.01)
    pts[:, 3:9, 20:28] = rng.standard_normal((B, 6, 8, 3)).astype(np.float32) * 3
    pts[0, 10, 5, 2] = 0.0
    pts[1, 15, 7, 0] = 0.0
    out["patch"] = (pts, pp)
    # per-view principal points, off-centre and non-integer; ragged sizes
    B, H, W = 2, 37, 53
    pp = np.float32([[24.3, 20.71], [30.125, 15.6]])
    out["offcentre"] = (pinhole(rng, B, H, W, 61.5, pp.astype(np.float64), 0.005), pp)
    # exact pinhole, f = 32, z = 1: every reprojection distance is 0 (the 1e-8 clip of the weights)
    H, W = 24, 32
    pp = np.float32([[W / 2, H / 2]])
    col, row = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32), indexing="xy")
    pts = np.stack([(col - pp[0, 0]) / np.float32(32), (row - pp[0, 1]) / np.float32(32), np.ones_like(col)], -1)[None].astype(np.float32)
    out["exact"] = (pts, pp)
    # several pixels per thread
    H, W = 101, 131
    pp = np.float32([[W / 2, H / 2]])
    out["large"] = (pinhole(rng, 1, H, W, 150.0, pp.astype(np.float64), 0.01), pp)
    # no geometry at all: the policy's rejection case
    B, H, W = 2, 24, 32
    pp = np.tile(np.float32([W / 2, H / 2]), (B, 1))
    out["noise"] = (np.random.default_rng(4).standard_normal((B, H, W, 3)).astype(np.float32), pp)      # (both raw estimates negative: clipped to 0)
    return out


def main():
    sys.path[:0] = [os.path.join(REF, "src")]
    from dust3r.post_process import estimate_focal_knowing_depth
    arrays = {}
    for name, (pts, pp) in cases().items():
        tp, tpp = torch.from_numpy(pts), torch.from_numpy(pp)
        arrays[f"{name}_pts"], arrays[f"{name}_pp"] = pts, pp
        arrays[f"{name}_median"] = estimate_focal_knowing_depth(tp, tpp, focal_mode="median").numpy().astype(np.float32)
        arrays[f"{name}_weiszfeld"] = estimate_focal_knowing_depth(tp, tpp, focal_mode="weiszfeld").numpy().astype(np.float32)
        arrays[f"{name}_weiszfeld64"] = estimate_focal_knowing_depth(tp.double(), tpp.double(), focal_mode="weiszfeld").numpy().astype(np.float64)
        print(name, pts.shape, arrays[f"{name}_median"], arrays[f"{name}_weiszfeld"], arrays[f"{name}_weiszfeld64"])
    path = os.path.join(HERE, "focal.npz")
    np.savez(path, **arrays)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
