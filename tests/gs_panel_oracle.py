"""The arithmetic of the diagnostic panels and frames (csrc/gs_panel.hip; include/cut3r_hip.h states it), once, in plain numpy: the kernels
must equal this in every byte.  fp32 operations are numpy float32 operations (one rounding each, no fused multiply-add), the two fp64
steps (the turbo denominator and the colour quantiser) are float64.  The turbo table is the kernels' own copy, csrc/turbo_u8.h."""
import os
import re

import numpy as np

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def turbo_table():
    """uint8 [256,3]: the numbers of csrc/turbo_u8.h in order (comment lines dropped)"""
    with open(os.path.join(ROOT, "cut3r_slam_amd", "csrc", "turbo_u8.h"), encoding="ascii") as fh:
        body = "".join(ln for ln in fh if not ln.lstrip().startswith("//"))
    t = np.array([int(v) for v in re.findall(r"\d+", body)])
    assert t.size == 768 and t.max() <= 255
    return t.astype(np.uint8).reshape(256, 3)


TURBO_U8 = turbo_table()


def turbo_cell(x, lo=None, hi=None):
    """x fp32 [H,W] -> uint8 [H,W,3]; lo, hi default to the map's own fp32 min and max"""
    x = np.asarray(x, f32)
    lo = f32(x.min()) if lo is None else f32(lo)
    hi = f32(x.max()) if hi is None else f32(hi)
    den = f32(np.float64(hi) - np.float64(lo) + 1e-10)
    q = np.clip((x - lo) / den, f32(0), f32(1)).astype(f32)
    idx = (q * f32(255)).astype(f32).astype(np.int64)                    # truncation of a value in [0, 255]
    return TURBO_U8[idx]


def color_cell(v):
    """v fp32 [3,H,W] -> uint8 [H,W,3]: floor(clamp(double(v), 0, 1) * 255 + 0.5)"""
    c = np.clip(np.asarray(v, f32).astype(np.float64), 0.0, 1.0)
    return np.floor(c * 255.0 + 0.5).astype(np.uint8).transpose(1, 2, 0)


def exposure(render, A, b):
    """e_c = ((r0 A[0,c] + r1 A[1,c]) + r2 A[2,c]) + b_c, every product and sum rounded to fp32"""
    r, A, b = np.asarray(render, f32), np.asarray(A, f32), np.asarray(b, f32)
    return np.stack([((r[0] * A[0, c] + r[1] * A[1, c]) + r[2] * A[2, c]) + b[c] for c in range(3)])


def depth_normal(d, fx, fy, cx, cy):
    """gs_mapper.depth_to_normal: d fp32 [H,W] -> fp32 [3,H,W], zero on the one-pixel border"""
    d = np.asarray(d, f32)
    H, W = d.shape
    n = np.zeros((3, H, W), f32)
    if H < 3 or W < 3:
        return n
    fx, fy, cx, cy = f32(fx), f32(fy), f32(cx), f32(cy)
    rx = ((np.arange(W, dtype=f32) - cx) / fx)[None, :]
    ry = ((np.arange(H, dtype=f32) - cy) / fy)[:, None]
    p = np.stack([rx * d, ry * d, d])                                     # (1 * d == d exactly)
    a = p[:, 1:-1, 2:] - p[:, 1:-1, :-2]
    b = p[:, 2:, 1:-1] - p[:, :-2, 1:-1]
    c0 = a[1] * b[2] - a[2] * b[1]
    c1 = a[2] * b[0] - a[0] * b[2]
    c2 = a[0] * b[1] - a[1] * b[0]
    ln = np.maximum(np.sqrt((c0 * c0 + c1 * c1) + c2 * c2), f32(1e-12))
    n[:, 1:-1, 1:-1] = np.stack([c0 / ln, c1 / ln, c2 / ln])
    return n


def normal_cell(n):
    return color_cell((np.asarray(n, f32) + f32(1)) * f32(0.5))


def panel(gt, render, exposure_a, exposure_b, gt_depth, depth, normal, alpha, fx, fy, cx, cy):
    """uint8 [3H,3W,3]; gt, render, normal [3,H,W]; gt_depth, depth, alpha [H,W]"""
    gt, render = np.asarray(gt, f32), np.asarray(render, f32)
    gt_depth, depth, alpha = (np.asarray(t, f32).reshape(gt.shape[1:]) for t in (gt_depth, depth, alpha))
    err = np.abs(gt - exposure(render, exposure_a, exposure_b)) * f32(10)
    row0 = [color_cell(gt), color_cell(render), color_cell(err)]
    row1 = [turbo_cell(gt_depth), turbo_cell(depth), turbo_cell(np.abs(gt_depth - depth))]
    row2 = [normal_cell(normal), normal_cell(depth_normal(depth, fx, fy, cx, cy)), turbo_cell((alpha > f32(0.5)).astype(f32))]
    return np.concatenate([np.concatenate(r, 1) for r in (row0, row1, row2)], 0)


def frame(src, layer, depth_range=None):
    """uint8 [H,W,3] of one layer: "rgb" / "normal" of src [3,H,W], "depth" of src [H,W] over its own range or a fixed (near, far)"""
    if layer == "rgb":
        return color_cell(src)
    if layer == "normal":
        return normal_cell(src)
    src = np.asarray(src, f32)
    src = src.reshape(src.shape[-2:])
    return turbo_cell(src) if depth_range is None else turbo_cell(src, depth_range[0], depth_range[1])
