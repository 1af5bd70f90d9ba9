"""Run without a calibration file: the focal length from the network's own self-view pointmaps.

`estimate_focal_knowing_depth` has the signature and the return value of the reference's function (src/dust3r/post_process.py:12-64,
which hislam2/track_frontend.py:10 imports in a comment) plus an optional confidence gate; both estimators are HIP kernels
(csrc/calib.hip, ops.focal_median / ops.focal_weiszfeld), the final clip is one elementwise op.  `SelfCalibration` is the tracker's policy
on top of it: one focal for the run from the per-view estimates of the first window, with the principal point at the image centre.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import ops

MODES = ("median", "weiszfeld")


def focal_base(H: int, W: int) -> float:
    """post_process.py:59-61: the focal of a 60 degree field of view over the longer side, max(H, W) / (2 tan 30 deg)"""
    return max(H, W) / (2 * np.tan(np.deg2rad(60) / 2))


def estimate_focal_knowing_depth(pts3d, pp, focal_mode="median", min_focal=0.0, max_focal=np.inf, conf=None, conf_min=None):
    """pts3d fp32 [B,H,W,3] and pp fp32 [B,2] (or [2] for all views) on the GPU -> focal fp32 [B] on the GPU, clipped to
    [min_focal, max_focal] x focal_base (NaN stays NaN).  conf fp32 [B,H,W] with conf_min: pixels below it take no part."""
    B, H, W, THREE = pts3d.shape
    assert THREE == 3
    if focal_mode not in MODES:
        raise ValueError(f"bad {focal_mode=}")
    pp = pp.reshape(-1, 2).expand(B, 2).contiguous()
    if focal_mode == "median":
        focal = ops.focal_median(pts3d, pp, conf=conf, conf_min=conf_min)
    else:
        focal = ops.focal_weiszfeld(pts3d, pp, iters=10, conf=conf, conf_min=conf_min)
    base = focal_base(H, W)
    return focal.clamp_(min=min_focal * base, max=max_focal * base)


class SelfCalibration:
    """The policy of an uncalibrated run (config section Tracking.calibration): mode `weiszfeld` (what CUT3R's own demo uses) or `median`;
    conf_min gates pixels by the network's confidence (None: no gate); min_focal / max_focal bound the estimate in units of focal_base --
    0.25 .. 4 is a field of view between roughly 133 and 16 degrees.  The bounds are declared policy, not measurements: an estimate on a
    bound means that the pointmaps carry no usable geometry."""

    DEFAULTS = {"mode": "weiszfeld", "conf_min": None, "min_focal": 0.25, "max_focal": 4.0}

    def __init__(self, cfg=None):
        sec = dict(self.DEFAULTS)
        sec.update(((cfg or {}).get("Tracking", {}) or {}).get("calibration", {}) or {})
        unknown = set(sec) - set(self.DEFAULTS)
        if unknown:
            raise ValueError(f"Tracking.calibration: unknown keys {sorted(unknown)}")
        if sec["mode"] not in MODES:
            raise ValueError(f"Tracking.calibration.mode must be one of {MODES}, not {sec['mode']!r}")
        self.mode = sec["mode"]
        self.conf_min = None if sec["conf_min"] is None else float(sec["conf_min"])
        self.min_focal, self.max_focal = float(sec["min_focal"]), float(sec["max_focal"])
        if not (0 <= self.min_focal < self.max_focal):
            raise ValueError("Tracking.calibration: 0 <= min_focal < max_focal")
        self.per_view = None            # the clipped per-view estimates of the window that calibrated the run
        self.intrinsics = None          # (fx, fy, cx, cy) at the tracking resolution
        self.count = 0                  # calibrations performed (a run performs one)

    def bounds(self, H, W):
        """the clip bounds as the fp32 values a clipped estimate carries"""
        base = focal_base(H, W)
        return float(np.float32(self.min_focal * base)), float(np.float32(self.max_focal * base))

    def select(self, per_view, H, W):
        """host half: per-view estimates (clipped, NaN for a view without votes) -> (fx, fy, cx, cy); the lower median of the finite ones"""
        vals = [float(v) for v in np.asarray(per_view, np.float32).reshape(-1)]
        finite = sorted(v for v in vals if math.isfinite(v))
        if not finite:
            raise RuntimeError(f"self-calibration: no view of the window yields a finite focal (per view: {vals}); pass a calibration")
        f = finite[(len(finite) - 1) // 2]
        lo, hi = self.bounds(H, W)
        if f <= lo or f >= hi:
            raise RuntimeError(f"self-calibration: the focal estimate {f:g} sits on a bound of [{lo:g}, {hi:g}] (per view: {vals}): the "
                               "pointmaps carry no usable geometry; pass a calibration")
        return (f, f, W / 2.0, H / 2.0)

    def from_window(self, pts, conf=None):
        """pts fp32 [V,H,W,3], conf fp32 [V,H,W] of one window (device) -> (fx, fy, cx, cy).  One read-back of V floats."""
        V, H, W, _ = pts.shape
        pp = torch.tensor([W / 2.0, H / 2.0], dtype=torch.float32).to(pts.device)
        gate = self.conf_min is not None and conf is not None
        est = estimate_focal_knowing_depth(pts.contiguous(), pp, self.mode, self.min_focal, self.max_focal,
                                           conf.contiguous() if gate else None, self.conf_min if gate else None)
        per_view = est.cpu().numpy()                   # THE read-back of the calibration
        K = self.select(per_view, H, W)
        self.per_view, self.intrinsics = per_view, K
        self.count += 1
        return K
