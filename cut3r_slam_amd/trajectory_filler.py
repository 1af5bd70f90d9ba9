"""Poses of the frames between the keyframes (hislam2/util/trajectory_filler.py:15-114 PoseTrajectoryFiller, run by
Hi2.terminate(fill=True)): every non-keyframe is registered against the FROZEN Gaussian map by `GSMapper.pose_estimator`
(hislam2/gs_backend_per_frame.py:123-177), starting from the pose of the frame before it.

Not built: the reference's unused `_PnP` helper (cv2.solvePnPRansac, never called by `run`)."""
from __future__ import annotations

import numpy as np
import torch


class PoseTrajectoryFiller:
    """fills in the non-keyframe poses of a finished run"""

    def __init__(self, slam):
        self.mapper = slam.mapper
        self.keyframes = slam.keyframes

    def fill(self, tstamp0, tstamp1, images, pose0, iters=100):
        """trajectory_filler.py:60-85: the frames strictly between tstamp0 and tstamp1, each started from the estimate of the one
        before it (the first from pose0) -> list of [7] camera->world poses"""
        out, prev = [], pose0
        for i in range(tstamp0 + 1, tstamp1):
            with torch.enable_grad():
                prev = self.mapper.pose_estimator(prev, images[i], i, iters=iters)
            out.append(torch.as_tensor(prev, dtype=torch.float32).cpu())
        return out

    @torch.no_grad()
    def run(self, images, iters=100):
        """trajectory_filler.py:88-114.  images: the frames by tstamp (a dict or a sequence; len(images) frames).  kf_num = counter - 1
        keyframes take part; for each of them the rows are its own pose, then the frames up to the next keyframe's tstamp, the last
        segment runs to len(images).  Returns (tstamps [n] int64, poses [n,7] float32 camera->world, t + q_xyzw) as numpy; the rows start at
        the first keyframe's tstamp, n = len(images) - tstamp[0]."""
        kf = self.keyframes
        kf_num = kf.counter.value - 1
        if kf_num < 1:
            raise RuntimeError("PoseTrajectoryFiller: no tracked keyframe")
        stamps, rows = [], []
        for i in range(kf_num):
            t0 = int(kf.tstamp[i])
            t1 = int(kf.tstamp[i + 1]) if i < kf_num - 1 else len(images)
            pose0 = torch.as_tensor(kf.pose[i], dtype=torch.float32).cpu()
            rows.append(pose0)
            rows += self.fill(t0, t1, images, pose0, iters)
            stamps += list(range(t0, max(t1, t0 + 1)))
        return np.asarray(stamps, dtype=np.int64), torch.stack(rows).numpy()
