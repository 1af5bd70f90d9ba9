"""CPU: the stitching of trajectory_filler.PoseTrajectoryFiller.run (hislam2/util/trajectory_filler.py:88-114) on a stub mapper, the
keep_images requirement of Cut3rSlam.terminate(fill=True), and the traj_full.txt writer."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cut3r_slam_amd import stream  # noqa: E402
from cut3r_slam_amd.slam import Cut3rSlam  # noqa: E402
from cut3r_slam_amd.trajectory_filler import PoseTrajectoryFiller  # noqa: E402


class _StubMapper:
    """pose_estimator returns prev + f(tstamp) and records its calls"""

    def __init__(self):
        self.calls = []

    def pose_estimator(self, prev, image, tstamp, gt_depth=None, iters=100):
        assert torch.is_grad_enabled()                                    # trajectory_filler.py:72: the filler re-enables autograd
        self.calls.append((int(tstamp), int(image), int(iters), torch.as_tensor(prev).clone()))
        return torch.as_tensor(prev) + float(tstamp) * 0.001


def _slam(kf_tstamps, counter):
    n = len(kf_tstamps)
    kf = types.SimpleNamespace(counter=types.SimpleNamespace(value=counter), tstamp=torch.tensor(kf_tstamps, dtype=torch.float),
                               pose=torch.arange(n * 7, dtype=torch.float).reshape(n, 7) * 100.0)
    return types.SimpleNamespace(mapper=_StubMapper(), keyframes=kf)


def test_segments_follow_the_reference_order():
    s = _slam([0, 3, 5, 9], counter=4)                                    # counter - 1 = 3 keyframes take part: the one at tstamp 9 does not
    images = list(range(8))                                               # (the stub reads the frame back as its index)
    ts, poses = PoseTrajectoryFiller(s).run(images, iters=7)
    assert ts.tolist() == list(range(8)) and poses.shape == (8, 7) and poses.dtype == np.float32
    kf = s.keyframes.pose.numpy()
    for row, k in ((0, 0), (3, 1), (5, 2)):
        assert np.array_equal(poses[row], kf[k])                          # a keyframe's own pose, bit for bit
    # every frame starts from the one before it; the first of a segment from its keyframe
    np.testing.assert_allclose(poses[1], kf[0] + 0.001, rtol=0, atol=1e-4)
    np.testing.assert_allclose(poses[2], kf[0] + 0.001 + 0.002, rtol=0, atol=1e-4)
    np.testing.assert_allclose(poses[4], kf[1] + 0.004, rtol=0, atol=1e-4)
    np.testing.assert_allclose(poses[7], kf[2] + 0.006 + 0.007, rtol=0, atol=1e-4)      # the tail runs to len(images)
    calls = s.mapper.calls
    assert [c[0] for c in calls] == [1, 2, 4, 6, 7] and all(c[1] == c[0] and c[2] == 7 for c in calls)      # frames looked up by tstamp
    assert torch.equal(calls[2][3], s.keyframes.pose[1]) and torch.equal(calls[1][3], torch.as_tensor(poses[1]))


def test_rows_start_at_the_first_keyframe():
    s = _slam([3, 6, 20], counter=3)                                      # two keyframes take part
    ts, poses = PoseTrajectoryFiller(s).run(list(range(9)), iters=1)
    assert ts.tolist() == [3, 4, 5, 6, 7, 8] and len(poses) == 9 - 3
    assert np.array_equal(poses[0], s.keyframes.pose[0].numpy()) and np.array_equal(poses[3], s.keyframes.pose[1].numpy())
    assert [c[0] for c in s.mapper.calls] == [4, 5, 7, 8]


def test_adjacent_keyframes_and_a_last_keyframe_on_the_last_frame():
    s = _slam([0, 1, 4, 9], counter=4)
    ts, poses = PoseTrajectoryFiller(s).run(list(range(5)), iters=1)
    assert ts.tolist() == [0, 1, 2, 3, 4] and [c[0] for c in s.mapper.calls] == [2, 3]
    assert np.array_equal(poses[4], s.keyframes.pose[2].numpy())
    with pytest.raises(RuntimeError):
        PoseTrajectoryFiller(_slam([0], counter=1)).run([0], iters=1)     # no tracked keyframe


def test_terminate_fill_needs_the_kept_frames():
    s = types.SimpleNamespace(keyframes=types.SimpleNamespace(counter=types.SimpleNamespace(value=3)), images={}, mapper=object())
    with pytest.raises(RuntimeError, match="keep_images"):
        Cut3rSlam.terminate(s, fill=True)


def test_traj_full_writer_round_trips(tmp_path):
    img_dir, out = tmp_path / "colors", tmp_path / "out"
    img_dir.mkdir()
    out.mkdir()
    for i in range(12):
        (img_dir / f"frame{10 * i:06d}.jpg").write_bytes(b"")
    kf = types.SimpleNamespace(counter=types.SimpleNamespace(value=3), tstamp=torch.tensor([3.0, 6.0, 0.0]),
                               pose=torch.rand(3, 7), intrinsic=torch.tensor([[100.0, 100.0, 64.0, 48.0]]))
    s = types.SimpleNamespace(keyframes=kf)
    g = np.random.default_rng(0)
    poses = g.standard_normal((9, 7)).astype(np.float32)
    idx = np.arange(3, 12)
    stream.save_trajectory(s, str(img_dir), str(out), traj_full=poses, traj_full_index=idx)
    back = np.loadtxt(out / "traj_full.txt")
    assert back.shape == (9, 8) and back[:, 0].tolist() == [10.0 * i for i in range(3, 12)]
    assert np.array_equal(back[:, 1:].astype(np.float32), poses)         # full precision: the rows read back are the rows written
    stream.save_trajectory(s, str(img_dir), str(out), traj_full=poses)    # the reference's stamping: the first len(traj_full) frames
    assert np.loadtxt(out / "traj_full.txt")[:, 0].tolist() == [10.0 * i for i in range(9)]
