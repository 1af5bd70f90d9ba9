"""GPU, end to end: demo.py --mesh --gt-mesh --eval-2d scores a run's mesh against itself with the 2-D depth metric, leaves the trajectory
and the 3-D scores as they are, and without the switch writes the file it wrote before."""
import ast
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cut3r_slam_amd import tsdf as T  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_demo_eval_2d_adds_the_depth_l1_and_nothing_else(tmp_path, monkeypatch):
    import demo
    from cut3r_slam_amd import eval_recon as ER
    from cut3r_slam_amd import stream
    from tests.test_stream_gpu import _write_sequence
    d = tmp_path / "colors"
    d.mkdir()
    _write_sequence(str(d), 36)
    calib = tmp_path / "calib.txt"
    calib.write_text("600.0 600.0 320.0 240.0")
    base = ["--imagedir", str(d), "--calib", str(calib), "--kf_every", "2", "--synthetic-weights", "--small", "--seed", "1"]
    seen = []
    real = stream.save_trajectory

    def spy(slam, *a, **k):
        seen.append(slam)
        return real(slam, *a, **k)

    monkeypatch.setattr(stream, "save_trajectory", spy)
    assert demo.main(base + ["--output", str(tmp_path / "plain")]) == 0
    kf = seen[0].keyframes
    n = kf.counter.value - 1
    dep = kf.depth[:n]
    depth_max = float(dep[(dep > 0) & torch.isfinite(dep)].max())
    lo, hi = T.depth_bounds(dep, kf.w2c[:n], kf.intrinsic[:n].to(DEV), depth_max)
    voxel = float(np.max(hi - lo)) / 64
    mesh_args = ["--mesh", "--voxel-size", repr(voxel), "--depth-max", repr(depth_max)]
    first = tmp_path / "first"
    assert demo.main(base + ["--output", str(first)] + mesh_args) == 0
    gt = first / "tsdf_mesh_w1.0.ply"
    three = tmp_path / "three"
    assert demo.main(base + ["--output", str(three), "--gt-mesh", str(gt)] + mesh_args) == 0
    calls = []
    real_2d = ER.calc_2d_metric
    monkeypatch.setattr(ER, "calc_2d_metric", lambda *a, **k: calls.append(k) or real_2d(*a, **k))
    both = tmp_path / "both"
    assert demo.main(base + ["--output", str(both), "--gt-mesh", str(gt), "--eval-2d", "--n-imgs", "4"] + mesh_args) == 0
    assert len(calls) == 1 and calls[0]["n_imgs"] == 4 and calls[0]["unseen"] is None
    assert (both / "traj_kf.txt").read_bytes() == (three / "traj_kf.txt").read_bytes() == (tmp_path / "plain" / "traj_kf.txt").read_bytes()
    res3 = ast.literal_eval((three / "eval_recon_w1.0.txt").read_text())
    res = ast.literal_eval((both / "eval_recon_w1.0.txt").read_text())
    assert set(res3) == {"accuracy", "completion", "completion_ratio"}
    assert set(res) == {"accuracy", "completion", "completion_ratio", "depth l1"}
    print(f"3-D {res3}, with --eval-2d {res}")
    assert res["depth l1"] == 0.0
    # without the switch: the file of before, i.e. exactly the text of the 3-D result
    assert (three / "eval_recon_w1.0.txt").read_text() == f"{ {k: res[k] for k in res3} }" == f"{res3}"
    # an unseen cloud the views must avoid, given as a file
    mesh = T.read_ply(gt)
    np.save(tmp_path / "unseen.npy", mesh.vertices[:1] + np.float32([0.0, 0.0, 0.0]))
    cloud = tmp_path / "cloud"
    assert demo.main(base + ["--output", str(cloud), "--gt-mesh", str(gt), "--eval-2d", "--n-imgs", "3", "--gt-unseen",
                             str(tmp_path / "unseen.npy")] + mesh_args) == 0
    assert calls[1]["unseen"].shape == (1, 3)
    assert ast.literal_eval((cloud / "eval_recon_w1.0.txt").read_text())["depth l1"] == 0.0
    with pytest.raises(SystemExit):
        demo.main(base + ["--output", str(tmp_path / "bad"), "--eval-2d"] + mesh_args)
