"""GPU, end to end: the sparse brick volume behind the driver -- Cut3rSlam.fuse(sparse=True) on a tracking run's keyframe store gives
the dense fuse()'s mesh as a set of triangles, and demo.py --mesh --mesh-sparse writes the PLY of the dense run."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cut3r_slam_amd import synth  # noqa: E402
from cut3r_slam_amd import tsdf as T  # noqa: E402
from cut3r_slam_amd.config import tiny_config  # noqa: E402
from cut3r_slam_amd.model import Cut3rModel  # noqa: E402
from cut3r_slam_amd.slam import Cut3rSlam  # noqa: E402
from cut3r_slam_amd.weights import synth_state_dict  # noqa: E402
from tests import tsdf_sparse_oracle as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_driver_fuse_sparse_gives_the_dense_mesh():
    """the tiny-config run of test_tsdf_e2e_gpu.py"""
    H, W = 32, 48
    cfg = tiny_config("dpt")
    model = Cut3rModel(cfg, synth_state_dict(cfg, 3), DEV, minimal=True)
    cfgd = {"Tracking": {"motion_filter": {"thresh": 0.9, "skip": 1, "kf_every": 2}, "frontend": {"iteration": 0}}}
    slam = Cut3rSlam(model, cfgd, (H, W), buffer=40, device=DEV)
    n = 40
    frames = synth.pan_stream(n, H, W, pool=5, num=2, den=1, seed=0)
    intr = torch.tensor([40.0, 40.0, 23.5, 15.5])
    for t in range(n):
        slam.run(t, frames[t:t + 1], intr, frames[t:t + 1], intr, last_frame=(t == n - 1))
    torch.cuda.synchronize()
    kf = slam.keyframes
    nkf = kf.counter.value - 1
    d = kf.depth[:nkf]
    valid = d[(d > 0) & torch.isfinite(d)]
    depth_max = float(torch.quantile(valid.float(), 0.9))
    lo, hi = T.depth_bounds(d, kf.w2c[:nkf], kf.intrinsic[:nkf].to(DEV), depth_max)
    voxel = float(np.max(hi - lo)) / 48
    conf = kf.conf_ds[torch.arange(nkf, device=DEV) // 5, torch.arange(nkf, device=DEV) % 5]
    conf_min = float(torch.quantile(conf.flatten().float(), 0.25))
    for kw in ({}, {"conf_min": conf_min}, {"bounds": (lo, hi), "source": "tracker"}):
        dense = slam.fuse(voxel, depth_max=depth_max, trunc_voxels=4.0, **kw)
        sparse = slam.fuse(voxel, depth_max=depth_max, trunc_voxels=4.0, sparse=True, **kw)
        assert isinstance(sparse, T.SparseTSDFVolume) and isinstance(dense, T.TSDFVolume)
        assert sparse.dims == dense.dims and sparse.origin == dense.origin and sparse.n_bricks > 0
        vm = sparse.allocated_mask()
        for a, b in zip(sparse.to_dense(), (dense.tsdf, dense.weight, dense.color)):
            m = vm if a.dim() == 3 else vm[None].expand_as(a)
            assert torch.equal(a[m].view(torch.int32), b[m].view(torch.int32))
        assert not bool(((dense.tsdf < 0) & ~vm).any())
        for thr in (1.0, 2.0):
            ms, md = sparse.extract_mesh(thr), dense.extract_mesh(thr)
            assert len(md.faces) > 0 and len(ms.faces) == len(md.faces) and len(ms.vertices) == len(md.vertices)
            assert np.array_equal(S.soup(*ms), S.soup(*md))
    m1 = slam.reconstruct(voxel, depth_max=depth_max, trunc_voxels=4.0, weight_threshold=2.0, source="tracker", sparse=True)
    m2 = slam.reconstruct(voxel, depth_max=depth_max, trunc_voxels=4.0, weight_threshold=2.0, source="tracker")
    assert len(m1.faces) > 0 and np.array_equal(S.soup(*m1), S.soup(*m2))


def test_demo_mesh_sparse_writes_the_dense_runs_mesh(tmp_path, monkeypatch, capsys):
    import demo
    from cut3r_slam_amd import stream
    from tests.test_stream_gpu import _write_sequence
    d = tmp_path / "colors"
    d.mkdir()
    _write_sequence(str(d), 36)
    calib = tmp_path / "calib.txt"
    calib.write_text("600.0 600.0 320.0 240.0")
    base = ["--imagedir", str(d), "--calib", str(calib), "--kf_every", "2", "--synthetic-weights", "--small", "--seed", "1"]
    with pytest.raises(SystemExit):
        demo.main(base + ["--output", str(tmp_path / "bad"), "--mesh-sparse"])          # needs --mesh
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
    mesh_args = ["--mesh", "--voxel-size", repr(voxel), "--depth-max", repr(depth_max), "--mesh-weight", "1", "2"]
    capsys.readouterr()
    assert demo.main(base + ["--output", str(tmp_path / "dense")] + mesh_args) == 0
    assert "bricks" not in capsys.readouterr().out
    assert demo.main(base + ["--output", str(tmp_path / "sparse"), "--mesh-sparse"] + mesh_args) == 0
    out = capsys.readouterr().out
    assert "bricks allocated" in out and "GB" in out
    assert (tmp_path / "sparse" / "traj_kf.txt").read_bytes() == (tmp_path / "plain" / "traj_kf.txt").read_bytes()
    for w in ("1.0", "2.0"):
        ms, md = T.read_ply(tmp_path / "sparse" / f"tsdf_mesh_w{w}.ply"), T.read_ply(tmp_path / "dense" / f"tsdf_mesh_w{w}.ply")
        assert len(ms.faces) == len(md.faces) >= 1 and ms.faces.max() < len(ms.vertices)
        assert np.array_equal(S.soup(*ms), S.soup(*md))
