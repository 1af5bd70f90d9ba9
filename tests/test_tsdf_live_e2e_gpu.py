"""GPU, end to end: the live TSDF volume behind the driver -- Cut3rSlam.start_live_volume keeps tsdf.LiveTSDFVolume in step with the
keyframe store during a tracking run and after poses and depths are rewritten, without touching the trajectory; demo.py --mesh-live writes
its mesh and previews."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cut3r_slam_amd import ops, synth  # noqa: E402
from cut3r_slam_amd import tsdf as T  # noqa: E402
from cut3r_slam_amd.config import tiny_config  # noqa: E402
from cut3r_slam_amd.model import Cut3rModel  # noqa: E402
from cut3r_slam_amd.slam import Cut3rSlam  # noqa: E402
from cut3r_slam_amd.weights import synth_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(live=None):
    """the tiny-config run of test_tsdf_sparse_e2e_gpu.py; live: the arguments of start_live_volume"""
    H, W = 32, 48
    cfg = tiny_config("dpt")
    model = Cut3rModel(cfg, synth_state_dict(cfg, 3), DEV, minimal=True)
    cfgd = {"Tracking": {"motion_filter": {"thresh": 0.9, "skip": 1, "kf_every": 2}, "frontend": {"iteration": 0}}}
    slam = Cut3rSlam(model, cfgd, (H, W), buffer=40, device=DEV)
    assert slam.live_volume is None
    if live is not None:
        slam.start_live_volume(**live)
    n = 40
    frames = synth.pan_stream(n, H, W, pool=5, num=2, den=1, seed=0)
    intr = torch.tensor([40.0, 40.0, 23.5, 15.5])
    for t in range(n):
        slam.run(t, frames[t:t + 1], intr, frames[t:t + 1], intr, last_frame=(t == n - 1))
    torch.cuda.synchronize()
    return slam


def _fresh_like(live, kf, n):
    vol = T.LiveTSDFVolume(live.origin, live.voxel_size, live.dims, trunc_voxels=4.0, depth_max=live.depth_max, device=DEV)
    assert vol.trunc == live.trunc
    assert vol.sync(kf, n) == (n, 0)
    return vol


def _assert_equal_on_the_fresh_bricks(live, fresh):
    assert fresh.n_bricks > 0 and bool((live.flags >= fresh.flags).all())
    slot = live.table.reshape(-1)[fresh.bricks.long()].long()
    assert torch.equal(live.acc[:, slot], fresh.acc)
    assert bool(fresh.acc[1].any()) and bool((fresh.acc[0] < 0).any())


def test_the_driver_keeps_the_live_volume_equal_to_a_fresh_fusion(monkeypatch):
    plain = _run()
    kf = plain.keyframes
    nkf = kf.counter.value - 1
    d = kf.depth[:nkf]
    valid = d[(d > 0) & torch.isfinite(d)]
    depth_max = float(torch.quantile(valid.float(), 0.9))
    lo, hi = T.depth_bounds(d, kf.w2c[:nkf], kf.intrinsic[:nkf].to(DEV), depth_max)
    voxel = float(np.max(hi - lo)) / 48                                 # as test_tsdf_sparse_e2e_gpu.py chooses it
    calls = []
    real = T.LiveTSDFVolume.sync

    def spy(self, *a, **k):
        out = real(self, *a, **k)
        calls.append(out)
        return out

    monkeypatch.setattr(T.LiveTSDFVolume, "sync", spy)
    slam = _run(dict(voxel_size=voxel, half_extent=float(np.max(hi - lo)), depth_max=depth_max, trunc_voxels=4.0))
    monkeypatch.setattr(T.LiveTSDFVolume, "sync", real)
    live, kf = slam.live_volume, slam.keyframes
    n = kf.counter.value - 1
    assert n == nkf and isinstance(live, T.LiveTSDFVolume) and isinstance(live, T._Volume) and sorted(live.records) == list(range(n))
    print(f"{len(calls)} syncs during the run: {sum(a for a, _ in calls)} keyframes added, {sum(u for _, u in calls)} updates")
    assert len(calls) > 0 and sum(a for a, _ in calls) == n, calls
    # the trajectory does not know about the volume
    for a, b in zip(slam.trajectory(), plain.trajectory()):
        assert a.tobytes() == b.tobytes()
    assert torch.equal(kf.w2c[:n], plain.keyframes.w2c[:n]) and torch.equal(kf.depth[:n], plain.keyframes.depth[:n])
    _assert_equal_on_the_fresh_bricks(live, _fresh_like(live, kf, n))
    assert live.sync(kf, n) == (0, 0)
    mesh = live.extract_mesh(1.0)
    assert len(mesh.faces) > 0 and mesh.faces.max() < len(mesh.vertices)
    rc = slam.ray_cast(volume=live, source="tracker")
    assert rc.depth.shape == (n, 32, 48) and int((rc.depth > 0).sum()) > 0
    # poses of three keyframes and depths of two rewritten in the store, as loop closure and the Sim(3) correction do
    g = np.random.default_rng(0)
    poses = kf.pose[[1, 4, 6]].numpy().copy()
    poses[:, :3] += g.uniform(-0.02, 0.02, (3, 3)).astype(np.float32)
    kf.set_poses_at([1, 4, 6], poses)
    ops.scale_planes(kf.depth[4:6], torch.tensor([1.03, 0.98], device=DEV))
    launches = []
    real_int = ops.tsdf_live_integrate
    monkeypatch.setattr(ops, "tsdf_live_integrate", lambda *a, **k: (launches.append(1), real_int(*a, **k))[1])
    assert live.sync(kf, n) == (0, 4)                                   # keyframes 1, 4, 5 and 6
    assert launches
    del launches[:]
    assert live.sync(kf, n) == (0, 0) and not launches
    _assert_equal_on_the_fresh_bricks(live, _fresh_like(live, kf, n))


def test_demo_mesh_live_writes_the_mesh_and_previews(tmp_path, monkeypatch, capsys):
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
        demo.main(base + ["--output", str(tmp_path / "bad"), "--mesh-live-preview", "4"])          # needs --mesh-live
    with pytest.raises(SystemExit):
        demo.main(base + ["--output", str(tmp_path / "bad"), "--mesh-live", "--mesh-live-extent", "0"])
    seen = []
    real = stream.save_trajectory

    def spy(slam, *a, **k):
        seen.append(slam)
        return real(slam, *a, **k)

    monkeypatch.setattr(stream, "save_trajectory", spy)
    assert demo.main(base + ["--output", str(tmp_path / "plain")]) == 0
    kf = seen[0].keyframes                                              # the scale of the scene, as test_tsdf_sparse_e2e_gpu.py takes it
    n = kf.counter.value - 1
    dep = kf.depth[:n]
    depth_max = float(dep[(dep > 0) & torch.isfinite(dep)].max())
    lo, hi = T.depth_bounds(dep, kf.w2c[:n], kf.intrinsic[:n].to(DEV), depth_max)
    extent = float(np.max(hi - lo))
    capsys.readouterr()
    out_dir = tmp_path / "live"
    assert demo.main(base + ["--output", str(out_dir), "--mesh-live", "--mesh-live-extent", repr(extent), "--voxel-size", repr(extent / 64),
                             "--depth-max", repr(depth_max), "--mesh-weight", "1", "--mesh-live-preview", "4"]) == 0
    out = capsys.readouterr().out
    assert "live TSDF" in out and "bricks allocated" in out
    assert (out_dir / "traj_kf.txt").read_bytes() == (tmp_path / "plain" / "traj_kf.txt").read_bytes()
    assert not (out_dir / "tsdf_mesh_w1.0.ply").exists()                # independent of --mesh: no fuse pass
    mesh = T.read_ply(out_dir / "tsdf_mesh_live_w1.0.ply")
    assert len(mesh.faces) >= 1 and mesh.faces.min() >= 0 and mesh.faces.max() < len(mesh.vertices)
    names = sorted(os.listdir(out_dir / "tsdf_live_preview"))
    assert len(names) >= 3 and len(names) % 3 == 0 and {n.split("_")[1] for n in names} == {"depth.png", "normal.png", "color.png"}
