"""GPU, end to end: TSDF fusion of a tracking run's keyframe store (bit for bit against the numpy oracle fed with the same store
tensors), demo.py --mesh (a PLY next to an unchanged traj_kf.txt), and the Gaussian mapper's rendered keyframes fused onto the wall
they were trained on."""
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
from tests import tsdf_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _same_volume(vol, ref):
    for name, a, b in zip(("tsdf", "weight", "color"), (vol.tsdf, vol.weight, vol.color), ref):
        a = a.cpu().numpy()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{name}: {np.count_nonzero(a != b)} voxels differ"


def _same_mesh(mesh, ref):
    v, c, f = ref
    assert mesh.vertices.shape == v.shape and mesh.faces.shape == f.shape
    assert np.array_equal(mesh.vertices.view(np.uint32), v.view(np.uint32)) and np.array_equal(mesh.colors, c)
    assert np.array_equal(mesh.faces, f)


def test_tracker_keyframes_fuse_like_the_oracle():
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
    assert nkf >= 10 and nkf == len(slam.trajectory()[0])
    # random weights have no metric scale: the voxel and depth_max come from the store's own depths
    d = kf.depth[:nkf]
    valid = d[(d > 0) & torch.isfinite(d)]
    assert valid.numel() > 0.5 * d.numel()
    depth_max = float(torch.quantile(valid.float(), 0.9))              # the farthest tenth is rejected
    lo, hi = T.depth_bounds(d, kf.w2c[:nkf], kf.intrinsic[:nkf].to(DEV), depth_max)
    voxel = float(np.max(hi - lo)) / 48
    idx = torch.arange(nkf, device=DEV)
    conf = kf.conf_ds[idx // 5, idx % 5].contiguous()
    conf_min = float(torch.quantile(conf.flatten().float(), 0.25))      # a quarter of the pixels fail the gate
    vol = T.fuse_keyframes(kf, nkf, voxel, trunc_voxels=4.0, depth_max=depth_max, conf_min=conf_min)
    ref = O.integrate(O.new_volume(vol.dims), vol.origin, vol.voxel_size, d.cpu().numpy(), kf.w2c[:nkf].cpu().numpy(),
                      kf.intrinsic[:nkf].numpy(), vol.trunc, vol.depth_max, rgb=kf.image[:nkf].cpu().numpy(), conf=conf.cpu().numpy(),
                      conf_ds=kf.downsample_ratio, conf_min=conf_min)
    assert (ref[1] > 0).mean() > 0.05
    _same_volume(vol, ref)
    mesh = vol.extract_mesh(1.0)
    assert len(mesh.faces) > 0
    _same_mesh(mesh, O.extract(ref, vol.origin, vol.voxel_size, 1.0))
    # the driver's entry point: the tracked keyframes, no confidence gate by default
    vol2 = slam.fuse(voxel, depth_max=depth_max, trunc_voxels=4.0, source="auto", bounds=(lo, hi))
    ref2 = O.integrate(O.new_volume(vol2.dims), vol2.origin, vol2.voxel_size, d.cpu().numpy(), kf.w2c[:nkf].cpu().numpy(),
                       kf.intrinsic[:nkf].numpy(), vol2.trunc, vol2.depth_max, rgb=kf.image[:nkf].cpu().numpy())
    _same_volume(vol2, ref2)
    m2 = slam.reconstruct(voxel, depth_max=depth_max, trunc_voxels=4.0, weight_threshold=2.0, source="tracker")
    assert len(m2.faces) > 0 and m2.faces.max() < len(m2.vertices)


def test_demo_writes_a_mesh_and_leaves_the_trajectory_unchanged(tmp_path, monkeypatch):
    import demo
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
    # the random network's depth scale sets the voxel: 64 voxels over the largest extent of the fused points
    kf = seen[0].keyframes
    n = kf.counter.value - 1
    dep = kf.depth[:n]
    depth_max = float(dep[(dep > 0) & torch.isfinite(dep)].max())
    lo, hi = T.depth_bounds(dep, kf.w2c[:n], kf.intrinsic[:n].to(DEV), depth_max)
    voxel = float(np.max(hi - lo)) / 64
    out = tmp_path / "mesh"
    assert demo.main(base + ["--output", str(out), "--mesh", "--voxel-size", repr(voxel), "--depth-max", repr(depth_max),
                             "--mesh-weight", "1", "2"]) == 0
    assert (out / "traj_kf.txt").read_bytes() == (tmp_path / "plain" / "traj_kf.txt").read_bytes()
    for w in ("1.0", "2.0"):
        mesh = T.read_ply(out / f"tsdf_mesh_w{w}.ply")
        assert len(mesh.faces) >= 1 and mesh.faces.max() < len(mesh.vertices) and np.isfinite(mesh.vertices).all()
    assert len(T.read_ply(out / "tsdf_mesh_w2.0.ply").faces) <= len(T.read_ply(out / "tsdf_mesh_w1.0.ply").faces) * 2


def _wall_z(x, y):
    return 3.0 + 0.2 * np.sin(x) * np.cos(1.3 * y)


def test_mapper_renders_fuse_onto_the_wall():
    from cut3r_slam_amd import gs_mapper as GM
    H, W, f = 96, 128, 110.0
    packet, _, cfg = synth.gs_wall_window(H, W, focal=f, n_views=4, device=DEV)
    mapper = GM.GSMapper(cfg, f, f, W / 2, H / 2, downsample_ratio=2, device=DEV)
    with torch.enable_grad():
        mapper.run(packet, iterations=30)
    voxel = 0.03
    vol = T.fuse_mapper(mapper, voxel, trunc_voxels=4.0)
    mesh = vol.extract_mesh(1.0)
    assert len(mesh.faces) > 1000
    # the same renders through the oracle: the same volume and mesh
    depth, rgb, w2c, K = T.render_mapper_views(mapper)
    assert depth.shape == (4, H, W) and rgb.dtype == torch.uint8
    q = depth.double() * T.DEPTH_SCALE
    assert float((q - q.round()).abs().max()) < 1e-2                                        # uint16 steps of 1 / 6553.5 m
    again = T.TSDFVolume(vol.origin, vol.voxel_size, vol.dims, trunc_voxels=4.0, device=DEV).integrate(depth, w2c, K, rgb=rgb)
    ref = O.integrate(O.new_volume(vol.dims), vol.origin, vol.voxel_size, depth.cpu().numpy(), w2c.cpu().numpy(), K.cpu().numpy(), vol.trunc,
                      vol.depth_max, rgb=rgb.cpu().numpy())
    _same_volume(again, ref)
    ov, oc, of = O.extract(ref, vol.origin, vol.voxel_size, 1.0)
    _same_mesh(again.extract_mesh(1.0), (ov, oc, of))
    # distance to the wall the mapper was trained on, in voxels.  The oracle's mesh of the same renders (the mapper after 30 iterations per
    # call on 4 views at 128x96) gives median 0.49, p90 1.34, max 2.36 voxels: the bounds leave ~20 % room
    v = mesh.vertices.astype(np.float64)
    err = np.abs(v[:, 2] - _wall_z(v[:, 0], v[:, 1])) / voxel
    oerr = np.abs(ov[:, 2].astype(np.float64) - _wall_z(ov[:, 0].astype(np.float64), ov[:, 1].astype(np.float64))) / voxel
    print(f"wall distance in voxels: GPU mesh median {np.median(err):.3f} p90 {np.percentile(err, 90):.3f}; "
          f"oracle median {np.median(oerr):.3f} p90 {np.percentile(oerr, 90):.3f} max {oerr.max():.3f}")
    assert np.median(err) <= 0.6 and np.percentile(err, 90) <= 1.6 and err.max() <= 3.0
