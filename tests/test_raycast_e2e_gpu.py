"""GPU, end to end: the ray cast behind the public surface -- eval_dense.from_volume / from_slam(source="fused") on a small synthetic
keyframe store (the box room of tests/consistency_oracle.py), Cut3rSlam.ray_cast, dense_metrics on the fused depth maps, and one tiny
demo.py --mesh --mesh-preview run whose PNGs decode to the cast images."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cut3r_slam_amd import eval_dense as ED  # noqa: E402
from cut3r_slam_amd import tsdf as T  # noqa: E402
from cut3r_slam_amd.slam import Cut3rSlam  # noqa: E402
from tests import consistency_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VOXEL, TRUNC_VOXELS, DEPTH_MAX = 0.1, 3.0, 6.0


@pytest.fixture(scope="module")
def run():
    """a stand-in for a finished run: the keyframe store of the box-room walk and the two methods of Cut3rSlam that the sources use"""
    depth, w2c, K = O.box_room()
    n, H, W = depth.shape
    c, Rm = O.room_cameras()
    pose = np.zeros((n, 7))
    pose[:, :3] = c
    for i, R in enumerate(Rm):
        w = 0.5 * np.sqrt(1 + np.trace(R))
        pose[i, 3:] = [(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w]
    g = torch.Generator().manual_seed(0)
    kf = SimpleNamespace(device=torch.device(DEV), depth=torch.from_numpy(depth).to(DEV), w2c=torch.from_numpy(w2c).float().to(DEV),
                         image=torch.randint(0, 256, (n, 3, H, W), generator=g, dtype=torch.uint8).to(DEV), intrinsic=torch.from_numpy(K),
                         pose=torch.from_numpy(pose), tstamp=torch.arange(float(n)), conf_ds=None, downsample_ratio=1,
                         counter=SimpleNamespace(value=n + 1))
    slam = SimpleNamespace(keyframes=kf, mapper=None, tracked_only=False)
    slam.fuse = lambda voxel_size, source="auto", **k: T.fuse_keyframes(kf, n, voxel_size, trunc_voxels=TRUNC_VOXELS, depth_max=DEPTH_MAX, **k)
    return slam, depth


def _want(vol, views, **cast):
    n, H, W = views.depth.shape
    w2c = np.linalg.inv(ED.pose_matrices(views.c2w))[:, :3].reshape(n, 12).astype(np.float32)
    return vol.ray_cast(w2c, np.asarray(views.K, np.float32), H, W, **cast)


@pytest.mark.parametrize("sparse", [False, True])
def test_from_volume_is_the_ray_cast_of_the_keyframes(run, sparse):
    slam, depth = run
    vol = slam.fuse(VOXEL, sparse=sparse)
    views = ED.from_keyframes(slam.keyframes, depth.shape[0])
    want = _want(vol, views)
    got = ED.from_volume(vol, views)
    assert torch.equal(got.depth, want.depth) and torch.equal(got.rgb, want.color)
    assert np.array_equal(got.c2w, views.c2w) and np.array_equal(got.stamps, views.stamps) and np.array_equal(got.K, views.K)
    # the fused model seen from inside the room: nearly every ray hits a wall, within a voxel of the depth map that was fused
    hit = got.depth > 0
    assert float(hit.float().mean()) > 0.95
    assert float((got.depth - slam.keyframes.depth)[hit].abs().median()) < 0.5 * VOXEL
    # the options go through
    thick = ED.from_volume(vol, views, weight_threshold=3.0, step_voxels=1.0)
    assert torch.equal(thick.depth, _want(vol, views, weight_threshold=3.0, step_voxels=1.0).depth) and not torch.equal(thick.depth, got.depth)


def test_from_slam_fused_reaches_it_and_dense_metrics_runs(run):
    slam, depth = run
    vol = slam.fuse(VOXEL)
    views = ED.from_keyframes(slam.keyframes, depth.shape[0])
    given = ED.from_slam(slam, "fused", volume=vol)
    made = ED.from_slam(slam, "fused", fuse={"voxel_size": VOXEL})
    assert torch.equal(given.depth, ED.from_volume(vol, views).depth) and torch.equal(made.depth, given.depth)
    with pytest.raises(ValueError):
        ED.from_slam(slam, "fused")
    with pytest.raises(ValueError):
        ED.from_slam(slam, "volume")
    rc = Cut3rSlam.ray_cast(slam, volume=vol)
    assert torch.equal(rc.depth, given.depth) and rc.normal.shape == given.depth.shape + (3,)
    assert torch.equal(Cut3rSlam.ray_cast(slam, voxel_size=VOXEL, colors=False).depth, given.depth)
    with pytest.raises(ValueError):
        Cut3rSlam.ray_cast(slam)
    # the inward normals of a box seen from inside point at the viewer: n . (camera - surface) > 0 on (nearly) every hit
    c2w = ED.pose_matrices(views.c2w)
    hit = rc.depth > 0
    for b in range(depth.shape[0]):
        K = np.asarray(views.K, np.float64)[b]
        v, u = np.nonzero(hit[b].cpu().numpy())
        d = rc.depth[b].cpu().numpy()[v, u].astype(np.float64)
        p = (np.stack([(u - K[2]) / K[0] * d, (v - K[3]) / K[1] * d, d], 1) @ c2w[b, :3, :3].T) + c2w[b, :3, 3]
        facing = (rc.normal[b].cpu().numpy()[v, u] * (c2w[b, :3, 3] - p)).sum(1)
        assert (facing > 0).mean() > 0.99
    gt = ED.DepthViews(torch.from_numpy(depth), views.c2w, views.K, views.stamps, None)
    res = ED.dense_metrics(given, gt, depth_trunc=DEPTH_MAX)
    assert res["pairs"] == depth.shape[0] and res["n_est"] > 0.9 * res["n_gt"]
    assert np.isfinite(res["Chamfer_distance"]) and res["Chamfer_distance"] < VOXEL


def test_demo_mesh_preview_writes_the_cast_images(tmp_path, monkeypatch):
    """one tiny demo.py --mesh --mesh-preview 2 run with random weights: three PNGs per chosen keyframe, the depth PNG being the cast
    depth at DEPTH_SCALE.  (The random network's depth scale sets the voxel, so the spy on fuse replaces the command line's voxel size
    and depth range by the store's.)"""
    import demo
    from PIL import Image
    from tests.test_stream_gpu import _write_sequence
    d = tmp_path / "colors"
    d.mkdir()
    _write_sequence(str(d), 36)
    (tmp_path / "calib.txt").write_text("600.0 600.0 320.0 240.0")
    seen, real = [], Cut3rSlam.fuse

    def fuse(self, voxel_size, depth_max=5.0, **k):
        kf = self.keyframes
        n = kf.counter.value - 1
        dep = kf.depth[:n]
        top = float(dep[(dep > 0) & torch.isfinite(dep)].max())
        lo, hi = T.depth_bounds(dep, kf.w2c[:n], kf.intrinsic[:n].to(DEV), top)
        vol = real(self, float(np.max(hi - lo)) / 64, depth_max=top, **k)
        seen.append((self, vol))
        return vol
    monkeypatch.setattr(Cut3rSlam, "fuse", fuse)
    out = tmp_path / "out"
    assert demo.main(["--imagedir", str(d), "--calib", str(tmp_path / "calib.txt"), "--kf_every", "2", "--synthetic-weights", "--small",
                      "--seed", "1", "--output", str(out), "--mesh", "--mesh-preview", "2"]) == 0
    slam, vol = seen[0]
    rc = slam.ray_cast(volume=vol)
    n = rc.depth.shape[0]
    names = sorted(os.listdir(out / "tsdf_preview"))
    assert n >= 3 and names == sorted(f"{k:05d}_{what}.png" for k in range(0, n, 2) for what in ("depth", "normal", "color"))
    for k in range(0, n, 2):
        png = np.asarray(Image.open(out / "tsdf_preview" / f"{k:05d}_depth.png"))
        want = torch.floor(torch.clamp(rc.depth[k] * T.DEPTH_SCALE, 0, 65535)).cpu().numpy().astype(np.uint16)
        assert png.dtype == np.uint16 and np.array_equal(png, want)
        col = np.asarray(Image.open(out / "tsdf_preview" / f"{k:05d}_color.png"))
        assert np.array_equal(col, rc.color[k].permute(1, 2, 0).cpu().numpy())
        nrm = np.asarray(Image.open(out / "tsdf_preview" / f"{k:05d}_normal.png"))
        assert nrm.shape == col.shape and not nrm[png == 0].any()
