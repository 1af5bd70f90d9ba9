"""GPU: what leaves the Gaussian mapper -- 3dgs_final.ply and gaussians_viz_{n}.ply from finalize(out_dir=...), the panel folders of
`viz_dir`, and the map renderer (gs_view.render_cloud, its command line) -- on the synthetic wall of tests/test_gs_mapper_gpu.py.  The
reference's backend cannot run here: functional tests, parity with its own files UNPINNED."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import test_gs_mapper_gpu as S  # noqa: E402  (the scene: _truth, _observe, _pose7, CONFIG and the camera constants)
from cut3r_slam_amd import gs_mapper as GM, gs_ply, gs_view, tsdf  # noqa: E402

DEV = S.DEV
K_SMALL = 6


@pytest.fixture(scope="module")
def mapper():
    """two keyframes of the wall, a few iterations"""
    truth = S._truth()
    poses = [S._pose7(0, 0, 0, 0, 0), S._pose7(0.15, 0.0, 0.0, 0.0, -0.04)]
    m = GM.GSMapper(S.CONFIG, S.FX, S.FY, S.CX, S.CY, downsample_ratio=2, device=DEV)
    for k, p in enumerate(poses):
        img, depth = S._observe(truth, p)
        m.add_new_view((img * 255).round().to(torch.uint8), p, depth, new_tstamp=10 * k, kf_sub_idx=k, iters=4)
    m.optimization(4, current_window=[0, 1])
    return m


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def test_finalize_writes_the_standard_ply_and_the_point_cloud(mapper, tmp_path):
    out = str(tmp_path / "run")
    assert mapper.viz_dir is None
    poses = mapper.finalize(iteration_total=K_SMALL, out_dir=out)
    assert poses.shape == (2, 7)
    assert sorted(os.listdir(out)) == ["3dgs_final.ply", f"gaussians_viz_{K_SMALL}.ply"]      # and no panel folder: viz_dir is None
    theta = mapper.gaussians.theta.detach()
    d = gs_ply.read_gaussian_ply(os.path.join(out, "3dgs_final.ply"))
    assert d["K"] == 1 and d["f_rest"].shape == (len(theta), 0, 3)
    cols = torch.from_numpy(np.concatenate([d["xyz"], d["f_dc"], d["opacity"], d["scaling"], d["rotation"]], 1))
    assert torch.equal(_bits(cols), _bits(theta.cpu()))
    pcd = tsdf.read_ply(os.path.join(out, f"gaussians_viz_{K_SMALL}.ply"))
    assert np.array_equal(pcd.vertices.view(np.uint32), theta[:, 0:3].cpu().numpy().view(np.uint32)) and len(pcd.faces) == 0
    c = np.clip(theta[:, 3:6].cpu().numpy() * np.float32(GM.SH_C0) + np.float32(0.5), 0, 1).astype(np.float64)
    assert np.array_equal(pcd.colors, np.floor(c * 255 + 0.5).astype(np.uint8))
    # the file is the map: loaded into a fresh GaussianMap it renders a keyframe to the same bits
    bg = torch.zeros(3, device=DEV)
    view = mapper.viewpoints[1]
    with torch.no_grad():
        before = GM.render(view, mapper.gaussians, bg)
    other = GM.GaussianMap(S.CONFIG["opt_params"], DEV)
    other.load_ply(os.path.join(out, "3dgs_final.ply"))
    assert torch.equal(_bits(other.theta), _bits(theta)) and other.steps == 0 and not other.m.any() and not other.denom.any()
    assert bool((other.kf_id == -1).all()) and other.kf_id.dtype == torch.int32 and other.m.shape == theta.shape
    with torch.no_grad():
        after = GM.render(view, other, bg)
    for k in ("render", "depth", "normal", "mask"):
        assert torch.equal(_bits(after[k]), _bits(before[k])), k
    # GaussianMap.save_ply is that writer; a file with f_rest belongs to GaussianCloud, and the error says so
    mapper.gaussians.save_ply(str(tmp_path / "again.ply"))
    assert open(str(tmp_path / "again.ply"), "rb").read() == open(os.path.join(out, "3dgs_final.ply"), "rb").read()
    _seeded_cloud(5).save_ply(str(tmp_path / "deg3.ply"))
    with pytest.raises(ValueError, match="GaussianCloud"):
        other.load_ply(str(tmp_path / "deg3.ply"))


def test_panels_are_written_only_with_viz_dir(mapper, tmp_path, monkeypatch):
    from PIL import Image
    monkeypatch.chdir(tmp_path)
    called = []
    monkeypatch.setattr(mapper, "viz", lambda *a, **k: called.append(a))
    assert mapper.viz_dir is None
    mapper.optimization(2, current_window=[0, 1])
    mapper.finalize(iteration_total=2)
    assert not called and os.listdir(str(tmp_path)) == []                  # nothing rendered, no file, no directory
    monkeypatch.undo()
    monkeypatch.setattr(mapper, "viz_dir", str(tmp_path / "viz"))
    mapper.optimization(2, current_window=[1])
    mapper.finalize(iteration_total=2)
    H, W = S.H, S.W
    assert sorted(os.listdir(str(tmp_path / "viz"))) == ["rendering", "rendering_final"]
    assert os.listdir(str(tmp_path / "viz" / "rendering")) == ["1_tstamp_10.jpg"]
    final = sorted(os.listdir(str(tmp_path / "viz" / "rendering_final")))
    assert final == ["0_tstamp_0.jpg", "1_tstamp_10.jpg"]                   # one per keyframe, the reference's file name
    for name in final:
        with Image.open(str(tmp_path / "viz" / "rendering_final" / name)) as im:
            assert im.size == (3 * W, 3 * H) and im.mode == "RGB"
    # the panel itself: a u8 device tensor whose first cell is the keyframe image and whose render cell is the rendering
    view = mapper.viewpoints[0]
    p = mapper.panel(view)
    assert p.is_cuda and p.dtype == torch.uint8 and tuple(p.shape) == (3 * H, 3 * W, 3)
    q = lambda img: torch.floor(img.double().clamp(0, 1) * 255 + 0.5).to(torch.uint8).permute(1, 2, 0)
    with torch.no_grad():
        pkg = GM.render(view, mapper.gaussians, mapper.background)
    assert torch.equal(p[:H, :W], q(view.original_image)) and torch.equal(p[:H, W:2 * W], q(pkg["render"]))


def _seeded_cloud(P=200, seed=0, device=DEV):
    """a degree-3 cloud around the origin with non-zero f_rest"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    feats = torch.cat([r(P, 1, 3), 0.3 * r(P, 15, 3)], 1)
    return gs_ply.GaussianCloud(0.5 * r(P, 3).to(device), feats, 1.0 + r(P, 1), torch.log(0.05 + 0.1 * torch.rand(P, 3, generator=g)), r(P, 4))


def _w2c_front():
    M = torch.eye(4)
    M[2, 3] = 3.0                                                          # the camera at (0, 0, -3) looks along +z
    return M


def _w2c_side():
    M = torch.eye(4)                                                       # the camera at (3, 0, 0) looks along -x
    M[:3, :3] = torch.tensor([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])
    M[2, 3] = 3.0
    return M


def test_render_cloud_round_trips_a_degree_3_file_and_is_view_dependent(tmp_path):
    H, W, K = 48, 64, (60.0, 60.0, 32.0, 24.0)
    cloud = _seeded_cloud()
    assert cloud.sh_degree == 3 and bool(cloud.features[:, 1:].abs().max() > 0)
    path = str(tmp_path / "deg3.ply")
    cloud.save_ply(path)
    loaded = gs_ply.GaussianCloud.from_ply(path, DEV)
    assert loaded.sh_degree == 3 and torch.equal(_bits(loaded.features), _bits(cloud.features))
    for w2c in (_w2c_front(), _w2c_side()):
        a, b = gs_view.render_cloud(cloud, w2c, K, H, W), gs_view.render_cloud(loaded, w2c, K, H, W)
        assert float(a["mask"].max()) > 0.5                                # the cloud is in view
        for k in ("render", "depth", "normal", "mask"):
            assert torch.equal(_bits(a[k]), _bits(b[k])), k
    # view dependence: ONE isotropic Gaussian at the origin, seen from two sides at the same distance, has the same footprint; its mean
    # colour differs with the higher SH bands and agrees without them (what gs_mapper.render's campos = 0 could not show)
    one = gs_ply.GaussianCloud(torch.zeros(1, 3, device=DEV), cloud.features[:1], torch.full((1, 1), 3.0), torch.full((1, 3), float(np.log(0.2))),
                               torch.tensor([[1.0, 0.0, 0.0, 0.0]]))
    flat = gs_ply.GaussianCloud(one.xyz, torch.cat([one.features[:, :1], torch.zeros(1, 15, 3, device=DEV)], 1), one.opacity, one.scaling, one.rotation)

    def mean_colour(c, w2c):
        pkg = gs_view.render_cloud(c, w2c, K, H, W)
        return pkg["render"].sum((1, 2)) / pkg["mask"].sum()
    assert float((mean_colour(flat, _w2c_front()) - mean_colour(flat, _w2c_side())).abs().max()) < 1e-4
    assert float((mean_colour(one, _w2c_front()) - mean_colour(one, _w2c_side())).abs().max()) > 1e-2


def test_command_line_writes_the_frames_of_the_in_process_call(tmp_path):
    from PIL import Image
    H, W, K = 24, 32, (30.0, 30.0, 16.0, 12.0)
    cloud = _seeded_cloud(seed=1)
    ply, traj, out = str(tmp_path / "map.ply"), str(tmp_path / "traj.txt"), str(tmp_path / "frames")
    cloud.save_ply(ply)
    rows = np.array([[0.0, 0.0, 0.0, -3.0, 0.0, 0.0, 0.0, 1.0], [1.0, 0.2, -0.1, -2.8, 0.0, 0.0342, 0.0, 0.9994]])      # t, c2w (t, q_xyzw)
    np.savetxt(traj, rows)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "cut3r_slam_amd.gs_view", ply, "--traj", traj, "--calib", " ".join(str(v) for v in K), "--size",
                        str(H), str(W), "--out", out, "--layers", "rgb", "depth", "normal"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(out)) == [f"{i:05d}_{layer}.png" for i in range(2) for layer in ("depth", "normal", "rgb")]
    from cut3r_slam_amd import views
    w2c = views.inverse44(views.tum_matrices(np.loadtxt(traj, ndmin=2)))
    loaded = gs_ply.GaussianCloud.from_ply(ply, DEV)
    for i in range(2):
        frames = gs_view.render_frames(loaded, w2c[i], K, H, W)
        assert float(frames["rgb"].float().max()) > 0                      # something is in view
        for layer, img in frames.items():
            with Image.open(os.path.join(out, f"{i:05d}_{layer}.png")) as im:
                assert np.array_equal(np.asarray(im), img.cpu().numpy()), (i, layer)
