"""GPU: LPIPS inside the rendering evaluation (GSMapper.eval_rendering / eval_rendering_kf, gaussian/utils/eval_utils.py:14-150), the command
line of cut3r_slam_amd.lpips and demo.py --lpips-weights.  Scene and helpers: tests/test_trajectory_fill_gpu.py (views of 96 x 128)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pytestmark = pytest.mark.gpu

from cut3r_slam_amd import gs_mapper as GM  # noqa: E402
from cut3r_slam_amd import lpips as LP  # noqa: E402
from tests import lpips_ref as LR  # noqa: E402
from tests import test_trajectory_fill_gpu as TF  # noqa: E402

DEV = TF.DEV


def _scene():
    """11 frames, keyframes at tstamps 0 and 6 with their own views in the mapper"""
    poses = [TF._pose7(0.01 * k, 0.0, 0.0, 0.0, -0.002 * k) for k in range(11)]
    obs = [TF._observe(TF._truth(), p) for p in poses]
    m = TF._mapper(True)
    for n, t in enumerate((0, 6)):
        m.viewpoints[n] = GM.Camera(n, obs[t][0], obs[t][1], TF._w2c(poses[t]), TF.FX, TF.FY, TF.CX, TF.CY, float(t), DEV)
    # the frames carry noise, so that rendering and frame differ and the metric has something to measure
    g = torch.Generator().manual_seed(0)
    images = {k: (o[0] + 0.1 * torch.randn(o[0].shape, generator=g).to(DEV)).clamp(0, 1) for k, o in enumerate(obs)}
    return m, images, poses


def _rendered(m, v):
    """the image that eval_rendering scores for view v: the public render, the view's exposure model, the clamp"""
    with torch.no_grad():
        pkg = GM.render(v, m.gaussians, m.background)
        A, b = v.exposure_a.detach(), v.exposure_b.detach()
        return torch.clamp((pkg["render"].permute(1, 2, 0) @ A + b).permute(2, 0, 1), 0.0, 1.0).contiguous()


def test_eval_rendering_reports_lpips(tmp_path):
    L = LP.LPIPS(LR.weights(), DEV)
    m, images, poses = _scene()
    traj = torch.stack(poses)
    res = m.eval_rendering(images, np.arange(11), traj, [0, 6], lpips=L, result_dir=str(tmp_path))
    rows = res["per_frame"]
    assert [r[0] for r in rows] == [0, 5, 6, 10] and all(len(r) == 4 and isinstance(r[3], float) for r in rows)
    assert res["mean_lpips"] == sum(r[3] for r in rows) / 4 and all(np.isfinite(r[3]) and r[3] >= 0 for r in rows)
    assert list(res) == ["mean_psnr", "mean_ssim", "mean_lpips", "mean_l1", "per_frame"]
    saved = json.load(open(tmp_path / "psnr" / "after_opt" / "final_result.json"))
    assert list(saved) == ["mean_psnr", "mean_ssim", "mean_lpips", "mean_l1"] and saved == {k: res[k] for k in saved}
    # a keyframe: the mapper's own view, scored against its own image
    kf = m.viewpoints[1]
    assert rows[2][3] == L(_rendered(m, kf), kf.original_image)
    # a non-keyframe: a camera at the trajectory's pose, scored against the frame
    v = GM.Camera(5, images[5], torch.zeros(TF.H, TF.W, device=DEV), TF._w2c(poses[5]), TF.FX, TF.FY, TF.CX, TF.CY, 5, DEV)
    assert rows[1][3] == L(_rendered(m, v), images[5]) and rows[1][3] > 0
    # without the object nothing changes
    plain = m.eval_rendering(images, np.arange(11), traj, [0, 6])
    assert "mean_lpips" not in plain and all(len(r) == 3 for r in plain["per_frame"])
    assert [r[:3] for r in rows] == plain["per_frame"]


def test_eval_rendering_kf_reports_lpips():
    L = LP.LPIPS(LR.weights(), DEV)
    m, _, _ = _scene()
    noisy = (m.viewpoints[1].original_image + 0.1 * torch.randn(3, TF.H, TF.W, device=DEV)).clamp(0, 1)
    m.viewpoints[1].original_image = noisy
    res = m.eval_rendering_kf(lpips=L)
    rows = res["per_view"]
    assert list(res) == ["mean_psnr", "mean_ssim", "mean_lpips", "per_view"] and [r[0] for r in rows] == [0, 1]
    assert all(len(r) == 4 for r in rows) and res["mean_lpips"] == (rows[0][3] + rows[1][3]) / 2
    for r in rows:
        v = m.viewpoints[r[0]]
        with torch.no_grad():
            img = torch.clamp(GM.render(v, m.gaussians, m.background)["render"], 0.0, 1.0)
        assert r[3] == L(img, v.original_image)
    assert rows[1][3] > rows[0][3] >= 0
    plain = m.eval_rendering_kf()
    assert "mean_lpips" not in plain and [r[:3] for r in rows] == plain["per_view"]


def test_views_too_small_for_lpips_are_refused_before_the_loop():
    L = LP.LPIPS(LR.weights(), DEV)
    m = TF._mapper(True)
    m.viewpoints[0] = GM.Camera(0, torch.zeros(3, 24, 48), torch.ones(24, 48), torch.eye(4, device=DEV), 40.0, 40.0, 24.0, 12.0, 0.0, DEV)
    with pytest.raises(ValueError, match="31x31"):
        m.eval_rendering({0: torch.zeros(3, 24, 48)}, [0], torch.tensor([[0, 0, 0, 0, 0, 0, 1.0]]), [0], lpips=L)
    with pytest.raises(ValueError, match="31x31"):
        m.eval_rendering_kf(lpips=L)


def test_command_line_equals_the_api(tmp_path, capsys):
    from PIL import Image
    from safetensors.torch import save_file
    g = np.random.default_rng(0)
    names = ["f2.png", "f10.png", "f1.png"]                          # natural order: f1, f2, f10
    for d in ("a", "b"):
        (tmp_path / d).mkdir()
        for n in names:
            Image.fromarray(g.integers(0, 256, (40, 56, 3), dtype=np.uint8)).save(tmp_path / d / n)
    wfile = tmp_path / "w.safetensors"
    save_file({k: v.contiguous() for k, v in LR.weights().items()}, str(wfile))
    rows = LP.main([str(tmp_path / "a"), str(tmp_path / "b"), "--weights", str(wfile)])
    assert [os.path.basename(r[0]) for r in rows] == ["f1.png", "f2.png", "f10.png"] == [os.path.basename(r[1]) for r in rows]
    L = LP.LPIPS(LR.weights(), DEV)
    read = lambda p: torch.from_numpy(np.array(Image.open(p).convert("RGB"))).to(DEV).permute(2, 0, 1).float() / 255.0
    want = [L(read(tmp_path / "a" / n), read(tmp_path / "b" / n)) for n in ("f1.png", "f2.png", "f10.png")]
    assert [r[2] for r in rows] == want and len(set(want)) == 3
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 4 and out[0] == f"f1.png f1.png {want[0]:.6f}" and out[3] == f"mean_lpips {sum(want) / 3:.6f}"
    one = LP.main([str(tmp_path / "a" / "f2.png"), str(tmp_path / "b" / "f2.png"), "--weights", str(wfile)])
    assert len(one) == 1 and one[0][2] == want[1]


def test_demo_reports_lpips(tmp_path):
    """demo.py --gs --fill --eval-render --lpips-weights F on the synthetic tiny configuration of tests/test_stream_gpu.py"""
    import demo
    from safetensors.torch import save_file
    from tests.test_stream_gpu import _write_sequence
    d = tmp_path / "colors"
    d.mkdir()
    _write_sequence(str(d), 24)
    calib = tmp_path / "calib.txt"
    calib.write_text("600.0 600.0 320.0 240.0")
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("""
Mapping: {itr_num: 2}
Training: {lambda_depth: 10.0, lambda_normal: 0.1, lambda_iso: 10.0, gaussian_th: 0.1, gaussian_extent: 1.0, size_threshold: 20, window_size: 4,
           compensate_exposure: true}
opt_params: {pose_lr: 0.0001, position_lr_init: 0.0005, feature_lr: 0.005, opacity_lr: 0.05, scaling_lr: 0.001, rotation_lr: 0.001, exposure_lr: 0.0005,
             percent_dense: 0.01, densify_grad_threshold: 0.0005}
""")
    wfile = tmp_path / "lpips.safetensors"
    save_file({k: v.contiguous() for k, v in LR.weights().items()}, str(wfile))
    out = tmp_path / "out"
    common = ["--imagedir", str(d), "--calib", str(calib), "--config", str(cfg), "--output", str(out), "--kf_every", "2", "--synthetic-weights",
              "--small", "--seed", "1"]
    with pytest.raises(SystemExit):
        demo.main(common + ["--lpips-weights", str(wfile)])                          # an error without --gs
    rc = demo.main(common + ["--gs", "--gs-final-iters", "20", "--fill", "--fill-iters", "2", "--eval-render", "--lpips-weights", str(wfile)])
    assert rc == 0
    saved = json.load(open(out / "psnr" / "after_opt" / "final_result.json"))
    assert list(saved) == ["mean_psnr", "mean_ssim", "mean_lpips", "mean_l1"]
    assert np.isfinite(saved["mean_lpips"]) and saved["mean_lpips"] > 0
