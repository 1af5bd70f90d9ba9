"""GSMapper.pose_estimator (hislam2/gs_backend_per_frame.py:123-177) on the tape-free trainer with cut3r_gs_pose_backward, against the
autograd formulation and the three-call backward; trajectory_filler.PoseTrajectoryFiller (util/trajectory_filler.py:88-114) and
GSMapper.eval_rendering (gaussian/utils/eval_utils.py:14-105).  Scene: the wall of tests/test_gs_mapper_gpu.py (96 x 128), the mapper's
Gaussians set to the truth, pose_lr = 0.0005."""
import json
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pytestmark = pytest.mark.gpu

from cut3r_slam_amd import gs_mapper as GM  # noqa: E402
from cut3r_slam_amd.lietorch import SE3  # noqa: E402
from cut3r_slam_amd.trajectory_filler import PoseTrajectoryFiller  # noqa: E402

DEV = "cuda:0"
H, W, FX, FY, CX, CY = 96, 128, 110.0, 110.0, 64.0, 48.0
CONFIG = {"Training": {"lambda_depth": 10.0, "lambda_normal": 0.1, "lambda_iso": 10.0, "gaussian_th": 0.05, "gaussian_extent": 1.0, "size_threshold": 20},
          "opt_params": {"pose_lr": 0.0005, "position_lr_init": 0.0005, "feature_lr": 0.005, "opacity_lr": 0.05, "scaling_lr": 0.001, "rotation_lr": 0.001,
                         "percent_dense": 0.01, "densify_grad_threshold": 0.0005}}
_TRUTH = []


def _truth():
    """tests/test_gs_mapper_gpu.py `_truth`, built once: 96 x 128 Gaussians on z = 3 + 0.2 sin(x) cos(1.3 y), colours a smooth texture
    (every test here leaves the map as it is: pose_estimator and eval_rendering freeze it)"""
    if _TRUTH:
        return _TRUTH[0]
    ys, xs = torch.meshgrid(torch.linspace(-1.6, 1.6, 96), torch.linspace(-2.2, 2.2, 128), indexing="ij")
    z = 3.0 + 0.2 * torch.sin(xs) * torch.cos(1.3 * ys)
    pts = torch.stack([xs, ys, z], -1).reshape(-1, 3)
    col = torch.stack([0.5 + 0.4 * torch.sin(3 * xs), 0.5 + 0.4 * torch.cos(2.5 * ys), 0.5 + 0.4 * torch.sin(2 * xs + 3 * ys)], -1).reshape(-1, 3)
    gm = GM.GaussianMap(CONFIG["opt_params"], DEV)
    gm.extend_from_pcd_seq(0, rgb=col, pointmap=pts)
    with torch.no_grad():
        gm.p["opacity"].fill_(float(GM.inverse_sigmoid(torch.tensor(0.9))))
        gm.p["scaling"] += math.log(1.3)
    _TRUTH.append(gm)
    return gm


def _pose7(tx, ty, tz, rx, ry):
    return SE3.exp(torch.tensor([[tx, ty, tz, rx, ry, 0.0]], device=DEV)).data[0].cpu()


def _w2c(pose7):
    return torch.inverse(GM.pose_vec_to_matrix(torch.as_tensor(pose7).float()[None].to(DEV))[0])


def _observe(truth, pose7):
    cam = GM.Camera(0, torch.zeros(3, H, W), torch.ones(H, W), _w2c(pose7), FX, FY, CX, CY, device=DEV)
    with torch.no_grad():
        pkg = GM.render(cam, truth, torch.zeros(3, device=DEV))
    assert float((pkg["mask"] > 0.9).float().mean()) > 0.95
    return pkg["render"].clamp(0, 1), pkg["depth"][0]


def _mapper(fused=True):
    m = GM.GSMapper(CONFIG, FX, FY, CX, CY, downsample_ratio=2, device=DEV)
    m.gaussians = _truth()
    m.fused = fused
    return m


def _pixel_shift(pose_a, pose_b):
    """mean displacement in pixels of the projected truth Gaussians between two camera->world poses"""
    x = _truth().get_xyz.detach()
    uv = []
    for p in (pose_a, pose_b):
        T = _w2c(p)
        c = x @ T[:3, :3].T + T[:3, 3]
        uv.append(torch.stack([FX * c[:, 0] / c[:, 2] + CX, FY * c[:, 1] / c[:, 2] + CY], -1))
    return float((uv[0] - uv[1]).norm(dim=-1).mean())


def test_five_iterations_agree_between_the_formulations():
    """fused (cut3r_gs_pose_backward), fused with the three-call backward, and autograd from the same start: the poses agree to 2e-5 (the
    bound of five unfused pose iterations at tests/test_gs_mapper_gpu.py:412), and they moved"""
    true_pose = _pose7(0.05, -0.03, 0.02, 0.01, -0.02)
    img, _ = _observe(_truth(), true_pose)
    start = _pose7(0.05 + 0.02, -0.03 - 0.015, 0.02 + 0.012, 0.01 + 0.005, -0.02 - 0.006)
    auto = _mapper(False).pose_estimator(start, img, 3, iters=5)
    fused = _mapper(True).pose_estimator(start, img, 3, iters=5)
    chain = _mapper(True).pose_estimator(start, img, 3, iters=5, pose_backward="chain")
    print(f"[fill] 5 iterations: max |fused - autograd| {float((fused - auto).abs().max()):.2e}, max |chain - autograd| "
          f"{float((chain - auto).abs().max()):.2e}, moved {float((auto - start).abs().max()):.2e}")
    assert auto.shape == (7,) and fused.dtype == torch.float32 and fused.device.type == "cpu"
    assert float((auto - start).abs().max()) > 1e-4 and float((fused - start).abs().max()) > 1e-4
    torch.testing.assert_close(fused, auto, atol=2e-5, rtol=0)
    torch.testing.assert_close(chain, auto, atol=2e-5, rtol=0)


def test_a_perturbed_pose_converges_on_both_formulations():
    """start off by 1 cm and 0.2 degrees (within 100 * pose_lr); after 100 iterations the mean pixel displacement to the true pose is below
    the start's on both formulations, and the two differ by at most 0.1 x the start's (the render backward's atomics)"""
    true_pose = _pose7(0.05, -0.03, 0.02, 0.01, -0.02)
    img, depth = _observe(_truth(), true_pose)
    start = _pose7(0.05 + 0.01, -0.03, 0.02, 0.01, -0.02 + math.radians(0.2))
    e0 = _pixel_shift(start, true_pose)
    fused = _mapper(True).pose_estimator(start, img, 0, iters=100)
    auto = _mapper(False).pose_estimator(start, img, 0, iters=100)
    ef, ea, d = _pixel_shift(fused, true_pose), _pixel_shift(auto, true_pose), _pixel_shift(fused, auto)
    print(f"[fill] 100 iterations: start {e0:.4f} px, fused {ef:.4f} px ({ef / e0:.3f}), autograd {ea:.4f} px ({ea / e0:.3f}), "
          f"fused vs autograd {d:.4f} px ({d / e0:.3f})")
    assert ef < e0 and ea < e0
    assert d <= 0.1 * e0
    # with the frame's depth the inverse-depth term joins the loss on both formulations
    fd = _mapper(True).pose_estimator(start, img, 0, gt_depth=depth, iters=5)
    ad = _mapper(False).pose_estimator(start, img, 0, gt_depth=depth, iters=5)
    torch.testing.assert_close(fd, ad, atol=2e-5, rtol=0)


def test_filler_beats_repeating_the_keyframe_pose():
    """9 frames 5 mm and 0.1 degrees apart, keyframes at tstamps 0, 4, 8 with their true poses"""
    poses = [_pose7(0.005 * k, 0.0, 0.0, math.radians(0.1) * k, 0.0) for k in range(9)]
    images = [_observe(_truth(), p)[0] for p in poses]
    kf_pose = torch.zeros(6, 7)
    kf_pose[:3] = torch.stack([poses[0], poses[4], poses[8]])
    kf = types.SimpleNamespace(counter=types.SimpleNamespace(value=4), tstamp=torch.tensor([0.0, 4.0, 8.0, 0.0, 0.0, 0.0]), pose=kf_pose)
    slam = types.SimpleNamespace(mapper=_mapper(True), keyframes=kf)
    ts, full = PoseTrajectoryFiller(slam).run(images, iters=100)
    assert ts.tolist() == list(range(9)) and full.shape == (9 - 0, 7)
    for row, k in ((0, 0), (4, 1), (8, 2)):
        assert np.array_equal(full[row], kf_pose[k].numpy())
    rest = [k for k in range(9) if k % 4]
    filled = np.mean([_pixel_shift(torch.as_tensor(full[k]), poses[k]) for k in rest])
    repeat = np.mean([_pixel_shift(poses[4 * (k // 4)], poses[k]) for k in rest])
    print(f"[fill] mean pixel displacement of the non-keyframes: filled {filled:.4f} px, preceding keyframe repeated {repeat:.4f} px")
    assert filled < repeat


def test_eval_rendering_scores_the_reference_frame_selection(tmp_path):
    """11 frames, keyframes {0, 6}: frames 0, 5, 6, 10 are scored; PSNR with the true trajectory beats every non-keyframe shifted by 2 cm;
    the depth L1 comes from the keyframes only (the other frames' GT depth files hold a constant that would give ~2 m)"""
    from PIL import Image
    poses = [_pose7(0.01 * k, 0.0, 0.0, 0.0, -0.002 * k) for k in range(11)]
    obs = [_observe(_truth(), p) for p in poses]
    images = {k: o[0] for k, o in enumerate(obs)}
    m = _mapper(True)
    for n, t in enumerate((0, 6)):
        m.viewpoints[n] = GM.Camera(n, obs[t][0], obs[t][1], _w2c(poses[t]), FX, FY, CX, CY, float(t), DEV)
    traj = torch.stack(poses)
    ddir = tmp_path / "depth"
    ddir.mkdir()
    for k in range(11):
        d = obs[k][1].cpu().numpy() if k in (0, 6) else np.ones((H, W), np.float32)
        Image.fromarray(np.clip(d * 6553.5, 0, 65535).astype(np.uint16)).save(ddir / f"depth{k:06d}.png")
    good = m.eval_rendering(images, np.arange(11), traj, [0, 6], gtdepthdir=str(ddir), out_dir=str(tmp_path / "good"))
    assert [r[0] for r in good["per_frame"]] == [0, 5, 6, 10] and "mean_lpips" not in good
    saved = json.load(open(tmp_path / "good" / "psnr" / "after_opt" / "final_result.json"))
    assert saved == {k: good[k] for k in ("mean_psnr", "mean_ssim", "mean_l1")}
    for k in (0, 5, 6, 10):
        assert (tmp_path / "good" / "renders" / "image_after_opt" / f"{k:06d}.jpg").is_file()
        png = np.asarray(Image.open(tmp_path / "good" / "renders" / "depth_after_opt" / f"{k:06d}.png"))
        assert png.shape == (H, W) and png.dtype == np.uint16 and png.max() > 6553
    assert not (tmp_path / "good" / "renders" / "image_after_opt" / "000001.jpg").exists()
    assert math.isfinite(good["mean_l1"]) and 0 <= good["mean_l1"] < 1e-3                 # keyframes only: the PNG's quantisation
    shifted = traj.clone()
    shifted[[k for k in range(11) if k not in (0, 6)], 0] += 0.02
    bad = m.eval_rendering(images, np.arange(11), shifted, [0, 6], result_dir=str(tmp_path / "bad"))
    print(f"[fill] eval_rendering: PSNR {good['mean_psnr']:.2f} dB / SSIM {good['mean_ssim']:.4f} with the true trajectory, "
          f"{bad['mean_psnr']:.2f} dB / {bad['mean_ssim']:.4f} with the non-keyframes shifted by 2 cm; depth L1 {good['mean_l1']:.2e}")
    assert good["mean_psnr"] > bad["mean_psnr"] and good["mean_ssim"] > bad["mean_ssim"]
    assert (tmp_path / "bad" / "psnr" / "after_opt" / "final_result.json").is_file() and not (tmp_path / "bad" / "renders").exists()
    assert bad["mean_l1"] == 0 and bad["per_frame"][0][1:] == pytest.approx(good["per_frame"][0][1:], abs=1e-3)      # keyframes: their own pose
