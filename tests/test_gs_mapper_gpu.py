"""GS mapper (cut3r_slam_amd/gs_mapper.py, mirrors hislam2/gs_backend_per_frame.py:87-121,202-326,451-587) on a synthetic scene: a
textured, gently curved wall modelled by ground-truth Gaussians, observed (image + depth) through the HIP rasteriser.  The reference's
backend cannot run here (CUDA rasteriser, open3d): functional tests, PARITY UNPINNED."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pytestmark = pytest.mark.gpu

from cut3r_slam_amd import gs_mapper as GM  # noqa: E402
from cut3r_slam_amd.lietorch import SE3  # noqa: E402

DEV = "cuda:0"
H, W, FX, FY, CX, CY = 96, 128, 110.0, 110.0, 64.0, 48.0
CONFIG = {"Training": {"lambda_depth": 10.0, "lambda_normal": 0.1, "lambda_iso": 10.0, "gaussian_th": 0.05, "gaussian_extent": 1.0, "size_threshold": 20},
          "opt_params": {"pose_lr": 0.0003, "position_lr_init": 0.0005, "feature_lr": 0.005, "opacity_lr": 0.05, "scaling_lr": 0.001, "rotation_lr": 0.001,
                         "percent_dense": 0.01, "densify_grad_threshold": 0.0005}}


def _truth():
    """ground-truth map: 96 x 128 Gaussians on z = 3 + 0.2 sin(x) cos(1.3 y), colours a smooth texture"""
    ys, xs = torch.meshgrid(torch.linspace(-1.6, 1.6, 96), torch.linspace(-2.2, 2.2, 128), indexing="ij")
    z = 3.0 + 0.2 * torch.sin(xs) * torch.cos(1.3 * ys)
    pts = torch.stack([xs, ys, z], -1).reshape(-1, 3)
    col = torch.stack([0.5 + 0.4 * torch.sin(3 * xs), 0.5 + 0.4 * torch.cos(2.5 * ys), 0.5 + 0.4 * torch.sin(2 * xs + 3 * ys)], -1).reshape(-1, 3)
    gm = GM.GaussianMap(CONFIG["opt_params"], DEV)
    gm.extend_from_pcd_seq(0, rgb=col, pointmap=pts)
    with torch.no_grad():
        gm.p["opacity"].fill_(float(GM.inverse_sigmoid(torch.tensor(0.9))))
        gm.p["scaling"] += math.log(1.3)
    return gm


def _pose7(tx, ty, tz, rx, ry):
    """camera->world [7] (t, q_xyzw) from a small translation and rotation"""
    return SE3.exp(torch.tensor([[tx, ty, tz, rx, ry, 0.0]], device=DEV)).data[0].cpu()


def _observe(truth, pose7):
    cam = GM.Camera(0, torch.zeros(3, H, W), torch.ones(H, W), torch.inverse(GM.pose_vec_to_matrix(pose7[None].to(DEV))[0]), FX, FY, CX, CY, device=DEV)
    with torch.no_grad():
        pkg = GM.render(cam, truth, torch.zeros(3, device=DEV))
    assert float((pkg["mask"] > 0.9).float().mean()) > 0.95                # the wall fills the view
    return pkg["render"].clamp(0, 1), pkg["depth"][0]


def _psnr(a, b):
    return float(-10 * torch.log10(((a - b) ** 2).mean()))


def test_render_geometry_is_a_pinhole_camera():
    """isolated Gaussians land where the REFERENCE's camera puts them: graphics_utils.getProjectionMatrix2 (P[0,2] = 2 cx / W - 1) through
    the rasteriser's ndc2Pix gives u = fx X/Z + cx - 0.5, v = fy Y/Z + cy - 0.5 (alpha centroid) -- also with an off-centre principal
    point and a moved camera; Camera.half_pixel_center = True (declared deviation, off by default) gives u = fx X/Z + cx exactly.  The
    rendered depth of the wall follows the analytic surface"""
    pts = torch.tensor([[0.3, -0.2, 2.0], [-0.8, 0.5, 3.0], [0.9, 0.6, 4.0]])
    gm = GM.GaussianMap(CONFIG["opt_params"], DEV)
    gm._append({"xyz": pts, "f_dc": torch.ones(3, 3), "opacity": torch.full((3, 1), 3.0), "scaling": torch.full((3, 3), math.log(0.03)),
                "rotation": torch.tensor([[1.0, 0, 0, 0]] * 3)}, torch.zeros(3))
    ys, xs = torch.meshgrid(torch.arange(H, device=DEV).float(), torch.arange(W, device=DEV).float(), indexing="ij")
    for cx, cy, pose, half in ((64.0, 48.0, _pose7(0, 0, 0, 0, 0), False), (70.25, 41.5, _pose7(0.1, -0.05, 0.2, 0.02, -0.03), False),
                               (70.25, 41.5, _pose7(0.1, -0.05, 0.2, 0.02, -0.03), True)):
        w2c = torch.inverse(GM.pose_vec_to_matrix(pose[None].to(DEV))[0])
        GM.Camera.half_pixel_center = half
        try:
            cam = GM.Camera(0, torch.zeros(3, H, W), torch.ones(H, W), w2c, FX, FY, cx, cy, device=DEV)
        finally:
            GM.Camera.half_pixel_center = False
        with torch.no_grad():
            alpha = GM.render(cam, gm, torch.zeros(3, device=DEV))["mask"][0]
        pc = pts.to(DEV) @ w2c[:3, :3].T + w2c[:3, 3]
        off = 0.0 if half else 0.5
        for k in range(3):
            u, v = FX * pc[k, 0] / pc[k, 2] + cx - off, FY * pc[k, 1] / pc[k, 2] + cy - off
            win = ((xs - u).abs() < 6) & ((ys - v).abs() < 6)
            a = alpha * win
            cu, cv = float((a * xs).sum() / a.sum()), float((a * ys).sum() / a.sum())
            assert abs(cu - float(u)) < 0.06 and abs(cv - float(v)) < 0.06, (k, cu, float(u), cv, float(v))
    truth = _truth()
    img, depth = _observe(truth, _pose7(0, 0, 0, 0, 0))
    X, Y = (xs - CX) / FX * depth, (ys - CY) / FY * depth
    z_expected = 3.0 + 0.2 * torch.sin(X) * torch.cos(1.3 * Y)
    err = (depth - z_expected).abs()[8:-8, 8:-8]
    print(f"[gs mapper] rendered depth vs analytic surface: median {float(err.median()):.4f} m, max {float(err.max()):.4f} m")
    assert float(err.median()) < 0.02 and float(err.max()) < 0.08      # (Gaussians of finite size on a slanted surface)


def test_pose_refine_recovers_a_perturbed_pose():
    truth = _truth()
    true_pose = _pose7(0.05, -0.03, 0.02, 0.01, -0.02)
    img, depth = _observe(truth, true_pose)
    mapper = GM.GSMapper(CONFIG, FX, FY, CX, CY, downsample_ratio=2, device=DEV)
    mapper.gaussians = truth
    start = _pose7(0.05 + 0.03, -0.03 - 0.02, 0.02 + 0.015, 0.01 + 0.006, -0.02 - 0.008)
    w2c0 = torch.inverse(GM.pose_vec_to_matrix(start[None].to(DEV))[0])
    mapper.viewpoints[0] = GM.Camera(0, img, depth, w2c0, FX, FY, CX, CY, device=DEV)
    T_true = GM.pose_vec_to_matrix(true_pose[None].to(DEV))[0]

    def err():
        d = torch.inverse(GM.get_pose(mapper.viewpoints[0])).detach() @ torch.inverse(T_true)
        ang = math.degrees(math.acos(max(-1.0, min(1.0, (float(d[:3, :3].trace()) - 1) / 2))))
        return float(d[:3, 3].norm()), ang
    t0, r0 = err()
    n_before = len(mapper.gaussians)
    pm, valid = mapper.pose_refine([0], iters=150)
    t1, r1 = err()
    print(f"[gs mapper] pose refine: translation error {100 * t0:.2f} -> {100 * t1:.2f} cm, rotation error {r0:.3f} -> {r1:.3f} deg")
    assert t1 < 0.35 * t0 and r1 < 0.35 * r0
    assert len(mapper.gaussians) == n_before and pm.shape == (1, H // 2, W // 2, 3) and valid.shape == (1, H // 2, W // 2)
    assert float(valid.mean()) < 0.05                                     # the map already covers the view: nothing to add


def test_mapping_from_keyframes_reaches_the_observations():
    truth = _truth()
    poses = [_pose7(0, 0, 0, 0, 0), _pose7(0.15, 0.0, 0.0, 0.0, -0.04), _pose7(-0.12, 0.08, 0.02, 0.03, 0.03)]
    obs = [_observe(truth, p) for p in poses]
    mapper = GM.GSMapper(CONFIG, FX, FY, CX, CY, downsample_ratio=2, device=DEV)
    g = torch.Generator().manual_seed(3)
    for k, (p, (img, depth)) in enumerate(zip(poses, obs)):
        noisy = depth.cpu() * (1 + 0.01 * torch.randn(H, W, generator=g))
        mapper.add_new_view((img * 255).round().to(torch.uint8), p, noisy.to(DEV), kf_sub_idx=k, iters=10)
    n0 = len(mapper.gaussians)
    assert n0 >= (H // 2) * (W // 2)                                       # the first keyframe seeds one Gaussian per stride-2 pixel
    bg = torch.zeros(3, device=DEV)
    with torch.no_grad():
        before = np.mean([_psnr(GM.render(mapper.viewpoints[k], mapper.gaussians, bg)["render"], obs[k][0]) for k in range(3)])
    first = mapper.optimization(1, optimize_pose=False, current_window=[0, 1, 2])
    last = mapper.optimization(80, optimize_pose=True, current_window=[0, 1, 2], densify=True)
    with torch.no_grad():
        pk = [GM.render(mapper.viewpoints[k], mapper.gaussians, bg) for k in range(3)]
        after = np.mean([_psnr(pk[k]["render"], obs[k][0]) for k in range(3)])
        derr = np.mean([float((pk[k]["depth"][0] - obs[k][1]).abs().median()) for k in range(3)])
    print(f"[gs mapper] mapping: {n0} -> {len(mapper.gaussians)} Gaussians, loss {first:.4f} -> {last:.4f}, PSNR {before:.2f} -> {after:.2f} dB, "
          f"median depth error {100 * derr:.2f} cm")
    assert last < 0.6 * first and after > before + 3.0 and after > 22.0 and derr < 0.05
    # global BA (one random keyframe per iteration, the rendered-normal terms, densification at half time): stays at the optimum
    n_before = len(mapper.gaussians)
    ba = mapper.global_BA(60, densify=True, densify_every=30, opacity_reset=False)
    with torch.no_grad():
        after_ba = np.mean([_psnr(GM.render(mapper.viewpoints[k], mapper.gaussians, bg)["render"], obs[k][0]) for k in range(3)])
    print(f"[gs mapper] global BA: loss {ba:.4f}, PSNR {after_ba:.2f} dB, {n_before} -> {len(mapper.gaussians)} Gaussians")
    assert ba is not None and np.isfinite(ba) and after_ba > after - 3.0
    assert mapper.global_pose_refine(iters=1) is not None
    # Gaussian re-training from the keyframes' pointmaps (gs_backend_per_frame.py:865-944): a fresh map reaches the observations again
    ys, xs = torch.meshgrid(torch.arange(H, device=DEV).float(), torch.arange(W, device=DEV).float(), indexing="ij")
    pms = []
    for k in range(3):
        d = obs[k][1]
        T = torch.inverse(GM.get_pose(mapper.viewpoints[k])).detach()
        pc = torch.stack([(xs - CX) / FX * d, (ys - CY) / FY * d, d], -1)
        pms.append(pc @ T[:3, :3].T + T[:3, 3])
    rgbs = torch.stack([(obs[k][0] * 255).round().to(torch.uint8) for k in range(3)])
    mapper.gaussian_reinit(rgbs, torch.stack(pms), iteration_total=150)
    ev2 = mapper.eval_rendering_kf()
    print(f"[gs mapper] re-training: {len(mapper.gaussians)} Gaussians, PSNR {ev2['mean_psnr']:.2f} dB")
    assert ev2["mean_psnr"] > 25.0
    traj = mapper.trajectory()
    assert traj.shape == (3, 4, 4) and torch.isfinite(traj).all()
    # evaluation and checkpoint round trip (gs_backend_per_frame.py:1088-1102)
    ev = mapper.eval_rendering_kf()
    assert ev["mean_psnr"] > 22.0 and 0.5 < ev["mean_ssim"] <= 1.0 and len(ev["per_view"]) == 3
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        mapper.save(os.path.join(d, "map.safetensors"))
        other = GM.GSMapper(CONFIG, FX, FY, CX, CY, downsample_ratio=2, device=DEV)
        other.load(os.path.join(d, "map.safetensors"))
    assert torch.equal(other.gaussians.theta.detach(), mapper.gaussians.theta.detach()) and torch.equal(other.gaussians.m, mapper.gaussians.m)
    other.viewpoints = mapper.viewpoints
    assert abs(other.eval_rendering_kf()["mean_psnr"] - ev["mean_psnr"]) < 1e-3


def test_tracker_hand_over_runs_the_mapper_and_writes_back():
    """Cut3rSlam.call_gs (hi2.py:56-91) with a keyframe store filled by hand: one 6-keyframe window of the synthetic wall with
    centimetre pose noise goes through GSMapper.run (gs_backend_per_frame.py:776-862); the store receives the refined poses,
    depths and stride-2 pointmaps"""
    from types import SimpleNamespace
    from cut3r_slam_amd.keyframe import KeyFrame
    from cut3r_slam_amd.slam import Cut3rSlam, DEFAULT_CONFIG
    truth = _truth()
    g = torch.Generator().manual_seed(8)
    true_poses = [_pose7(0.06 * k, 0.01 * (k % 2), 0.0, 0.0, -0.012 * k) for k in range(6)]
    kf = KeyFrame(DEFAULT_CONFIG, (H, W), 16, 2, DEV, feat_dim=8, patch=16)
    ys, xs = torch.meshgrid(torch.arange(H, device=DEV).float(), torch.arange(W, device=DEV).float(), indexing="ij")
    noisy = []
    for k, p in enumerate(true_poses):
        img, depth = _observe(truth, p)
        tw = torch.cat([torch.randn(3, generator=g) * 0.01, torch.randn(3, generator=g) * 0.002]) if k else torch.zeros(6)
        T = SE3.exp(tw[None].to(DEV)).matrix()[0] @ GM.pose_vec_to_matrix(p[None].to(DEV))[0]
        p_noisy = GM.SE3_from_matrix(T).cpu()
        noisy.append(p_noisy)
        kf.append(float(10 * k), (img * 255).round().to(torch.uint8), p_noisy.numpy(), None, depth, None, torch.tensor([FX, FY, CX, CY]))
        pts_c = torch.stack([(xs - CX) / FX * depth, (ys - CY) / FY * depth, depth], -1)
        kf.submap_ds[0, k] = (pts_c @ T[:3, :3].T + T[:3, 3])[::2, ::2]
        kf.conf_ds[0, k] = 1.0
    cfg = dict(CONFIG, Training=dict(CONFIG["Training"], window_size=10))
    mapper = GM.GSMapper(cfg, FX, FY, CX, CY, downsample_ratio=2, device=DEV)
    slam = SimpleNamespace(keyframes=kf, mapper=mapper, downsample_ratio=2)

    def terr(poses):
        e = []
        for k in range(1, 6):
            d = GM.pose_vec_to_matrix(torch.as_tensor(poses[k])[None].to(DEV))[0] @ torch.inverse(GM.pose_vec_to_matrix(true_poses[k][None].to(DEV))[0])
            e.append(float(d[:3, 3].norm()))
        return float(np.mean(e))
    before = terr(noisy)
    idx = Cut3rSlam.call_gs(slam, range(0, 6), 0, 20, torch.tensor([FX, FY, CX, CY]))
    after = terr([kf.pose[k] for k in range(6)])
    bg = torch.zeros(3, device=DEV)
    with torch.no_grad():
        psnr = np.mean([_psnr(GM.render(mapper.viewpoints[k], mapper.gaussians, bg)["render"], kf.image[k].float() / 255) for k in range(6)])
    print(f"[gs mapper] window hand-over: {len(mapper.gaussians)} Gaussians, mean translation error {100 * before:.2f} -> {100 * after:.2f} cm, "
          f"PSNR {psnr:.2f} dB")
    assert sorted(idx) == list(range(6)) and len(mapper.viewpoints) == 6
    assert after < 0.8 * before and psnr > 25.0          # (observed 0.28-0.45 of the initial error: the atomics of the backward pass make runs differ)
    w2c = torch.inverse(GM.pose_vec_to_matrix(kf.pose[3][None].to(DEV))[0])
    np.testing.assert_allclose(kf.w2c[3].cpu().numpy().reshape(3, 4), w2c[:3].cpu().numpy(), atol=2e-5)   # device mirror follows
    assert torch.isfinite(kf.submap_ds[0, :6]).all() and float((kf.depth[:6] > 0).float().mean()) > 0.95


def test_loop_closure_correction_moves_the_map_rigidly():
    """GSMapper.gaussain_update (gs_backend_per_frame.py:701-774): a rigid correction applied to every submap and every keyframe pose
    must leave every rendering unchanged -- positions, orientations of anisotropic Gaussians and camera poses move together.  The
    reference's quaternion-order mix-up (see the docstring) breaks exactly this for anisotropic Gaussians, which the test also shows."""
    truth = _truth()
    poses = [_pose7(0, 0, 0, 0, 0), _pose7(0.15, 0.0, 0.0, 0.0, -0.04), _pose7(-0.12, 0.08, 0.02, 0.03, 0.03)]
    obs = [_observe(truth, p) for p in poses]

    def build():
        m = GM.GSMapper(CONFIG, FX, FY, CX, CY, downsample_ratio=2, device=DEV)
        for k, (p, (img, depth)) in enumerate(zip(poses, obs)):
            m.add_new_view(img, p, depth, kf_sub_idx=k, iters=5)
        m.h, m.w = H // 2, W // 2
        g = torch.Generator().manual_seed(1)
        with torch.no_grad():                                              # make the Gaussians clearly anisotropic and randomly oriented
            m.gaussians.p["scaling"][:, 0] += math.log(2.5)
            q = torch.randn(len(m.gaussians), 4, generator=g).to(DEV)
            m.gaussians.p["rotation"].copy_(q / q.norm(dim=-1, keepdim=True))
        return m
    bg = torch.zeros(3, device=DEV)
    tw = torch.tensor([[0.3, -0.2, 0.1, 0.2, -0.3, 0.25]], device=DEV)
    T = SE3.exp(tw)
    results = {}
    for ref_order in (False, True):
        m = build()
        with torch.no_grad():
            before = [GM.render(m.viewpoints[k], m.gaussians, bg)["render"] for k in range(3)]
            xyz0 = m.gaussians.get_xyz.detach().clone()
        new_c2w = [T.matrix()[0] @ torch.inverse(GM.get_pose(m.viewpoints[k])).detach() for k in range(3)]
        packet = {"camera_idx": range(0, 3), "camera_pose": torch.stack([GM.SE3_from_matrix(c) for c in new_c2w]).cpu(),
                  "submap_idx": range(0, 3), "pose_updates": T.data.repeat(3, 1).cpu()}
        upd, idx = m.gaussain_update(packet, reference_quat_order=ref_order, refine_iters=0)      # (the re-refinement is tested elsewhere)
        with torch.no_grad():
            after = [GM.render(m.viewpoints[k], m.gaussians, bg)["render"] for k in range(3)]
        results[ref_order] = np.mean([_psnr(a, b) for a, b in zip(after, before)])
        assert idx == [0, 1, 2] and upd["poses"].shape == (3, 7) and upd["pointmaps"].shape == (3, H, W, 3)
        moved = (T.matrix()[0, :3, :3] @ xyz0.T).T + T.matrix()[0, :3, 3]
        np.testing.assert_allclose(m.gaussians.get_xyz.detach().cpu().numpy(), moved.cpu().numpy(), atol=2e-5)
    print(f"[gs mapper] rigid correction, rendering before vs after: {results[False]:.1f} dB (consistent quaternions), "
          f"{results[True]:.1f} dB (the reference's order)")
    assert results[False] > 40.0 and results[True] < results[False] - 10.0


def test_slam_loop_with_the_mapper_attached():
    """BASELINE config 5 in miniature (tracker + GS mapper, hi2.py:101-133): the per-frame loop with `slam.mapper` set hands every tracked
    window to the mapper and takes its poses / depths / pointmaps back.  Random weights give meaningless geometry, so this checks the
    plumbing (packet shapes of a real tracker, write-back, finite state), not quality."""
    from cut3r_slam_amd.config import tiny_config
    from cut3r_slam_amd.model import Cut3rModel
    from cut3r_slam_amd.slam import Cut3rSlam
    from cut3r_slam_amd.weights import synth_state_dict
    h, w, n = 32, 48, 40
    cfg = tiny_config("dpt")
    model = Cut3rModel(cfg, synth_state_dict(cfg, 3), DEV, minimal=True)
    cfgd = {"Tracking": {"motion_filter": {"thresh": 0.9, "skip": 1, "kf_every": 2}, "frontend": {"iteration": 0}}, "Mapping": {"itr_num": 5}}
    slam = Cut3rSlam(model, cfgd, (h, w), buffer=40, device=DEV)
    mcfg = dict(CONFIG, Training=dict(CONFIG["Training"], window_size=4))
    slam.mapper = GM.GSMapper(mcfg, 40.0, 40.0, 24.0, 16.0, downsample_ratio=2, device=DEV)
    g = torch.Generator().manual_seed(0)
    base = torch.nn.functional.avg_pool2d(torch.rand(3, h + 2 * n, w + 2 * n, generator=g)[None], 5, 1, 2)[0]
    base = (base - base.min()) / (base.max() - base.min())
    frames = torch.stack([(base[:, t:t + h, 2 * t % n:2 * t % n + w] * 255).round().to(torch.uint8) for t in range(n)]).to(DEV)
    intr = torch.tensor([40.0, 40.0, 24.0, 16.0])
    calls = []
    real_run = slam.mapper.run

    def spy(packet, iterations):
        calls.append((list(packet["viz_idx"]), tuple(packet["pointmaps"].shape), tuple(packet["depths"].shape)))
        return real_run(packet, iterations, init_iters=5, gba_per_view=1)
    slam.mapper.run = spy
    for t in range(n):
        slam.run(t, frames[t:t + 1], intr, frames[t:t + 1], intr, last_frame=(t == n - 1))
    nkf = slam.keyframes.counter.value
    assert len(calls) >= 3 and calls[0][1][1:] == (h // 2, w // 2, 3) and calls[0][2][1:] == (h, w)
    assert len(slam.mapper.viewpoints) >= 10 and len(slam.mapper.gaussians) > 100
    assert torch.isfinite(slam.keyframes.pose[:nkf - 1]).all() and torch.isfinite(slam.mapper.trajectory()).all()
    # hi2.py:152-229: closing global BA of the mapper, its poses written back into the keyframe table
    before = slam.keyframes.pose[:nkf - 1].clone()
    poses, _ = slam.terminate(add_kf=False, finalize_iters=12, gaussian_retrain=True, retrain_iters=8)
    assert np.isfinite(poses[:nkf - 1]).all() and not np.array_equal(poses[:nkf - 1], before.numpy())
    print(f"[gs mapper] slam loop: {nkf} keyframes, {len(calls)} windows handed over, {len(slam.mapper.viewpoints)} mapper views, "
          f"{len(slam.mapper.gaussians)} Gaussians")


def test_exposure_compensation_absorbs_a_gain_change():
    """Training.compensate_exposure (gs_backend_per_frame.py:467-475,513): a keyframe observed 15 % darker than the map is explained by
    its affine exposure parameters rather than by repainting the Gaussians"""
    truth = _truth()
    pose = _pose7(0, 0, 0, 0, 0)
    img, depth = _observe(truth, pose)
    cfg = dict(CONFIG, Training=dict(CONFIG["Training"], compensate_exposure=True), opt_params=dict(CONFIG["opt_params"], exposure_lr=0.01))
    mapper = GM.GSMapper(cfg, FX, FY, CX, CY, downsample_ratio=2, device=DEV)
    mapper.gaussians = truth
    w2c = torch.inverse(GM.pose_vec_to_matrix(pose[None].to(DEV))[0])
    mapper.viewpoints[0] = GM.Camera(0, 0.85 * img, depth, w2c, FX, FY, CX, CY, device=DEV)
    colours0 = truth.p["f_dc"].detach().clone()
    mapper.gaussians.lr[:, 3:6] = 0.0                                     # keep the map's colours fixed: only the exposure can explain the change
    first = mapper.optimization(1, optimize_pose=True, current_window=[0])
    last = mapper.optimization(60, optimize_pose=True, current_window=[0])
    gain = float(torch.diagonal(mapper.viewpoints[0].exposure_a.detach()).mean())
    print(f"[gs mapper] exposure: loss {first:.4f} -> {last:.4f}, mean diagonal gain {gain:.3f}")
    assert last < 0.7 * first and 0.8 < gain < 0.95
    assert torch.equal(truth.p["f_dc"].detach(), colours0)


def test_captured_iterations_follow_the_eager_loop():
    """GSMapper.optimization(graph=True): one iteration captured as a hipGraph and replayed (rasteriser in capacity mode) reaches the same
    loss and poses as the eager loop, within the noise of the atomics"""
    truth = _truth()
    poses = [_pose7(0, 0, 0, 0, 0), _pose7(0.15, 0.0, 0.0, 0.0, -0.04)]
    obs = [_observe(truth, p) for p in poses]
    res = {}
    for mode in (False, True):
        m = GM.GSMapper(CONFIG, FX, FY, CX, CY, downsample_ratio=2, device=DEV)
        g = torch.Generator().manual_seed(4)
        for k, (p, (img, depth)) in enumerate(zip(poses, obs)):
            m.add_new_view(img, p, depth.cpu().mul(1 + 0.01 * torch.randn(H, W, generator=g)).to(DEV), kf_sub_idx=k, iters=5)
        loss = m.optimization(40, optimize_pose=True, current_window=[0, 1], graph=mode)
        res[mode] = (loss, m.trajectory().cpu(), m.gaussians.theta.detach().cpu().clone(), m.use_graphs)
    print(f"[gs mapper] 40 iterations: eager loss {res[False][0]:.5f}, captured {res[True][0]:.5f}")
    assert abs(res[True][0] - res[False][0]) < 0.02 * res[False][0]
    torch.testing.assert_close(res[True][1], res[False][1], atol=2e-4, rtol=0)
    # (Adam with eps 1e-15 turns the last-bit noise of the atomics into +-lr steps on parameters whose gradient is ~0: compare in the mean)
    dth = (res[True][2] - res[False][2]).abs()
    print(f"[gs mapper] parameters, captured vs eager: mean |diff| {float(dth.mean()):.2e}, max {float(dth.max()):.2e}")
    assert float(dth.mean()) < 2e-3 and float(dth.max()) < 0.2      # (measured 0.5e-3 .. 1.0e-3 over runs: two separately built maps)


def _two_view_mapper(fused):
    truth = _truth()
    poses = [_pose7(0, 0, 0, 0, 0), _pose7(0.15, 0.0, 0.0, 0.0, -0.04)]
    obs = [_observe(truth, p) for p in poses]
    m = GM.GSMapper(CONFIG, FX, FY, CX, CY, downsample_ratio=2, device=DEV)
    m.fused = False                                   # identical set-up for both: the tensor-op path builds the map
    g = torch.Generator().manual_seed(4)
    for k, (p, (img, depth)) in enumerate(zip(poses, obs)):
        m.add_new_view(img, p, depth.cpu().mul(1 + 0.01 * torch.randn(H, W, generator=g)).to(DEV), kf_sub_idx=k, iters=5)
    m.fused = fused
    return m


def _pair():
    """two mappers in the SAME state (the set-up runs through atomics: two builds differ in the last bits), one per formulation"""
    a, b = _two_view_mapper(False), _two_view_mapper(True)
    ga, gb = a.gaussians, b.gaussians
    gb.theta = ga.theta.detach().clone().requires_grad_(True)
    gb.m, gb.v, gb.step_count, gb.steps = ga.m.clone(), ga.v.clone(), ga.step_count.clone(), ga.steps
    gb.kf_id, gb.max_radii2D, gb.grad_accum, gb.denom = ga.kf_id.clone(), ga.max_radii2D.clone(), ga.grad_accum.clone(), ga.denom.clone()
    for k in a.viewpoints:
        va, vb = a.viewpoints[k], b.viewpoints[k]
        vb.update_RT(va.R, va.T, data=va.w2c_data)
        vb.cam_rot_delta.data.copy_(va.cam_rot_delta.data)
        vb.cam_trans_delta.data.copy_(va.cam_trans_delta.data)
        vb.depth, vb.original_image = va.depth.clone(), va.original_image.clone()
    return a, b


def test_tape_free_trainer_matches_the_tensor_op_formulation():
    """gs_step.FusedTrainer (direct C-ABI calls: cut3r_gs_activate / _activate_backward / _pose_step / _adam around the rasteriser and loss
    kernels) against the autograd formulation of gs_mapper.py on the same map and views:
      * one mapping iteration over two views: the gradient of every Gaussian parameter (read from Adam's first moment, m = 0.1 g) and of
        both poses' increments agree to 1e-4 of their scale -- activations, isotropy term, SSIM + pixel losses, pose chain through exp();
      * five pose-refinement iterations (increments NOT folded between iterations: the exp() Jacobian away from 0, the pull to the start);
      * 40 mapping iterations: same loss and trajectory within the noise of the atomics (as the captured-graph test)."""
    a, b = _pair()
    assert torch.equal(a.gaussians.theta, b.gaussians.theta)
    pa0 = a.trajectory().detach().clone()
    la, lb = a.optimization(1, optimize_pose=True, current_window=[0, 1]), b.optimization(1, optimize_pose=True, current_window=[0, 1])
    ga, gb = a.gaussians.m / 0.1, b.gaussians.m / 0.1
    names = {"xyz": (0, 3), "colour": (3, 6), "opacity": (6, 7), "log scale": (7, 10), "quaternion": (10, 14)}
    for name, (c0, c1) in names.items():
        sc = float(ga[:, c0:c1].abs().max())
        err = float((ga[:, c0:c1] - gb[:, c0:c1]).abs().max())
        print(f"[gs fused] d loss / d {name}: scale {sc:.3e}, max |autograd - fused| {err:.3e}")
        assert sc > 0 and err <= 2e-4 * sc + 1e-9, (name, sc, err)
    assert abs(la - lb) <= 1e-5 * abs(la) + 1e-6, (la, lb)
    assert a.gaussians.steps == b.gaussians.steps == int(a.gaussians.step_count) and b.gaussians._steps_dev_stale
    # first Adam step of the poses: +-lr per component with the sign of the gradient -- the same move on both paths
    da, db = a.trajectory().detach() - pa0, b.trajectory().detach() - pa0
    assert float(da.abs().max()) > 1e-5
    torch.testing.assert_close(db, da, atol=1e-5, rtol=0)
    # ---- pose refinement: increments accumulate over the iterations
    a2, b2 = _pair()
    start = _pose7(0.15 + 0.02, 0.01, -0.015, 0.005, -0.04 - 0.006)
    for m in (a2, b2):
        m.viewpoints[1].update_RT(*(lambda T: (T[:3, :3], T[:3, 3]))(torch.inverse(GM.pose_vec_to_matrix(start[None].to(DEV))[0])))
        m.pose_refine([0, 1], iters=5, return_args=False)
    torch.testing.assert_close(b2.trajectory().detach(), a2.trajectory().detach(), atol=2e-5, rtol=0)
    assert float((a2.trajectory()[1].detach() - GM.pose_vec_to_matrix(start[None].to(DEV))[0]).abs().max()) > 1e-4       # (it moved)
    # ---- a real loop
    a3, b3 = _pair()
    l3a, l3b = a3.optimization(40, optimize_pose=True, current_window=[0, 1]), b3.optimization(40, optimize_pose=True, current_window=[0, 1])
    print(f"[gs fused] 40 iterations: autograd loss {l3a:.5f}, fused {l3b:.5f}")
    assert abs(l3a - l3b) < 0.02 * l3a
    torch.testing.assert_close(b3.trajectory().detach(), a3.trajectory().detach(), atol=2e-4, rtol=0)
    dth = (a3.gaussians.theta.detach() - b3.gaussians.theta.detach()).abs()
    assert float(dth.mean()) < 1e-3 and float(dth.max()) < 0.2
    # the autograd path picks the step count up again
    b3.fused = False
    b3.optimization(1, optimize_pose=False, current_window=[0])
    assert int(b3.gaussians.step_count) == b3.gaussians.steps and not b3.gaussians._steps_dev_stale


def test_tape_free_global_ba_matches_the_tensor_op_formulation():
    """GSMapper.global_BA on the tape-free trainer (rendered-normal term on cut3r_normal_agree_*, statistics on cut3r_gs_densify_stats)
    against the autograd formulation: one iteration -> the same gradient of every parameter (m = 0.1 g), the same densification
    statistics, the same loss; 30 iterations with a densification at half time -> the same number of Gaussians and close losses."""
    a, b = _pair()
    # (densify_every=None: with a number, a ONE-iteration run densifies at iteration 0 = iteration_total // 2 -- and, in the reference's order,
    #  an iteration that densifies takes no Adam step (gs_backend_per_frame.py:1025-1041: the re-created parameters have no gradient))
    la = a.global_BA(1, densify=True, densify_every=None, opacity_reset=False, seed=3)
    lb = b.global_BA(1, densify=True, densify_every=None, opacity_reset=False, seed=3)
    ga, gb = a.gaussians.m / 0.1, b.gaussians.m / 0.1
    for name, (c0, c1) in {"xyz": (0, 3), "colour": (3, 6), "opacity": (6, 7), "log scale": (7, 10)}.items():
        sc, err = float(ga[:, c0:c1].abs().max()), float((ga[:, c0:c1] - gb[:, c0:c1]).abs().max())
        print(f"[gs fused global BA] d loss / d {name}: scale {sc:.3e}, max |autograd - fused| {err:.3e}")
        assert sc > 0 and err <= 2e-4 * sc + 1e-9, (name, sc, err)
    assert abs(la - lb) <= 1e-5 * abs(la) + 1e-6, (la, lb)
    torch.testing.assert_close(b.gaussians.denom, a.gaussians.denom)
    torch.testing.assert_close(b.gaussians.max_radii2D, a.gaussians.max_radii2D)
    torch.testing.assert_close(b.gaussians.grad_accum, a.gaussians.grad_accum, rtol=1e-4, atol=1e-9)
    torch.testing.assert_close(b.trajectory().detach(), a.trajectory().detach(), atol=1e-5, rtol=0)
    a2, b2 = _pair()
    l2a = a2.global_BA(30, densify=True, densify_every=15, opacity_reset=False, seed=5)
    l2b = b2.global_BA(30, densify=True, densify_every=15, opacity_reset=False, seed=5)
    print(f"[gs fused global BA] 30 iterations: autograd loss {l2a:.5f} ({len(a2.gaussians)} Gaussians), fused {l2b:.5f} ({len(b2.gaussians)})")
    assert abs(len(a2.gaussians) - len(b2.gaussians)) <= 0.02 * len(a2.gaussians) + 2
    assert abs(l2a - l2b) < 0.03 * l2a


def test_an_overflowed_capacity_is_never_kept():
    """capacity mode (no instance-count read) must not change results: with a capacity that is far too small the tape-free trainer restores
    its snapshot and redoes the call with exact counts, and the captured-graph loop of the tensor-op formulation redoes its replays eagerly
    -- both end where the exact loops end (truncated tile lists used to stay applied)"""
    import warnings
    a, b = _pair()                                    # b: tape-free
    ref_pair = _pair()[1]
    ref_pair.gaussians.theta = b.gaussians.theta.detach().clone().requires_grad_(True)
    ref_pair.gaussians.m, ref_pair.gaussians.v = b.gaussians.m.clone(), b.gaussians.v.clone()
    for k in b.viewpoints:
        ref_pair.viewpoints[k].update_RT(b.viewpoints[k].R, b.viewpoints[k].T, data=b.viewpoints[k].w2c_data)
    b._fused_trainer().capacity = (0.0, 64)
    lb = b.optimization(6, optimize_pose=True, current_window=[0, 1])
    assert b._fused_trainer().redone == 1
    lr_ = ref_pair.optimization(6, optimize_pose=True, current_window=[0, 1])
    assert ref_pair._fused_trainer().redone == 0
    assert abs(lb - lr_) < 0.02 * lr_
    torch.testing.assert_close(b.trajectory().detach(), ref_pair.trajectory().detach(), atol=1e-4, rtol=0)
    assert b.gaussians.steps == ref_pair.gaussians.steps
    # tensor-op formulation, captured iterations
    c, _ = _pair()
    c.graph_capacity = (0.0, 64)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        lc = c.optimization(12, optimize_pose=True, current_window=[0, 1], graph=True)
    assert any("redone eagerly" in str(x.message) for x in w) and not c.use_graphs
    la = a.optimization(12, optimize_pose=True, current_window=[0, 1], graph=False)
    assert abs(lc - la) < 0.02 * la
    torch.testing.assert_close(c.trajectory().detach(), a.trajectory().detach(), atol=2e-4, rtol=0)
    assert int(c.gaussians.step_count) == int(a.gaussians.step_count) == c.gaussians.steps


@functools.lru_cache(maxsize=None)
def _host_scene():
    """a map and one observed camera built on the host (no atomics before the first launch): 160 Gaussians seen in 32 x 48 pixels ->
    (Hs, Ws, f, K, theta0 [P,14], w2c [4,4], gt_image [3,Hs,Ws], gt_depth [Hs,Ws]), all on the CPU; shared, not to be written to"""
    from oracle import gs_loss_oracle as LO
    Hs, Ws, f = 32, 48, 40.0
    K = (f, f, Ws / 2, Hs / 2)
    g = torch.Generator().manual_seed(21)
    P = 160
    xyz = torch.cat([(torch.rand(P, 2, generator=g) - 0.5) * torch.tensor([3.2, 2.2]), 2.5 + 1.5 * torch.rand(P, 1, generator=g)], 1)
    theta0 = torch.cat([xyz, torch.randn(P, 3, generator=g) * 0.8, torch.randn(P, 1, generator=g) * 0.8 + 0.5,
                        torch.log(0.05 + 0.12 * torch.rand(P, 3, generator=g)), torch.nn.functional.normalize(torch.randn(P, 4, generator=g), dim=-1)], 1)
    w2c = SE3.exp(torch.tensor([[0.05, -0.03, 0.04, 0.02, -0.03, 0.01]], device=DEV)).matrix()[0].cpu()
    # observations: a rendering of a perturbed copy of the map (so every loss term is active), depth with holes
    with torch.no_grad():
        pert = theta0.double().clone()
        pert[:, 0:3] += 0.05 * torch.randn(P, 3, generator=g).double()
        pert[:, 3:6] += 0.3 * torch.randn(P, 3, generator=g).double()
        obs = LO.render(pert, w2c.double(), torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64), Hs, Ws, K)
        gt_image = obs["color"].clamp(0, 1).float()
        gt_depth = (obs["depth"][0] * (1 + 0.02 * torch.randn(Hs, Ws, generator=g).double())).float()
        gt_depth[5:9, 10:20] = 0.0
    return Hs, Ws, f, K, theta0, w2c, gt_image, gt_depth


def test_one_mapping_iteration_matches_the_fp64_restatement_of_the_loss():
    """the WHOLE mapping iteration -- pose composition exp([tau, phi]) T, activations, rasteriser, colour L1 + SSIM, inverse-depth L1,
    depth-normal agreement, isotropy -- against oracle/gs_loss_oracle.py (fp64 torch autograd over the fp64 rasteriser restatement): the
    loss value and the gradient of every Gaussian parameter, for the tape-free trainer AND the tensor-op formulation; the first Adam step
    of the pose increments moves against the oracle's pose gradient.  Parity unpinned vs the reference (its CUDA rasteriser cannot run
    here): this pins the mapper's iteration to an independent reading of gs_backend_per_frame.py:451-587."""
    from oracle import gs_loss_oracle as LO
    Hs, Ws, f, K, theta0, w2c, gt_image, gt_depth = _host_scene()
    P = theta0.shape[0]
    cfg = dict(CONFIG, Training=dict(CONFIG["Training"], lambda_depth=2.0, lambda_normal=0.3, lambda_iso=4.0))
    res = {}
    for fused in (True, False):
        m = GM.GSMapper(cfg, f, f, Ws / 2, Hs / 2, downsample_ratio=2, device=DEV)
        m.fused = fused
        gm = m.gaussians
        gm._append({"xyz": theta0[:, 0:3], "f_dc": theta0[:, 3:6], "opacity": theta0[:, 6:7], "scaling": theta0[:, 7:10], "rotation": theta0[:, 10:14]},
                   torch.zeros(P))
        m.viewpoints[0] = GM.Camera(0, gt_image, gt_depth, w2c.to(DEV), f, f, Ws / 2, Hs / 2, device=DEV)
        loss = m.optimization(1, optimize_pose=True, current_window=[0])
        v = m.viewpoints[0]
        res[fused] = (loss, (gm.m / 0.1).cpu().double(), torch.inverse(GM.get_pose(v).detach()).cpu())
    # ---- the restatement
    th = theta0.double().clone().requires_grad_(True)
    tau, phi = torch.zeros(3, dtype=torch.float64, requires_grad=True), torch.zeros(3, dtype=torch.float64, requires_grad=True)
    ref = LO.mapping_loss(th, w2c.double(), tau, phi, gt_image.double(), gt_depth.double(), K, 2.0, 0.3, 4.0)
    ref.backward()
    ref = ref.detach()
    for fused, (loss, grad, _) in res.items():
        tag = "tape-free" if fused else "autograd"
        assert abs(loss - float(ref)) <= 2e-4 * abs(float(ref)), (tag, loss, float(ref))
        for name, (c0, c1) in {"xyz": (0, 3), "colour": (3, 6), "opacity": (6, 7), "log scale": (7, 10), "quaternion": (10, 14)}.items():
            gr = th.grad[:, c0:c1]
            sc = float(gr.abs().max())
            err = (grad[:, c0:c1] - gr).abs()
            bad = float((err > 2e-3 * sc + 1e-9).double().mean())
            print(f"[gs iteration vs fp64, {tag}] d loss / d {name}: scale {sc:.3e}, median |err| {float(err.median()):.2e}, max {float(err.max()):.2e}, "
                  f"beyond 2e-3 of the scale {100 * bad:.2f} %")
            assert float(err.median()) <= 2e-5 * sc + 1e-12 and bad <= 0.02, (tag, name, sc, float(err.max()), bad)
    # ---- poses: one Adam step = -lr * sign(gradient) per component: compare with the oracle's pose gradient
    lr = cfg["opt_params"]["pose_lr"]
    Tn = torch.inverse(res[True][2].double())                                    # new world->camera = exp(delta) T
    D = Tn @ torch.inverse(w2c.double())
    d_tau, d_phi = D[:3, 3], torch.stack([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]]) / 2
    for got, gref, step in ((d_tau, tau.grad, 10 * lr), (d_phi, phi.grad, 2 * lr)):
        big = gref.abs() > 1e-3 * gref.abs().max()
        assert bool((torch.sign(got[big]) == -torch.sign(gref[big])).all()), (got, gref)
        assert float((got[big].abs() - step).abs().max()) < 0.05 * step, (got, step)
    torch.testing.assert_close(res[True][2], res[False][2], atol=1e-6, rtol=0)


def test_tape_free_reinit_loop_matches_the_tensor_op_formulation():
    """GSMapper._reinit_loop (the training loop of gaussian_reinit, on a prepared map) on the tape-free trainer against the autograd
    formulation: one iteration -> the same gradient of every parameter (m = 0.1 g) and the same loss; reinit fixes the poses, so both
    sides leave them where they were"""
    a, b = _pair()
    a.fused, b.fused = False, True
    pa0, pb0 = a.trajectory().detach().clone(), b.trajectory().detach().clone()
    la, lb = a._reinit_loop(1, seed=3), b._reinit_loop(1, seed=3)
    ga, gb = a.gaussians.m / 0.1, b.gaussians.m / 0.1
    for name, (c0, c1) in {"xyz": (0, 3), "colour": (3, 6), "opacity": (6, 7), "log scale": (7, 10)}.items():
        sc, err = float(ga[:, c0:c1].abs().max()), float((ga[:, c0:c1] - gb[:, c0:c1]).abs().max())
        print(f"[gs fused reinit] d loss / d {name}: scale {sc:.3e}, max |autograd - fused| {err:.3e}")
        assert sc > 0 and err <= 2e-4 * sc + 1e-9, (name, sc, err)
    print(f"[gs fused reinit] loss: autograd {la!r}, fused {lb!r}")
    assert abs(la - lb) <= 1e-5 * abs(la) + 1e-6, (la, lb)
    assert torch.equal(a.trajectory().detach(), pa0) and torch.equal(b.trajectory().detach(), pb0)
    for m in (a, b):
        for v in m.viewpoints.values():
            assert not bool(v.cam_trans_delta.any()) and not bool(v.cam_rot_delta.any())


class _Recorder:
    """stands in for FusedTrainer.lib: every entry point looked up is wrapped to note its name (without the cut3r_ prefix), then forwards"""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.names.append(name[len("cut3r_"):])
            return fn(*args)
        return call


def _two_camera_mapper():
    """the host-built scene of _host_scene under two cameras, the second a few centimetres off the first, on a tape-free mapper whose
    trainer's library is a _Recorder -> (mapper, trainer, views)"""
    Hs, Ws, f, K, theta0, w2c, gt_image, gt_depth = _host_scene()
    m = GM.GSMapper(CONFIG, f, f, Ws / 2, Hs / 2, downsample_ratio=2, device=DEV)
    m.gaussians._append({"xyz": theta0[:, 0:3], "f_dc": theta0[:, 3:6], "opacity": theta0[:, 6:7], "scaling": theta0[:, 7:10], "rotation": theta0[:, 10:14]},
                        torch.zeros(theta0.shape[0]))
    off = SE3.exp(torch.tensor([[0.03, -0.02, 0.01, 0.0, 0.0, 0.0]], device=DEV)).matrix()[0].cpu()
    for k, T in enumerate((w2c, off @ w2c)):
        m.viewpoints[k] = GM.Camera(k, gt_image, gt_depth, T.to(DEV), f, f, Ws / 2, Hs / 2, device=DEV)
    tr = m._fused_trainer()
    tr.lib = _Recorder(tr.lib)
    return m, tr, list(m.viewpoints.values())


def test_the_tape_free_loops_launch_what_they_always_launched():
    """the C-ABI entry points every FusedTrainer loop calls, in order, on two host-built cameras (no atomics in the set-up): pinned
    to the trace recorded before the loops were put on shared helpers (one colour block, one Adam step, one rasteriser backward), so a
    change to a helper that adds, drops or reorders a launch in ANY loop shows here"""
    render = ["gs_activate", "gs_preprocess", "gs_bin", "gs_render_forward"]
    colour = ["pixel_loss_forward", "gs_map_coef", "pixel_loss_backward", "ssim_forward", "ssim_backward"]
    backward = ["gs_render_backward", "gs_preprocess_backward", "gs_activate_backward"]
    view = render + colour + backward
    view_x = render + ["exposure_forward"] + colour + ["exposure_backward"] + backward
    view_refine = render + ["refine_loss_forward", "gs_refine_coef", "refine_loss_backward"] + backward

    def trace(call):
        m, tr, views = _two_camera_mapper()
        call(m, tr, views)
        torch.cuda.synchronize()
        return tr.lib.names

    # optimization: per iteration both views, then ONE Adam step and a pose step per view; iteration 1 runs in capacity mode (same launches)
    iteration = view + view + ["gs_adam", "gs_pose_step", "gs_pose_step"]
    assert trace(lambda m, tr, views: tr.optimization(views, 2, True)) == ["exposure_partial_rows"] + iteration + iteration
    iteration_x = view_x + view_x + ["gs_adam", "gs_pose_step", "gs_pose_step", "gs_exposure_step", "gs_exposure_step"]
    assert trace(lambda m, tr, views: tr.optimization(views, 2, True, exposure=True)) == ["exposure_partial_rows"] + iteration_x + iteration_x
    # pose_refine: a pose step per view after the views, and the fold of the increments after the loop
    assert trace(lambda m, tr, views: tr.pose_refine(views, 1)) == view_refine + view_refine + ["gs_pose_step"] * 2 + ["gs_pose_step"] * 2
    # pose_estimator: dgeom straight to the pose sums, or the three-call chain
    assert trace(lambda m, tr, views: tr.pose_estimator(views[0], 1)) == (
        ["gs_pose_partial_rows"] + render + colour + ["gs_render_backward", "gs_pose_backward"] + ["gs_pose_step"])
    assert trace(lambda m, tr, views: tr.pose_estimator(views[0], 1, pose_backward="chain")) == ["gs_pose_partial_rows"] + view + ["gs_pose_step"]
    # global_BA: one drawn view, the rendered-normal term (its value in the last iteration only) before the backward pass
    assert trace(lambda m, tr, views: tr.global_BA(1, densify=True, densify_every=None, opacity_reset=False, seed=3)) == (
        ["exposure_partial_rows"] + render + colour + ["normal_agree_forward", "normal_agree_backward"] + backward
        + ["gs_densify_stats", "gs_adam", "gs_pose_step"])
    # reinit_loop: one drawn view, fixed poses
    assert trace(lambda m, tr, views: tr.reinit_loop(1, seed=3)) == view + ["gs_adam"]
