"""GPU: loop closure over sim(3) end to end -- the fused optimiser on the scale-drift scenario against its fp64 restatement
(tests/lc_sim3_oracle.py), three successive closures through TrackBackend.close_loop in loop_group = "sim3" mode (rigid poses, rescaled
depth maps, Sim3 pose_updates), and the Gaussian mapper's hand-over (GSMapper.gaussain_update with 8-wide packets).  The mode has no
counterpart in the reference; tolerances are those tests/test_loop_closure_gpu.py and tests/test_gs_mapper_gpu.py use for the rigid mode."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cut3r_slam_amd import geom_host as gh  # noqa: E402
from cut3r_slam_amd import ops  # noqa: E402
from cut3r_slam_amd.lietorch import SE3, Sim3  # noqa: E402
from tests import lc_sim3_oracle as Q  # noqa: E402

DEV = "cuda:0"
LR = 5e-4
U = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ the optimiser on a planted scale drift
def test_sim3_optimiser_closes_a_scale_drift_like_the_fp64_run():
    """lc_sim3_oracle.drift_scenario (B = 5, N = 257, noise 5 mm, scale 1.1 at the loop), 2000 iterations at lr 5e-4 from zero through
    ops.lc_optimize(group="sim3") against the fp64 autograd run; and against the se(3) optimiser on the same inputs"""
    iters = 2000
    sub, mask, cur, cur_lc, sA = Q.drift_scenario()
    xi_ref, T_ref, losses = Q.loop_closure_init(sub, mask, cur, cur_lc, iters, K=7)
    args = (sub.to(DEV), mask.to(DEV), cur.to(DEV), cur_lc.to(DEV), iters, LR)
    xi, T, loss = ops.lc_optimize(*args, return_loss=True, group="sim3")
    xi6, T6, loss6 = ops.lc_optimize(*args, return_loss=True)
    torch.cuda.synchronize()
    loss, loss6 = loss.cpu().numpy(), loss6.cpu().numpy()
    assert xi.shape == (5, 7) and T.shape == (5, 3, 4) and xi6.shape == (5, 6)
    assert abs(loss[0] - losses[0]) < 1e-5 * max(1.0, losses[0]) and loss[0] == loss6[0]
    np.testing.assert_allclose(loss, np.asarray(losses), rtol=2e-2, atol=1e-3)
    np.testing.assert_allclose(xi.cpu().numpy(), xi_ref.numpy(), atol=6 * LR)
    np.testing.assert_allclose(T.cpu().numpy(), T_ref[:, :3, :4].numpy(), atol=5e-3)
    s = Q.scale_of(T.cpu().double())
    rel = float((s * sA - 1).abs().max())
    print(f"\n[lc sim3] GPU: final loss sim3 {loss[-1]:.4f} = {loss[-1] / loss6[-1]:.3f} x se3 {loss6[-1]:.4f} (fp64 sim3 {losses[-1]:.4f}); "
          f"recovered scales within {rel:.2e}")
    assert loss[-1] <= 0.25 * loss6[-1]
    assert rel <= 2e-3
    assert not xi[0].any() and torch.equal(T[0].cpu(), torch.eye(4)[:3])


def test_unknown_group_is_refused():
    with pytest.raises(ValueError):
        ops.lc_optimize(torch.zeros(2, 6, 1, 4, 3, device=DEV), None, torch.zeros(4, 3, device=DEV), torch.zeros(4, 3, device=DEV), 1, group="so3")


# ------------------------------------------------------------------------------------------------ three closures through the backend
def _rigid(A, P):
    """similarity A [4,4] on a rigid camera-to-world P [4,4], kept rigid (fp64 torch)"""
    s = Q.scale_of(A)
    out = torch.eye(4, dtype=torch.float64)
    out[:3, :3] = (A[:3, :3] / s) @ P[:3, :3]
    out[:3, 3] = A[:3, :3] @ P[:3, 3] + A[:3, 3]
    return out


def _scale_drifting_store(S, h, w, seed):
    """A keyframe store of S submaps whose frames carry a similarity drift A_b (stored = A_b(true); scale growing to ~1.06), built so that
    for every keyframe the camera-frame z of its stride-2 stored pointmap equals depth[::2, ::2]:  keyframe k = 5 b + s has a true pose P_k
    and camera-frame points (x, y, depth_k[::2, ::2]); submap b holds A_b P_k(points) in slot s and A_b P_{5(b+1)}(points) in slot 5, the
    store's pose is A_b P_k made rigid, its depth scale(A_b) depth_k."""
    from scipy.spatial.transform import Rotation
    g = torch.Generator().manual_seed(seed)
    K = S * 5 + 6
    drift = torch.zeros(S, 7, dtype=torch.float64)
    drift[1:, :6] = torch.randn(S - 1, 6, generator=g, dtype=torch.float64) * 0.01
    drift[1:, 6] = 0.01 * torch.arange(1, S, dtype=torch.float64)
    A = Q.matrix7(drift)
    sA = Q.scale_of(A)
    depth = 1.5 + 3.0 * torch.rand(K, 2 * h, 2 * w, generator=g, dtype=torch.float64)
    P, X = [], []
    for k in range(K):
        tw = torch.randn(1, 6, generator=g, dtype=torch.float64) * torch.tensor([0.5, 0.5, 0.5, 0.2, 0.2, 0.2], dtype=torch.float64)
        Pk = torch.matrix_exp(Q.LO.twist(tw))[0]
        cam = torch.randn(h, w, 3, generator=g, dtype=torch.float64)
        cam[..., 2] = depth[k, ::2, ::2]
        P.append(Pk)
        X.append(cam @ Pk[:3, :3].T + Pk[:3, 3])
    sub = torch.empty(S, 6, h, w, 3, dtype=torch.float64)
    pose = torch.zeros(K, 7, dtype=torch.float64)
    for k in range(K):
        b = min(k // 5, S - 1)
        Pr = _rigid(A[b], P[k])
        pose[k] = torch.cat([Pr[:3, 3], torch.from_numpy(Rotation.from_matrix(Pr[:3, :3].numpy()).as_quat())])
        depth[k] = depth[k] * sA[b]
    for b in range(S):
        for s in range(6):
            sub[b, s] = X[5 * b + s] @ A[b, :3, :3].T + A[b, :3, 3]
    conf = torch.rand(S, 6, h, w, generator=g) - 0.08
    return sub.float(), conf, pose.float(), depth.float(), A


def _cam_z(pm, pose7):
    """camera-frame z of the points pm [h,w,3] under the camera-to-world pose (t, q_xyzw), fp64 from the stored fp32 values"""
    c2w = gh.pose_vec_to_matrix(np.asarray(pose7, np.float32)[None])[0].astype(np.float64)
    p = pm.double().numpy().reshape(-1, 3) - c2w[:3, 3]
    return torch.from_numpy(p @ c2w[:3, 2]).reshape(pm.shape[:2])


def test_three_successive_closures_in_sim3_mode_match_fp64_restatement():
    """TrackBackend.close_loop x3 with loop_group = "sim3" vs lc_sim3_oracle.LoopCloserSim3 (fp64): submaps, positions, orientations, depth
    maps and the stored lc submaps after every closure; every stored pose a unit quaternion with an orthonormal world->camera row block;
    e = (camera-frame z of the stride-2 pointmap) - depth[::2, ::2] of every rewritten keyframe becomes s e, to fp32 rounding of the products
    involved (64 x 2^-24 x (|p| + |c| + depth): an unscaled depth or a non-rigid pose would miss by (s - 1) x depth ~ 1e-2); everything
    outside the rewritten range bit-identical; pose_updates [m,8]."""
    from cut3r_slam_amd.config import tiny_config
    from cut3r_slam_amd.model import Cut3rModel
    from cut3r_slam_amd.slam import Cut3rSlam
    from cut3r_slam_amd.weights import synth_state_dict
    S, h, w, iters = 7, 16, 24, 150
    cfg = tiny_config("dpt")
    model = Cut3rModel(cfg, synth_state_dict(cfg, 3), DEV, minimal=True)
    conf_d = {"Tracking": {"motion_filter": {"thresh": 0.9, "skip": 1, "kf_every": 2}, "frontend": {"iteration": iters, "loop_group": "sim3"}}}
    slam = Cut3rSlam(model, conf_d, (2 * h, 2 * w), buffer=S * 5 + 8, device=DEV)
    sub, conf, pose, depth, A = _scale_drifting_store(S, h, w, 5)
    K = S * 5 + 6
    kf = slam.keyframes
    kf.submap_ds[:S] = sub.to(DEV)
    kf.conf_ds[:S] = conf.to(DEV)
    kf.depth[:K] = depth.to(DEV)
    kf.set_poses(0, pose.numpy())
    kf.counter.value = K
    # the store is consistent to begin with
    for k in range(S * 5):
        assert float((_cam_z(sub[k // 5, k % 5], pose[k]) - depth[k, ::2, ::2].double()).abs().max()) < 64 * U * 10
    ref = Q.LoopCloserSim3(sub.clone(), conf.clone(), pose.clone(), depth.clone(), iters)
    be = slam.backend
    assert be.loop_group == "sim3"
    g = torch.Generator().manual_seed(9)
    Ai = torch.inverse(A).float()
    loops = [(3 * 5 + 2, 0 * 5 + 1), (5 * 5 + 1, 1 * 5 + 3), (6 * 5 + 3, 2 * 5 + 2)]
    for n, (idx_cur, idx_m) in enumerate(loops):
        sc, sm = idx_cur // 5, idx_m // 5
        B = sc + 1
        R = B * 5 + 1                                                     # rewritten keyframes
        pm_lc = kf.submap_ds[sm].clone().cpu()
        cur_true = kf.submap_ds[sc, idx_cur % 5].cpu().reshape(-1, 3) @ Ai[sc, :3, :3].T + Ai[sc, :3, 3]
        pm_lc[5] = (cur_true + 0.002 * torch.randn(h * w, 3, generator=g)).reshape(h, w, 3)
        pm_lc = pm_lc + 0.001 * torch.randn(pm_lc.shape, generator=g)
        sub0, pose0, depth0 = kf.submap_ds[:S].cpu().clone(), kf.pose[:K].clone(), kf.depth[:K].cpu().clone()
        xi_ref = ref.close(pm_lc.clone(), idx_m, idx_cur)
        upd = be.close_loop(pm_lc.to(DEV), idx_m, idx_cur)
        torch.cuda.synchronize()
        assert tuple(upd["pose_updates"].shape) == (B, 8) and tuple(upd["camera_pose"].shape) == (R, 7)
        lg = Sim3(upd["pose_updates"]).log().cpu().numpy()
        np.testing.assert_allclose(lg[:, :3], xi_ref.numpy()[:B, :3], atol=8 * LR, err_msg=f"loop {n}: tau")
        np.testing.assert_allclose(lg[:, 6], xi_ref.numpy()[:B, 6], atol=8 * LR, err_msg=f"loop {n}: sigma")
        np.testing.assert_allclose(kf.submap_ds[:B].cpu().numpy(), ref.sub[:B].numpy(), atol=2e-2, err_msg=f"loop {n}: submaps")
        np.testing.assert_allclose(kf.pose[:R, :3].numpy(), ref.pose[:R, :3].numpy(), atol=2e-2, err_msg=f"loop {n}: positions")
        qa, qb = kf.pose[:R, 3:].numpy(), ref.pose[:R, 3:].numpy()
        assert np.abs(np.abs((qa * qb).sum(1)) - 1).max() < 1e-4, f"loop {n}: orientations"
        np.testing.assert_allclose(kf.depth[:R].cpu().numpy(), ref.depth[:R].numpy(), atol=2e-2, err_msg=f"loop {n}: depth maps")
        assert len(be.closed_loop["pointmaps_lc"]) == n + 1
        for k in range(n + 1):
            np.testing.assert_allclose(be.closed_loop["pointmaps_lc"][k].cpu().numpy(), ref.closed["pointmaps_lc"][k].numpy(), atol=2e-2,
                                       err_msg=f"loop {n}: stored lc submap {k}")
        # rigid, unit-quaternion poses
        assert np.abs(np.linalg.norm(qa, axis=1) - 1).max() < 1e-6
        Rw = kf.w2c[:R].cpu().double().reshape(R, 3, 4)[:, :, :3]
        assert float((Rw @ Rw.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-5
        # pointmap / depth / pose consistency moves with the similarity: e' = s e
        sT = upd["pose_updates"][:, 7].cpu().double()
        T34 = Sim3(upd["pose_updates"]).matrix().cpu().double()
        d_now, sub_now = kf.depth[:R].cpu(), kf.submap_ds[:S].cpu()
        worst = 0.0
        for k in range(R):
            b = min(k // 5, B - 1)
            if k < 5 * B:
                p_old, p_new = sub0[k // 5, k % 5], sub_now[k // 5, k % 5]
            else:                                                         # the shared last keyframe: its own map lies beyond the block
                p_old = sub0[B, 0] if B < S else sub0[B - 1, 5]
                p_new = (p_old.double() @ T34[b, :3, :3].T + T34[b, :3, 3]).float()
            e0 = _cam_z(p_old, pose0[k]) - depth0[k, ::2, ::2].double()
            e1 = _cam_z(p_new, kf.pose[k]) - d_now[k, ::2, ::2].double()
            c = float(kf.pose[k, :3].abs().max())
            bound = 64 * U * (float(p_new.abs().max()) + c + float(d_now[k].max()))
            worst = max(worst, float((e1 - sT[b] * e0).abs().max()) / bound)
        print(f"\n[lc sim3] loop {n}: scales {[round(float(x), 4) for x in sT]}, consistency {worst:.3f} of the fp32 bound")
        assert worst <= 1, f"loop {n}: pointmap / depth / pose consistency off by {worst:.2f} x the fp32 bound"
        # untouched keyframes and later submaps stay bit-identical
        assert torch.equal(kf.depth[R:K].cpu(), depth[R:K]) and torch.equal(kf.pose[R:K], pose[R:K])
        assert torch.equal(kf.submap_ds[B:S].cpu(), sub[B:S])
    assert be.closed_loop["idx_current"] == [c for c, _ in loops] and be.closed_loop["idx_matched"] == [m for _, m in loops]


# ------------------------------------------------------------------------------------------------ the mapper's hand-over
@pytest.mark.parametrize("s", [1.25, 0.8])
def test_similarity_correction_moves_the_map_and_scales_depth(s):
    """GSMapper.gaussain_update with Sim3 pose_updates [m,8]: a similarity applied to every submap and every camera (kept rigid) leaves every
    colour rendering unchanged (40 dB, the rigid test's threshold), multiplies the rendered depth by s (the same 40 dB on depth / s),
    moves the positions to s R x + t, the log-scales by exactly log s and the viewpoints' depths by s; a 7-wide packet takes the old path."""
    from cut3r_slam_amd import gs_mapper as GM
    from tests import test_gs_mapper_gpu as M
    truth = M._truth()
    poses = [M._pose7(0, 0, 0, 0, 0), M._pose7(0.15, 0.0, 0.0, 0.0, -0.04), M._pose7(-0.12, 0.08, 0.02, 0.03, 0.03)]
    obs = [M._observe(truth, p) for p in poses]

    def build():
        m = GM.GSMapper(M.CONFIG, M.FX, M.FY, M.CX, M.CY, downsample_ratio=2, device=DEV)
        for k, (p, (img, depth)) in enumerate(zip(poses, obs)):
            m.add_new_view(img, p, depth, kf_sub_idx=k, iters=5)
        m.h, m.w = M.H // 2, M.W // 2
        g = torch.Generator().manual_seed(1)
        with torch.no_grad():
            m.gaussians.p["scaling"][:, 0] += math.log(2.5)
            q = torch.randn(len(m.gaussians), 4, generator=g).to(DEV)
            m.gaussians.p["rotation"].copy_(q / q.norm(dim=-1, keepdim=True))
        return m
    bg = torch.zeros(3, device=DEV)
    tw = torch.tensor([[0.3, -0.2, 0.1, 0.2, -0.3, 0.25]], device=DEV)
    T = SE3.exp(tw)
    Tm = T.matrix()[0]
    out = {}
    for wide in (8, 7):
        m = build()
        sc = s if wide == 8 else 1.0
        with torch.no_grad():
            before = [GM.render(m.viewpoints[k], m.gaussians, bg) for k in range(3)]
            before = [(b["render"].clone(), b["depth"].clone()) for b in before]
            xyz0 = m.gaussians.get_xyz.detach().clone()
            ls0 = m.gaussians.theta.detach()[:, 7:10].clone()
            rot0 = m.gaussians.get_rotation.detach().clone()
        new_c2w = []
        for k in range(3):
            c2w = torch.inverse(GM.get_pose(m.viewpoints[k])).detach()
            n = torch.eye(4, device=DEV)
            n[:3, :3] = Tm[:3, :3] @ c2w[:3, :3]
            n[:3, 3] = sc * (Tm[:3, :3] @ c2w[:3, 3]) + Tm[:3, 3]
            new_c2w.append(n)
        data = T.data.repeat(3, 1)
        if wide == 8:
            data = torch.cat([data, torch.full((3, 1), s, device=DEV)], 1)
        packet = {"camera_idx": range(0, 3), "camera_pose": torch.stack([GM.SE3_from_matrix(c) for c in new_c2w]).cpu(),
                  "submap_idx": range(0, 3), "pose_updates": data.cpu()}
        upd, idx = m.gaussain_update(packet, refine_iters=0)
        with torch.no_grad():
            after = [GM.render(m.viewpoints[k], m.gaussians, bg) for k in range(3)]
        assert idx == [0, 1, 2] and upd["poses"].shape == (3, 7)
        psnr = np.mean([M._psnr(a["render"], b[0]) for a, b in zip(after, before)])
        dmax = max(float(b[1].max()) for b in before)
        psnr_d = np.mean([M._psnr(a["depth"] / sc / dmax, b[1] / dmax) for a, b in zip(after, before)])
        moved = sc * (Tm[:3, :3] @ xyz0.T).T + Tm[:3, 3]
        np.testing.assert_allclose(m.gaussians.get_xyz.detach().cpu().numpy(), moved.cpu().numpy(), atol=2e-5 * sc)
        ls1 = m.gaussians.theta.detach()[:, 7:10]
        if wide == 8:
            assert torch.equal(ls1, ls0 + torch.log(torch.tensor(s, device=DEV)))
        else:
            assert torch.equal(ls1, ls0)
        out[wide] = dict(psnr=psnr, psnr_d=psnr_d, depth=[m.viewpoints[k].depth.clone() for k in range(3)], rot=m.gaussians.get_rotation.detach().clone())
        print(f"\n[gs mapper] similarity s = {sc}: colour {psnr:.1f} dB, depth / s {psnr_d:.1f} dB")
        assert psnr > 40.0 and psnr_d > 40.0
        assert not torch.equal(out[wide]["rot"], rot0)
    # orientations compose exactly as on the 7-wide path; the viewpoints' depths are those of the 7-wide path times s (both paths end in
    # data_update's render-based depth scale, a clamped mean of log ratios that a similarity leaves unchanged up to rounding: 1e-4)
    assert torch.equal(out[8]["rot"], out[7]["rot"])
    for d8, d7 in zip(out[8]["depth"], out[7]["depth"]):
        np.testing.assert_allclose(d8.cpu().numpy(), s * d7.cpu().numpy(), rtol=1e-4)
