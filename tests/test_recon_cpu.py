"""CPU: the numpy restatement of the reconstruction-metric kernels (tests/recon_oracle.py) and the host logic of
cut3r_slam_amd/eval_recon.py -- sampling statistics, prefix stability, the ICP loop, voxel_down_sample, the Sim(3) of two trajectories
and the command line."""
import ast
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cut3r_slam_amd import eval_recon as ER  # noqa: E402
from cut3r_slam_amd import tsdf as T  # noqa: E402
from tests import recon_oracle as O  # noqa: E402


def _cdf(v, f):
    return np.cumsum(O.face_areas(v, f).astype(np.float64))


def test_samples_lie_on_their_faces():
    v, f = O.icosphere(2)
    s = O.sample(v, f, _cdf(v, f), 5000, seed=3, stream=1).astype(np.float64)
    # the sample's face: recover barycentrics against every face it could lie on (the nearest plane, then inside the triangle)
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    for p in s[:500]:
        dist = np.abs(((p - a) * n).sum(1))
        k = int(np.argmin(dist))
        assert dist[k] < 1e-6
        e1, e2, w = b[k] - a[k], c[k] - a[k], p - a[k]
        G = np.array([[e1 @ e1, e1 @ e2], [e1 @ e2, e2 @ e2]])
        u1, u2 = np.linalg.solve(G, [w @ e1, w @ e2])
        assert u1 >= -1e-5 and u2 >= -1e-5 and u1 + u2 <= 1 + 1e-5


def test_area_split_one_to_three_is_sampled_one_to_three():
    # two triangles of areas 1 and 3 (and a degenerate face between them, never picked)
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [5, 0, 0], [8, 0, 0], [5, 2, 0], [9, 9, 9]], np.float32)
    f = np.array([[0, 1, 2], [6, 6, 6], [3, 4, 5]], np.int32)
    areas = O.face_areas(v, f)
    assert areas.tolist() == [1.0, 0.0, 3.0]
    n = 40000
    s = O.sample(v, f, _cdf(v, f), n, seed=11)
    left = int((s[:, 0] < 2.5).sum())
    assert not np.any(np.all(s == v[6], axis=1))
    exp = np.array([n / 4, 3 * n / 4])
    chi2 = float((((np.array([left, n - left]) - exp) ** 2) / exp).sum())
    assert chi2 < 10.83                                   # 1 degree of freedom, p = 0.001


def test_samples_are_prefix_stable_and_streams_independent():
    v, f = O.icosphere(1)
    cdf = _cdf(v, f)
    long = O.sample(v, f, cdf, 3000, seed=5, stream=1)
    short = O.sample(v, f, cdf, 1000, seed=5, stream=1)
    assert np.array_equal(long[:1000].view(np.uint32), short.view(np.uint32))
    other = O.sample(v, f, cdf, 1000, seed=5, stream=2)
    assert np.count_nonzero(np.any(other != short, axis=1)) > 990


def test_numpy_icp_recovers_a_known_motion():
    rng = np.random.default_rng(0)
    v, f = O.box_room((2.0, 1.5, 1.2), 0.1)
    dst = O.sample(v, f, _cdf(v, f), 3000, seed=1)
    R = O.rot([0.3, -0.5, 0.8], np.deg2rad(2.0))
    t = np.array([0.03, -0.02, 0.01])
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, t
    src = ((dst.astype(np.float64) - t) @ R).astype(np.float32)          # M @ src = dst
    src = src[rng.permutation(len(src))]
    Tm, fit, rmse, it = O.icp(src, dst, 0.1)
    assert 1 < it <= 30 and fit == 1.0 and rmse < 1e-5
    dR = Tm[:3, :3] @ R.T
    assert np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1)) < 1e-4 and np.abs(Tm[:3, 3] - t).max() < 1e-4


def test_rigid_fit_from_moments_matches_the_pairwise_fit():
    rng = np.random.default_rng(1)
    s = rng.normal(size=(200, 3))
    d = s @ O.rot([1, 2, 3], 0.4).T + [0.5, -1.0, 2.0] + 0.01 * rng.normal(size=(200, 3))
    m = np.concatenate([[200.0, 0.0], s.sum(0), d.sum(0), (s[:, :, None] * d[:, None, :]).sum(0).ravel()])
    assert np.abs(ER.rigid_from_moments(m) - O.rigid_fit(s, d)).max() < 1e-12
    assert np.array_equal(ER.rigid_from_moments(np.zeros(17)), np.eye(4))


def test_voxel_down_sample_on_hand_made_cases():
    p = torch.tensor([[0.0, 0.0, 0.0], [0.04, 0.0, 0.0], [0.06, 0.0, 0.0], [0.0, 0.2, 0.0], [0.01, 0.21, 0.0]], dtype=torch.float64)
    # min = 0, the grid starts at -0.05: x in [-0.05, 0.05) -> 0, [0.05, 0.15) -> 1; y 0.2, 0.21 -> 2
    out = ER.voxel_down_sample(p, 0.1)
    exp = torch.tensor([[0.02, 0.0, 0.0], [0.005, 0.205, 0.0], [0.06, 0.0, 0.0]], dtype=torch.float64)
    assert out.shape == (3, 3) and torch.allclose(out, exp, atol=1e-15)
    one = ER.voxel_down_sample(np.array([[1.0, 2.0, 3.0]] * 4), 0.5)
    assert one.tolist() == [[1.0, 2.0, 3.0]]
    with pytest.raises(ValueError):
        ER.voxel_down_sample(p, 0.0)


def test_sim3_from_trajectories_recovers_scale_rotation_translation(tmp_path):
    rng = np.random.default_rng(2)
    n = 40
    gt = np.zeros((n, 8))
    gt[:, 0] = np.arange(n) * 0.1
    gt[:, 1:4] = rng.normal(size=(n, 3))
    gt[:, 7] = 1.0
    s, R, t = 0.37, O.rot([0.2, 1.0, -0.4], 0.9), np.array([1.0, -2.0, 0.5])
    est = gt.copy()
    est[:, 1:4] = ((gt[:, 1:4] - t) @ R) / s                             # gt = s R est + t
    np.savetxt(tmp_path / "gt.txt", gt)
    np.savetxt(tmp_path / "est.txt", est)
    M = ER.sim3_from_trajectories(str(tmp_path / "est.txt"), str(tmp_path / "gt.txt"))
    assert np.abs(M[:3, :3] - s * R).max() < 1e-9 and np.abs(M[:3, 3] - t).max() < 1e-9
    with pytest.raises(ValueError):
        ER.sim3_from_trajectories(est[:2], gt[:2])


def test_cli_parses_the_reference_arguments_and_save_round_trips(tmp_path, monkeypatch):
    a = ER.parse_args(["rec.ply", "gt.ply", "--eval_3d", "--save", "out.txt"])
    assert (a.rec_mesh, a.gt_mesh, a.eval_3d, a.save, a.no_align, a.samples, a.seed) == ("rec.ply", "gt.ply", True, "out.txt", False, 200000, 0)
    b = ER.parse_args(["r", "g", "--no-align", "--transform", "m.npy", "--traj-est", "e", "--traj-gt", "t", "--samples", "10", "--seed", "4"])
    assert b.no_align and b.transform == "m.npy" and (b.traj_est, b.traj_gt, b.samples, b.seed) == ("e", "t", 10, 4)
    with pytest.raises(SystemExit):
        ER.parse_args(["r", "g", "--traj-est", "e"])
    v, f = O.icosphere(0)
    T.write_ply(tmp_path / "m.ply", T.Mesh(v, np.zeros_like(v, dtype=np.uint8), f))
    seen = {}

    def fake(rec, gt, eval_3d=True, align=True, samples=0, seed=0):
        seen.update(rec=rec, gt=gt, align=align, samples=samples, seed=seed)
        return {"accuracy": 1.25, "completion": 2.5, "completion_ratio": 97.125}
    monkeypatch.setattr(ER, "eval_recon", fake)
    out = tmp_path / "res.txt"
    M = np.eye(4)
    M[:3, 3] = [1.0, 2.0, 3.0]
    np.save(tmp_path / "M.npy", M)
    assert ER.main([str(tmp_path / "m.ply"), str(tmp_path / "m.ply"), "--eval_3d", "--save", str(out), "--no-align", "--samples", "77",
                    "--transform", str(tmp_path / "M.npy")]) == 0
    assert ast.literal_eval(out.read_text()) == {"accuracy": 1.25, "completion": 2.5, "completion_ratio": 97.125}
    assert seen["align"] is False and seen["samples"] == 77
    assert np.allclose(seen["rec"].vertices, v + np.float32([1, 2, 3]))
