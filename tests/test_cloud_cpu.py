"""CPU: the numpy oracle of the dense point-cloud evaluation (tests/cloud_oracle.py) against analytic and hand-made cases, the depth PNG
reader and the command lines of cut3r_slam_amd.eval_dense and demo.py --eval-dense."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cut3r_slam_amd import eval_dense as ED  # noqa: E402
from cut3r_slam_amd import eval_recon as ER  # noqa: E402
from cut3r_slam_amd import ops  # noqa: E402
from tests import cloud_oracle as CO  # noqa: E402
from tests import recon_oracle as RO  # noqa: E402
from tests import tsdf_oracle as TO  # noqa: E402


def _c2w(w2c12):
    w = np.tile(np.eye(4), (len(w2c12), 1, 1))
    w[:, :3] = np.asarray(w2c12, np.float64).reshape(-1, 3, 4)
    return np.linalg.inv(w)


def test_sphere_scene_points_lie_on_the_sphere():
    depth, rgb, w2c, K = TO.sphere_scene()
    pts, col, counts = CO.backproject(depth, _c2w(w2c)[:, :3].reshape(-1, 12), K, 4.5, rgb=rgb)
    assert len(pts) == int((depth > 0).sum()) == counts.sum() == 98767 and col.shape == pts.shape and col.dtype == np.uint8
    err = np.abs(np.linalg.norm(pts.astype(np.float64), axis=1) - 0.5).max()
    print(f"max | |p| - r | = {err:.3e} over {len(pts)} points")
    assert err < 2e-7


def test_order_and_counts_of_a_hand_made_case():
    d = np.zeros((2, 3, 4), np.float32)
    d[0, 0, 1], d[0, 2, 3], d[0, 1, 0] = 2.0, 1.0, 4.0
    d[1, 2, 2] = 3.0
    rgb = np.arange(2 * 3 * 3 * 4, dtype=np.uint8).reshape(2, 3, 3, 4)
    c2w = np.array([[1, 0, 0, 10, 0, 1, 0, 20, 0, 0, 1, 30], [0, -1, 0, 0, 1, 0, 0, 0, 0, 0, 2, 1]], np.float64)
    K = np.array([2.0, 4.0, 1.0, 1.0])
    pts, col, counts = CO.backproject(d, c2w, K, 4.5, rgb=rgb)
    assert counts.tolist() == [3, 1]
    # view 0, row-major: (0,1) z 2, (1,0) z 4, (2,3) z 1; view 1: (2,2) z 3 -> x = 1.5, y = 0.75 -> (-0.75, 1.5, 7)
    want = np.array([[10 + 0.0, 20 - 0.5, 32], [10 - 2.0, 20 + 0.0, 34], [10 + 1.0, 20 + 0.25, 31], [-0.75, 1.5, 7.0]], np.float32)
    assert np.array_equal(pts, want)
    assert col.tolist() == [[1, 13, 25], [4, 16, 28], [11, 23, 35], [36 + 10, 48 + 10, 60 + 10]]
    # depth_trunc is exclusive, and nothing but finite positive depths counts
    d2 = np.array([[[0.0, -1.0, np.nan, np.inf, 4.5, np.nextafter(np.float32(4.5), np.float32(0))]]], np.float32)
    assert CO.backproject(d2, c2w[:1], K, 4.5)[2].tolist() == [1]


def test_nearest_index_rule():
    table = {(5, 3): [0, 1, 3], (5, 8): [0, 0, 1, 1, 2, 3, 3, 4], (4, 4): [0, 1, 2, 3]}
    for (n_src, n_dst), want in table.items():
        assert CO.nearest_index(n_src, n_dst).tolist() == want
    d = np.arange(1, 21, dtype=np.float32).reshape(1, 4, 5)
    pts, _, _ = CO.backproject(d, np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0.0]]), [1.0, 1.0, 0.0, 0.0], 100.0, size=(4, 8))
    assert pts[:, 2].reshape(4, 8)[1].tolist() == [6, 6, 7, 7, 8, 9, 9, 10]


def test_oracle_downsample_agrees_with_eval_recon():
    g = np.random.default_rng(3)
    p = (g.uniform(-1, 1, (5000, 3)) * [1.0, 0.6, 0.3]).astype(np.float32)
    p[:50] = np.round(p[:50] / 0.05) * 0.05                   # points on voxel faces
    for voxel in (0.05, 0.21):
        out, _, cnt = CO.voxel_downsample(p, voxel)
        ref = ER.voxel_down_sample(torch.from_numpy(p), voxel).numpy()
        assert out.shape == ref.shape and cnt.sum() == len(p)
        assert np.array_equal(out, ref.astype(np.float32))
        idx, key = CO.voxel_keys(p, voxel)
        assert np.array_equal(np.unique(idx, axis=0), idx[np.argsort(key, kind="stable")][np.r_[True, np.diff(np.sort(key)) != 0]])
    col = g.integers(0, 256, (5000, 3), dtype=np.uint8)
    _, c, cnt = CO.voxel_downsample(p, 0.5, col)
    assert c.dtype == np.uint8 and c.shape == (len(cnt), 3)
    one, c1, n1 = CO.voxel_downsample(p[:1], 0.05, col[:1])
    assert np.array_equal(one, p[:1]) and np.array_equal(c1, col[:1]) and n1.tolist() == [1]


def test_blocked_nn_equals_the_brute_force():
    g = np.random.default_rng(5)
    r = g.normal(size=(3000, 3))
    r = (0.5 * r / np.linalg.norm(r, axis=1, keepdims=True)).astype(np.float32)
    q = np.concatenate([r[:500] + g.normal(scale=2e-3, size=(500, 3)).astype(np.float32), g.uniform(-1, 1, (40, 3)).astype(np.float32),
                        r[:20]])
    for lim in (None, 0.5, 0.01):
        a, b = CO.nn_blocked(r, q, lim), RO.nn(r, q, lim)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_depth_png_round_trip(tmp_path):
    from PIL import Image
    d = tmp_path / "depth"
    d.mkdir()
    g = np.random.default_rng(0)
    raw = g.integers(0, 65536, (3, 6, 7), dtype=np.uint16)
    raw[0, 0, :3] = [65535, 0, 65534]
    for k, name in enumerate(("frame-2.depth.png", "frame-10.depth.png", "frame-1.depth.png")):
        Image.fromarray(raw[k]).save(d / name)
    (d / "notes.txt").write_text("not a depth map")
    traj = np.array([[1, 0, 0, 1, 0, 0, 0, 1], [2, 0, 0, 2, 0, 0, 0, 1], [7, 0, 0, 7, 0, 0, 0, 1], [10, 0, 0, 3, 0, 0, 1, 0]], np.float64)
    np.savetxt(tmp_path / "traj.txt", traj)
    v = ED.load_depth_dir(str(d), 1000.0, str(tmp_path / "traj.txt"), [585.0, 585.0, 320.0, 240.0])
    assert v.stamps.tolist() == [1.0, 2.0, 10.0]                                  # natural order, not the string order
    want = raw[[2, 0, 1]].astype(np.float32)
    want[want == 65535] = 0
    want = want / np.float32(1000.0)
    assert v.depth.dtype == torch.float32 and np.array_equal(v.depth.numpy(), want)
    assert v.depth[1, 0, 0] == 0 and v.depth[1, 0, 2] == np.float32(65534) / np.float32(1000)
    P = ED.pose_matrices(v.c2w)
    assert np.allclose(P[:, 2, 3], [1, 2, 3]) and np.allclose(P[2, :3, :3], np.diag([-1.0, -1.0, 1.0]))
    with pytest.raises(ValueError):
        ED.load_depth_dir(str(d), 1000.0, traj[2:3], [1, 1, 0, 0])             # no file at stamp 7


def test_results_file_round_trip(tmp_path):
    res = {"RMSE_acc": 0.0125, "RMSE_comp": 1e-5, "Chamfer_distance": 0.006255, "n_gt": 5}
    path = ED.write_results(str(tmp_path / "o"), res)
    assert open(path).read() == "RMSE_acc: 0.0125\nRMSE_comp: 1e-05\nChamfer_distance: 0.006255\n"
    assert ED.read_results(path) == {k: res[k] for k in ED.KEYS}


def test_grid_intrinsics_follow_the_resize():
    K = ED.grid_intrinsics([585.0, 585.0, 320.0, 240.0], 2, (480, 640), (392, 518))
    assert K.shape == (2, 4) and np.allclose(K[0], [585 * 518 / 640, 585 * 392 / 480, 320 * 518 / 640, 240 * 392 / 480])
    assert np.array_equal(ED.grid_intrinsics([1.0, 2.0, 3.0, 4.0], 1, (4, 4), None), [[1.0, 2.0, 3.0, 4.0]])


BASE = ["--est-depthdir", "D", "--est-traj", "t.txt", "--est-calib", "c.txt", "--gtdepthdir", "G", "--gt-traj", "g.txt", "--gt-calib", "k.txt"]


def test_cli_parsing():
    a = ED.parse_args(BASE)
    assert a.gt_depth_scale == 1000.0 and a.est_depth_scale == 6553.5 and a.resize is None and not a.no_icp and a.save is None
    a = ED.parse_args(BASE + ["--resize", "392", "518", "--no-icp", "--save", "out", "--gt-depth-scale", "5000"])
    assert a.resize == [392, 518] and a.no_icp and a.save == "out" and a.gt_depth_scale == 5000.0


@pytest.mark.parametrize("argv", [BASE[2:], BASE + ["--voxel", "0"], BASE + ["--gt-depth-scale", "-1"], BASE + ["--resize", "0", "5"],
                                  BASE + ["--resize", "392"], BASE + ["--est-depth-trunc", "0"], BASE + ["--max-diff", "-1"]])
def test_cli_refuses(argv):
    with pytest.raises(SystemExit):
        ED.parse_args(argv)


@pytest.mark.parametrize("extra", [["--eval-dense"], ["--eval-dense", "--gtdepthdir", "G"], ["--eval-dense", "--gt-traj", "g.txt"],
                                   ["--eval-dense", "--gtdepthdir", "G", "--gt-traj", "g.txt", "--gt-depth-scale", "0"],
                                   ["--eval-dense", "--gtdepthdir", "G", "--gt-traj", "g.txt", "--dense-source", "other"],
                                   ["--gt-traj", "g.txt"]])
def test_demo_refuses_bad_dense_flags(extra, tmp_path):
    import demo
    with pytest.raises(SystemExit):
        demo.main(["--imagedir", str(tmp_path), "--calib", "c.txt", "--output", str(tmp_path / "o")] + extra)


def test_too_few_pairs_is_an_error():
    v = ED.DepthViews(np.ones((2, 2, 2), np.float32), np.tile(np.eye(4), (2, 1, 1)), [1.0, 1.0, 0.0, 0.0], [0.0, 1.0])
    with pytest.raises(ValueError, match="associated"):
        ED.dense_metrics(v, v)


def test_aligned_trajectories_give_the_exact_identity():
    """trajectory_sim3: positions that are already aligned (here 50 seeded sets against themselves, where eval_ate.umeyama returns the
    identity only up to the rounding of its SVD) give s = 1, R = I, t = 0 exactly; a real similarity is umeyama's answer unchanged"""
    from cut3r_slam_amd.eval_ate import umeyama
    rng = np.random.default_rng(3)
    perturbed = 0
    for _ in range(50):
        p = rng.normal(size=(int(rng.integers(3, 40)), 3)) * rng.uniform(0.1, 30.0) + rng.normal(size=3) * 10
        s0, R0, t0 = umeyama(p, p, True)
        perturbed += not (s0 == 1.0 and np.array_equal(R0, np.eye(3)) and np.array_equal(t0, np.zeros(3)))
        s, R, t = ED.trajectory_sim3(p, p)
        assert s == 1.0 and np.array_equal(R, np.eye(3)) and np.array_equal(t, np.zeros(3))
    assert perturbed > 0                                                   # what the rule is there for
    p = rng.normal(size=(20, 3))
    q = 1.7 * p @ RO.rot([0.3, -0.5, 0.8], 0.4).T + [0.4, -1.1, 2.0]
    s, R, t = ED.trajectory_sim3(p, q)
    s0, R0, t0 = umeyama(p, q, True)
    assert s == s0 and np.array_equal(R, R0) and np.array_equal(t, t0) and abs(s - 1.7) < 1e-12


def test_mapper_views_without_a_frame_index_are_refused():
    """a mapper keyframe added without a tstamp has only its key, a keyframe index; from_mapper and from_slam refuse to take it for a
    frame index (it would pair the view with the wrong GT frame) before anything is rendered"""
    from types import SimpleNamespace as NS
    mapper = NS(viewpoints={0: NS(tstamp=0.0), 1: NS(tstamp=None), 2: NS(tstamp=8.0)})
    with pytest.raises(ValueError, match="tstamp"):
        ED.from_mapper(mapper)
    with pytest.raises(ValueError, match="tstamp"):
        ED.from_slam(NS(mapper=mapper), "mapper", stamps_full=np.arange(10.0))
    with pytest.raises(ValueError, match="no keyframes"):
        ED.from_mapper(NS(viewpoints={}))
    mapper.viewpoints[1].tstamp = 4.0
    assert ED._mapper_frame_indices(mapper) == [0.0, 4.0, 8.0]
