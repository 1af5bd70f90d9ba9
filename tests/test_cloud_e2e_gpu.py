"""GPU, end to end: cut3r_slam_amd.eval_dense on the sphere scene (GT depth PNGs + a TUM trajectory against a run that is the same scene
under a similarity, and against a run whose sphere is offset so that only ICP can align it), each against the numpy driver of
tests/cloud_oracle.py; the tracker's keyframes scored against themselves; demo.py --eval-dense."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cut3r_slam_amd import eval_dense as ED  # noqa: E402
from tests import cloud_oracle as CO  # noqa: E402
from tests import recon_oracle as RO  # noqa: E402
from tests import tsdf_oracle as TO  # noqa: E402

pytestmark = pytest.mark.gpu
SCALE = 6553.5
STEP = 1.0 / SCALE                                            # one quantisation step of the GT depth: 1.526e-4 m
OFFSET = np.array([0.02, -0.01, 0.015])


def _quat(R):
    """q = (x, y, z, w) of a rotation matrix (the branch of the largest diagonal term)"""
    t = np.trace(R)
    if t > 0:
        s = 2 * np.sqrt(1 + t)
        q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, s / 4]
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2 * np.sqrt(1 + R[i, i] - R[j, j] - R[k, k])
        q = [0.0, 0.0, 0.0, (R[k, j] - R[j, k]) / s]
        q[i], q[j], q[k] = s / 4, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s
    return np.asarray(q)


def _tum(poses, stamps):
    return np.stack([np.concatenate([[s], P[:3, 3], _quat(P[:3, :3])]) for P, s in zip(poses, stamps)])


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """the sphere scene as a GT data set on disk (depth PNGs floor-quantised at 6553.5, a TUM trajectory) read back by load_depth_dir"""
    from PIL import Image
    depth, rgb, w2c, K = TO.sphere_scene()
    w = np.tile(np.eye(4), (len(w2c), 1, 1))
    w[:, :3] = w2c.astype(np.float64).reshape(-1, 3, 4)
    c2w = np.linalg.inv(w)
    root = tmp_path_factory.mktemp("gt")
    (root / "depth").mkdir()
    for b, d in enumerate(depth):
        Image.fromarray(np.floor(d.astype(np.float64) * SCALE).astype(np.uint16)).save(root / "depth" / f"frame-{b:06d}.depth.png")
    np.savetxt(root / "gt.txt", _tum(c2w, np.arange(len(c2w))), fmt="%.18e")
    gt = ED.load_depth_dir(str(root / "depth"), SCALE, str(root / "gt.txt"), K.astype(np.float64))
    gt_np = (gt.depth.numpy(), ED.pose_matrices(gt.c2w), np.asarray(gt.K, np.float64), np.asarray(gt.stamps))
    return dict(depth=depth, c2w=c2w, K=K.astype(np.float64), gt=gt, gt_np=gt_np, root=root)


def _agree(got, want):
    for k in ED.KEYS:
        rel = abs(got[k] - want[k]) / want[k]
        print(f"{k}: GPU {got[k]:.9e} oracle {want[k]:.9e} rel {rel:.2e}")
    for k in ED.KEYS:
        assert abs(got[k] - want[k]) <= 1e-6 * want[k], k
    assert (got["n_gt"], got["n_est"], got["pairs"]) == (want["n_gt"], want["n_est"], want["pairs"])


def test_a_run_under_a_similarity_scores_below_one_quantisation_step(scene):
    s, R, t = 1 / 1.7, RO.rot([0.3, -0.5, 0.8], np.deg2rad(25.0)), np.array([0.4, -1.1, 2.0])
    poses = scene["c2w"].copy()
    poses[:, :3, :3] = R @ scene["c2w"][:, :3, :3]
    poses[:, :3, 3] = s * scene["c2w"][:, :3, 3] @ R.T + t
    e_depth = (scene["depth"].astype(np.float64) * s).astype(np.float32)
    stamps = np.arange(len(poses), dtype=np.float64)
    est = ED.DepthViews(torch.from_numpy(e_depth), poses, scene["K"], stamps)
    got = ED.dense_metrics(est, scene["gt"])
    want = CO.dense_metrics((e_depth, poses, scene["K"], stamps), scene["gt_np"])
    print(f"scale {got['scale']:.9f}, ICP {got['icp_iterations']} iterations, fitness {got['icp_fitness']:.4f}, n {got['n_gt']} / {got['n_est']}")
    assert abs(got["scale"] - 1.7) < 1e-6 and got["pairs"] == 24 and got["n_est"] == 98767
    _agree(got, want)
    assert got["RMSE_acc"] < STEP and got["RMSE_comp"] < STEP
    no_icp = ED.dense_metrics(est, scene["gt"], icp=False)
    print(f"without ICP: {[no_icp[k] for k in ED.KEYS]}")
    assert no_icp["RMSE_acc"] < STEP and no_icp["RMSE_comp"] < STEP and no_icp["icp_iterations"] == 0


def test_icp_recovers_an_offset_the_trajectories_cannot_see(scene):
    K4 = tuple(scene["K"])
    H, W = scene["depth"].shape[1:]
    w2c = np.linalg.inv(scene["c2w"])
    e_depth = np.stack([TO.render_sphere(T, K4, H, W, 0.5, center=OFFSET)[0] for T in w2c]).astype(np.float32)
    stamps = np.arange(len(w2c), dtype=np.float64)
    est = ED.DepthViews(torch.from_numpy(e_depth), scene["c2w"], scene["K"], stamps)
    got = ED.dense_metrics(est, scene["gt"])
    raw = ED.dense_metrics(est, scene["gt"], icp=False)
    want = CO.dense_metrics((e_depth, scene["c2w"], scene["K"], stamps), scene["gt_np"])
    T_icp = got["transformation"]
    print(f"ICP translation {T_icp[:3, 3]}, |t + offset| = {np.linalg.norm(T_icp[:3, 3] + OFFSET):.3e}, {got['icp_iterations']} iterations; "
          f"acc {raw['RMSE_acc']:.4e} -> {got['RMSE_acc']:.4e}, comp {raw['RMSE_comp']:.4e} -> {got['RMSE_comp']:.4e}")
    assert np.allclose(got["sim3"], np.eye(4), atol=1e-9)
    assert np.linalg.norm(T_icp[:3, 3] + OFFSET) < 5e-4
    assert got["RMSE_acc"] < 0.25 * raw["RMSE_acc"] and got["RMSE_comp"] < 0.25 * raw["RMSE_comp"]
    _agree(got, want)


def test_cli_scores_depth_directories(scene, tmp_path, capsys):
    from PIL import Image
    root = scene["root"]
    (tmp_path / "est").mkdir()
    for b, d in enumerate(scene["depth"]):
        Image.fromarray(np.floor(d.astype(np.float64) * SCALE).astype(np.uint16)).save(tmp_path / "est" / f"{b:06d}.png")
    calib = tmp_path / "calib.txt"
    calib.write_text(" ".join(repr(float(v)) for v in scene["K"]))
    rc = ED.main(["--est-depthdir", str(tmp_path / "est"), "--est-traj", str(root / "gt.txt"), "--est-calib", str(calib), "--gtdepthdir",
                  str(root / "depth"), "--gt-traj", str(root / "gt.txt"), "--gt-calib", str(calib), "--gt-depth-scale", repr(SCALE), "--no-icp",
                  "--save", str(tmp_path / "out")])
    assert rc == 0
    res = ED.read_results(tmp_path / "out" / "3D_eval_results.txt")
    assert set(res) == set(ED.KEYS) and all(v == 0.0 for v in res.values())          # the same cloud twice
    from cut3r_slam_amd.tsdf import read_ply
    a, b = read_ply(tmp_path / "out" / "pcd_est_aligned.ply"), read_ply(tmp_path / "out" / "pcd_gt.ply")
    assert len(a.faces) == 0 and a.vertices.shape == b.vertices.shape and len(a.vertices) > 90000


# ------------------------------------------------------------------------------------------------------------------- the run
@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """one tiny demo.py run with random weights, its Cut3rSlam kept"""
    import demo
    from cut3r_slam_amd import stream
    from tests.test_stream_gpu import _write_sequence
    root = tmp_path_factory.mktemp("run")
    (root / "colors").mkdir()
    _write_sequence(str(root / "colors"), 36)
    (root / "calib.txt").write_text("600.0 600.0 320.0 240.0")
    base = ["--imagedir", str(root / "colors"), "--calib", str(root / "calib.txt"), "--kf_every", "2", "--synthetic-weights", "--small", "--seed", "1"]
    seen, real = [], stream.save_trajectory
    mp = pytest.MonkeyPatch()
    mp.setattr(stream, "save_trajectory", lambda slam, *a, **k: (seen.append(slam), real(slam, *a, **k))[1])
    try:
        assert demo.main(base + ["--output", str(root / "plain")]) == 0
    finally:
        mp.undo()
    return dict(root=root, base=base, slam=seen[0])


def test_keyframes_scored_against_themselves_give_zero(run):
    slam = run["slam"]
    n = slam.keyframes.counter.value - 1
    views = ED.from_keyframes(slam.keyframes, n)
    assert views.depth.shape[0] == n >= 3 and views.rgb.shape[1] == 3
    dep = views.depth
    trunc = 1.01 * float(dep[(dep > 0) & torch.isfinite(dep)].max())
    res = ED.dense_metrics(views, views, depth_trunc=trunc, icp=False)
    print(f"{n} keyframes, {res['n_est']} points, scale {res['scale']!r}: {[res[k] for k in ED.KEYS]}")
    assert res["pairs"] == n and res["n_est"] == res["n_gt"] > 0
    assert res["RMSE_acc"] == 0.0 and res["RMSE_comp"] == 0.0 and res["Chamfer_distance"] == 0.0
    auto = ED.from_slam(slam, "auto")                          # no mapper attached: the tracker's keyframes
    assert auto.depth.shape == views.depth.shape
    with pytest.raises(ValueError):
        ED.from_slam(slam, "mapper")


def test_mapper_renders_are_a_source():
    """from_mapper / the mapper branch of from_slam on a 4-view Gaussian map of the synthetic wall: the stamps are the keyframes' frame
    indices (through stamps_full: the file stamps at those indices), the poses are camera-to-world.  The mapper's pose refinement moves
    a camera by at most its Adam step (pose_lr 1e-4) per iteration, far below 0.02 m here, and the views are 0.05 m apart, so a
    world-to-camera matrix taken for a pose (twice the distance off) cannot pass.  The renders scored against themselves give 0."""
    from types import SimpleNamespace as NS
    from cut3r_slam_amd import gs_mapper as GM
    from cut3r_slam_amd import synth
    H, W, f = 96, 128, 110.0
    packet, _, cfg = synth.gs_wall_window(H, W, focal=f, n_views=4, device="cuda:0")
    mapper = GM.GSMapper(cfg, f, f, W / 2, H / 2, downsample_ratio=2, device="cuda:0")
    with torch.enable_grad():
        mapper.run(packet, iterations=10)
    views = ED.from_mapper(mapper)
    assert tuple(views.depth.shape) == (4, H, W) and tuple(views.rgb.shape) == (4, 3, H, W) and views.rgb.dtype == torch.uint8
    assert views.stamps.tolist() == [0.0, 1.0, 2.0, 3.0] and np.allclose(views.K, [[f, f, W / 2, H / 2]] * 4)
    want = ED.pose_matrices(packet["poses"].numpy())
    off = np.linalg.norm(views.c2w[:, :3, 3] - want[:, :3, 3], axis=1)
    print(f"camera positions against the packet's: {off}")
    assert off.max() < 0.02 and np.abs(views.c2w[:, :3, :3] - want[:, :3, :3]).max() < 0.02
    slam = NS(mapper=mapper, keyframes=None, tracked_only=False)
    auto = ED.from_slam(slam, "auto", stamps_full=100.0 + 10.0 * np.arange(8))
    assert auto.stamps.tolist() == [100.0, 110.0, 120.0, 130.0] and torch.equal(auto.depth, views.depth)
    res = ED.dense_metrics(views, views, icp=False)
    assert res["pairs"] == 4 and res["n_est"] == res["n_gt"] > 0.9 * 4 * H * W
    assert res["RMSE_acc"] == 0.0 and res["RMSE_comp"] == 0.0 and res["Chamfer_distance"] == 0.0
    mapper.viewpoints[2].tstamp = None
    with pytest.raises(ValueError, match="tstamp"):
        ED.from_slam(slam, "mapper")


def test_demo_eval_dense_writes_the_results_and_leaves_the_trajectory_unchanged(run, tmp_path):
    import demo
    from PIL import Image
    slam, root = run["slam"], run["root"]
    kf = slam.keyframes
    n = kf.counter.value - 1
    dep = kf.depth[:n].cpu().numpy()
    top = float(dep[np.isfinite(dep) & (dep > 0)].max())
    scale = 60000.0 / top
    traj = np.loadtxt(root / "plain" / "traj_kf.txt")
    gtdir = tmp_path / "gtdepth"
    gtdir.mkdir()
    for row, d in zip(traj, dep):
        raw = np.floor(np.clip(np.nan_to_num(d.astype(np.float64), nan=0.0, posinf=0.0), 0, top) * scale).astype(np.uint16)
        Image.fromarray(raw).save(gtdir / f"depth{int(row[0]):06d}.png")
    K = kf.intrinsic[0].numpy()
    (tmp_path / "gtcalib.txt").write_text(" ".join(repr(float(v)) for v in K))
    out = tmp_path / "dense"
    rc = demo.main(run["base"] + ["--output", str(out), "--eval-dense", "--gtdepthdir", str(gtdir), "--gt-traj", str(root / "plain" / "traj_kf.txt"),
                                  "--gt-depth-scale", repr(scale), "--gt-calib", str(tmp_path / "gtcalib.txt"), "--dense-depth-trunc",
                                  repr(1.01 * top)])
    assert rc == 0
    assert (out / "traj_kf.txt").read_bytes() == (root / "plain" / "traj_kf.txt").read_bytes()
    res = ED.read_results(out / "3D_eval_results.txt")
    print(res)
    assert set(res) == set(ED.KEYS) and all(np.isfinite(v) and v >= 0 for v in res.values())
    assert not (root / "plain" / "3D_eval_results.txt").exists()


@pytest.mark.parametrize("extra", [["--eval-dense"], ["--eval-dense", "--gtdepthdir", "G"], ["--eval-dense", "--gt-traj", "g.txt"]])
def test_demo_refuses_eval_dense_without_its_inputs(extra, tmp_path):
    import demo
    with pytest.raises(SystemExit):
        demo.main(["--imagedir", str(tmp_path), "--calib", "c.txt", "--output", str(tmp_path / "o")] + extra)
