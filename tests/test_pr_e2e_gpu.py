"""GPU: precision / recall / F-score end to end (cut3r_slam_amd/eval_recon.py) -- an analytic two-plane case, ICP with scale on a known
similarity, run_evaluation on a pair of icospheres against the brute-force pipeline of tests/pr_oracle.py, and the command line."""
import ast
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cut3r_slam_amd import eval_recon as ER  # noqa: E402
from cut3r_slam_amd import ops  # noqa: E402
from cut3r_slam_amd import tsdf as T  # noqa: E402
from tests import pr_oracle as PO  # noqa: E402
from tests import recon_oracle as RO  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("precision", "recall", "f-score", "mean precision", "mean recall", "median precision", "median recall")


def _bits(x):
    return np.float64(x).view(np.uint64)


def _same_as_oracle(res, o, tau):
    """a PRResult against the dict of pr_oracle.precision_recall: shares and cumulatives exact, means / medians / std bit for bit"""
    assert len(res.dist2_rec) == int(o["rec"]["counts"][0]) and len(res.dist2_gt) == int(o["gt"]["counts"][0])     # all good
    assert (res.precision, res.recall, res.fscore) == (o["precision"], o["recall"], o["fscore"])
    assert np.array_equal(res.edges, o["edges"])
    assert np.array_equal(res.cum_rec, o["rec"]["cum"]) and np.array_equal(res.cum_gt, o["gt"]["cum"])
    nbins, w = len(res.edges) - 1, res.edges[1]
    for side, d2 in (("rec", res.dist2_rec), ("gt", res.dist2_gt)):
        for k in ("mean", "median", "std", "min", "max"):
            assert _bits(getattr(res, f"{k}_{side}")) == _bits(o[side][k]), (side, k, getattr(res, f"{k}_{side}"), o[side][k])
        counts, _, hist = ops.dist_stats(d2, tau, float(w), nbins)
        assert np.array_equal(hist.cpu().numpy(), o[side]["hist"]) and np.array_equal(counts.cpu().numpy(), o[side]["counts"])


def test_two_planes_score_one_half():
    # GT: a 32 x 32 grid at spacing 0.1 on z = 0; rec: the same grid 0.03 above it in the even columns and 0.07 above it in the odd ones.
    # Every nearest neighbour is the point straight below / above (the next column is 0.1 away), so at tau = 0.05 exactly half of each
    # cloud is inside, and both mean distances are (0.03 + 0.07) / 2 up to the fp32 rounding of coordinates <= 3.2
    i, j = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    gt = np.stack([0.1 * i, 0.1 * j, 0.0 * i], -1).reshape(-1, 3).astype(np.float32)
    rec = gt.copy()
    rec[:, 2] = np.where(i.reshape(-1) % 2 == 0, np.float32(0.03), np.float32(0.07))
    res = ER.precision_recall(rec, gt, tau=0.05, voxel=0)
    assert (res.precision, res.recall, res.fscore) == (0.5, 0.5, 0.5)
    assert abs(res.mean_rec - 0.05) < 1e-6 and abs(res.mean_gt - 0.05) < 1e-6
    assert abs(res.median_rec - 0.05) < 1e-6 and abs(res.min_rec - 0.03) < 1e-6 and abs(res.max_gt - 0.07) < 1e-6
    assert abs(res.std_rec - 0.02) < 1e-6
    _same_as_oracle(res, PO.precision_recall(rec, gt, 0.05, voxel=0), 0.05)
    assert res.cum_rec[-1] == 1.0 and res.cum_rec[141] == 1.0 and res.cum_rec[99] == 0.5 and res.cum_rec[60] == 0.5 and res.cum_rec[58] == 0.0
    d = ER.pr_dict(res)
    assert d["precision"] == 50.0 and d["recall"] == 50.0 and d["f-score"] == 50.0 and abs(d["mean precision"] - 5.0) < 1e-4
    # a cloud with a non-finite nearest-neighbour distance is refused, not averaged
    with pytest.raises(ValueError):
        ER._one_way(torch.tensor([0.1, float("inf")], device=DEV), 0.05, 5e-4, 500)


def _similarity_case(s, n=16, deg=5.0, seed=0):
    """target: a 16^3 grid over [-0.5, 0.5]^3 with every point jittered by up to half a cell (a lattice with less jitter aliases: ICP
    then settles a whole cell off, in Open3D as here); source: its inverse image under s R(5 deg) + t, |t| under a quarter of the cell"""
    rng = np.random.default_rng(seed)
    h = 1.0 / n
    g = (np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3) + 0.5) * h - 0.5
    tgt = g + rng.uniform(-0.5, 0.5, g.shape) * h
    tgt -= tgt.mean(0)
    R = RO.rot([0.3, -0.5, 0.8], np.deg2rad(deg))
    t = np.array([0.15, -0.1, 0.1]) * h                                    # |t| = 0.21 h
    src = ((tgt - t) @ R) / s                                              # s R src + t = tgt
    return src.astype(np.float32), tgt.astype(np.float32), R, t


def test_icp_with_scale_recovers_a_known_similarity():
    """s = 1.1, 5 degrees: the points at the rim move by more than a cell, so NOT every first correspondence is right (a sixth are);
    the loop still lands on the exact correspondences (the numpy loop of tests/pr_oracle.py: 12 iterations), after which the estimate is
    exact up to the fp32 application of T to coordinates <= 2, ~1e-6: the bounds are ten times that"""
    src, tgt, R, t = _similarity_case(1.1)
    res = ER.icp_point_to_point(src, tgt, 0.2, with_scaling=True)
    M = res.transformation
    s = np.cbrt(np.linalg.det(M[:3, :3]))
    assert res.fitness == 1.0 and res.iterations < 30 and res.inlier_rmse < 1e-6
    assert abs(s / 1.1 - 1) < 1e-5 and np.abs(M[:3, :3] / s - R).max() < 1e-5 and np.abs(M[:3, 3] - t).max() < 1e-5
    assert np.array_equal(M[3], [0, 0, 0, 1])
    # the rigid version: with_scaling=False is the call without the argument
    src, tgt, R, t = _similarity_case(1.0)
    a = ER.icp_point_to_point(src, tgt, 0.2)
    b = ER.icp_point_to_point(src, tgt, 0.2, with_scaling=False)
    assert np.array_equal(a.transformation, b.transformation) and a[1:] == b[1:]
    assert np.abs(a.transformation[:3, :3] - R).max() < 1e-5 and np.abs(a.transformation[:3, 3] - t).max() < 1e-5
    # and the scaled loop finds s = 1 there
    c = ER.icp_point_to_point(src, tgt, 0.2, with_scaling=True).transformation
    assert abs(np.cbrt(np.linalg.det(c[:3, :3])) - 1) < 1e-5


def _sphere(radius):
    v, f = RO.icosphere(3, radius)
    return T.Mesh(v, np.zeros((len(v), 3), np.uint8), f)


def test_run_evaluation_on_an_icosphere_pair(tmp_path):
    """radii 1.02 (rec) and 1 (GT), 4000 samples, at PO.SPHERE_TAU (see there: at 0.05 the score would measure the sampling).  The oracle
    pipeline gets the GPU's samples and, for the aligned run, the GPU's transform."""
    tau = PO.SPHERE_TAU
    rec_mesh, gt_mesh = _sphere(1.02), _sphere(1.0)
    rec_pc = ER.sample_surface(rec_mesh, 4000, seed=0, stream=ER.STREAM_REC)
    gt_pc = ER.sample_surface(gt_mesh, 4000, seed=0, stream=ER.STREAM_GT)
    rh, gh = rec_pc.cpu().numpy(), gt_pc.cpu().numpy()
    # as they come
    res, M = ER.evaluate_points(rec_pc, gt_pc, tau, icp_align=False)
    assert np.array_equal(M, np.eye(4))
    _same_as_oracle(res, PO.precision_recall(rh, gh, tau), tau)
    out = ER.run_evaluation(rec_mesh, gt_mesh, distance_thresh=tau, icp_align=False, samples=4000, out_dir=tmp_path / "pr")
    assert out == ER.pr_dict(res) and set(out) == set(KEYS) and all(type(v) is float for v in out.values())
    assert out["precision"] == 100.0 and out["recall"] == 100.0 and out["f-score"] == 100.0
    assert 1.9 < out["mean precision"] < 2 + 100 * tau and 1.9 < out["mean recall"] < 2 + 100 * tau
    metrics = ast.literal_eval(f"{out}")                                   # scripts/run_replica.py:53-57
    assert metrics['mean precision'] == out["mean precision"] and metrics['mean recall'] > 0 and metrics['recall'] == 100.0
    # the files
    for name, pts, d2 in (("precision", res.rec_points, res.dist2_rec), ("recall", res.gt_points, res.dist2_gt)):
        ply = T.read_ply(tmp_path / "pr" / f"{name}.ply")
        assert len(ply.faces) == 0 and np.array_equal(ply.vertices, pts.cpu().numpy())
        assert np.array_equal(ply.colors, ER.error_colors(d2.double().sqrt(), tau).cpu().numpy())
        assert ply.colors[:, 0].min() > 200 and ply.colors[:, 2].max() < 255          # 0.02 .. 0.12 of 0.6: the white-to-yellow end
    curve = np.loadtxt(tmp_path / "pr" / "pr_curve.txt")
    assert curve.shape == (500, 3) and np.allclose(curve[:, 0], res.edges[1:], rtol=1e-8) and np.allclose(curve[:, 1], res.cum_rec, atol=1e-8)
    # aligned, with scale
    res2, M2 = ER.evaluate_points(rec_pc, gt_pc, tau, icp_align=True, with_scaling=True)
    s = np.cbrt(np.linalg.det(M2[:3, :3]))
    assert abs(s * 1.02 - 1) < 0.01, s
    _same_as_oracle(res2, PO.precision_recall(PO.transform_points(rh, M2), gh, tau), tau)
    out2 = ER.run_evaluation(rec_mesh, gt_mesh, distance_thresh=tau, icp_align=True, with_scaling=True, samples=4000)
    assert out2 == ER.pr_dict(res2) and out2["precision"] == 100.0 and out2["recall"] == 100.0
    assert out2["mean precision"] < out["mean precision"] and out2["mean recall"] < out["mean recall"]


def test_demo_eval_pr_adds_the_keys_and_nothing_else(tmp_path, monkeypatch):
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
    monkeypatch.setattr(stream, "save_trajectory", lambda slam, *a, **k: seen.append(slam) or real(slam, *a, **k))
    for bad in (["--eval-pr"], ["--mesh", "--eval-pr"], ["--mesh", "--gt-mesh", "g.ply", "--eval-pr-scale"]):
        with pytest.raises(SystemExit):
            demo.main(base + ["--output", str(tmp_path / "bad")] + bad)
    assert demo.main(base + ["--output", str(tmp_path / "plain")]) == 0
    kf = seen[0].keyframes
    n = kf.counter.value - 1
    dep = kf.depth[:n]
    depth_max = float(dep[(dep > 0) & torch.isfinite(dep)].max())
    lo, hi = T.depth_bounds(dep, kf.w2c[:n], kf.intrinsic[:n].to(DEV), depth_max)
    mesh_args = ["--mesh", "--voxel-size", repr(float(np.max(hi - lo)) / 64), "--depth-max", repr(depth_max)]
    assert demo.main(base + ["--output", str(tmp_path / "first")] + mesh_args) == 0
    gt = tmp_path / "first" / "tsdf_mesh_w1.0.ply"
    assert demo.main(base + ["--output", str(tmp_path / "three"), "--gt-mesh", str(gt)] + mesh_args) == 0
    calls = []
    real_pr = ER.run_evaluation
    monkeypatch.setattr(ER, "run_evaluation", lambda *a, **k: calls.append(k) or real_pr(*a, **k))
    assert demo.main(base + ["--output", str(tmp_path / "pr"), "--gt-mesh", str(gt), "--eval-pr", "--eval-pr-scale"] + mesh_args) == 0
    assert calls == [{"with_scaling": True}]
    res3 = ast.literal_eval((tmp_path / "three" / "eval_recon_w1.0.txt").read_text())
    res = ast.literal_eval((tmp_path / "pr" / "eval_recon_w1.0.txt").read_text())
    assert set(res3) == {"accuracy", "completion", "completion_ratio"} and set(res) == set(res3) | set(KEYS)
    assert {k: res[k] for k in res3} == res3                               # the 3-D scores as they were
    assert all(np.isfinite(res[k]) and res[k] >= 0 for k in KEYS) and res["precision"] <= 100 and res["recall"] <= 100
    print(f"with --eval-pr {res}")


def test_cli_writes_what_the_run_script_reads(tmp_path):
    rec, gt, save = tmp_path / "rec.ply", tmp_path / "gt.ply", tmp_path / "eval.txt"
    T.write_ply(rec, _sphere(1.02))
    T.write_ply(gt, _sphere(1.0))
    common = [str(rec), str(gt), "--eval_3d", "--samples", "4000", "--no-align", "--save", str(save)]
    assert ER.main(common) == 0
    plain = ast.literal_eval(save.read_text())
    assert set(plain) == {"accuracy", "completion", "completion_ratio"}     # without --pr: the file of before
    assert ER.main(common + ["--pr", "--pr-thresh", str(PO.SPHERE_TAU), "--pr-out", str(tmp_path / "out")]) == 0
    result = ast.literal_eval(save.read_text())
    assert {k: result[k] for k in plain} == plain and set(result) == set(plain) | set(KEYS)
    assert result['mean precision'] > 0 and result['mean recall'] > 0 and result['recall'] == 100.0      # run_replica.py:54-56
    assert sorted(os.listdir(tmp_path / "out")) == ["pr_curve.txt", "precision.ply", "recall.ply"]
