"""CPU: self-calibration without a GPU.  The numpy oracle of csrc/calib.hip (tests/focal_oracle.py) against what the reference's own
`estimate_focal_knowing_depth` returned for the seeded pointmaps of tests/golden/focal.npz (tests/golden/make_focal_fixture.py); the alias
modules; the host half of the policy, the keyframe store and the stream's argument handling."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import focal_oracle as FO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPAT = os.path.join(ROOT, "cut3r_slam_amd", "compat")
CASES = ("patch", "offcentre", "exact", "large", "noise")


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "focal.npz"))


def clip0(f):
    """the reference's default clip, min_focal = 0 and max_focal = inf (NaN stays NaN)"""
    return np.where(np.isnan(f), f, np.maximum(f, np.float32(0)))


@pytest.mark.parametrize("name", CASES)
def test_oracle_median_equals_the_reference(fixture, name):
    got = clip0(FO.median(fixture[f"{name}_pts"], fixture[f"{name}_pp"]))
    print(name, "median", got, fixture[f"{name}_median"])
    assert got.dtype == np.float32 and np.array_equal(got, fixture[f"{name}_median"])          # by value (-0 == +0)


@pytest.mark.parametrize("name", CASES)
def test_oracle_weiszfeld_within_the_references_own_rounding_noise(fixture, name):
    """allowed deviation from the reference's fp64 run = 4 x |its fp32 run - its fp64 run|, at least 4 fp32 ulps of the value: the oracle
    rounds the same per-pixel terms to fp32, so its error is of that size and independent of the reference's; a wrong formula misses by
    1e-3 or more.  Measured ratios |oracle - fp64| / allowed: patch 0.05 / 0.20 / 0.30, offcentre 0.05 / 0.02, exact 0, large 0.04,
    noise 0 (both clipped to 0)."""
    got = clip0(FO.weiszfeld(fixture[f"{name}_pts"], fixture[f"{name}_pp"])).astype(np.float64)
    w32, w64 = fixture[f"{name}_weiszfeld"].astype(np.float64), fixture[f"{name}_weiszfeld64"]
    allowed = np.maximum(4 * np.abs(w32 - w64), 4 * np.spacing(np.abs(w64).astype(np.float32)).astype(np.float64))
    dev = np.abs(got - w64)
    print(name, "weiszfeld", got, w64, "deviation", dev, "allowed", allowed, "ratio", dev / allowed)
    assert np.all(dev <= allowed)


def test_exact_pinhole_walks_the_clip_of_the_weights(fixture):
    assert np.array_equal(fixture["exact_weiszfeld"], np.float32([32.0])) and np.array_equal(fixture["exact_median"], np.float32([32.0]))
    assert np.array_equal(FO.weiszfeld(fixture["exact_pts"], fixture["exact_pp"]), np.float32([32.0]))


def test_oracle_gate_and_empty_views():
    rng = np.random.default_rng(1)
    pts = rng.standard_normal((2, 9, 11, 3)).astype(np.float32) + np.float32([0, 0, 3])
    pp = np.float32([[5.5, 4.5]] * 2)
    conf = rng.uniform(0, 2, (2, 9, 11)).astype(np.float32)
    conf[1] = 0
    for fn in (FO.weiszfeld, FO.median):
        out = fn(pts, pp, conf=conf, conf_min=1.0)
        assert np.isfinite(out[0]) and np.isnan(out[1])
    # the gated estimate is the estimate of the kept pixels: gated pixels replaced by NaN points are void votes / non-finite ratios
    # only for the median (a NaN ratio counts as 0 in the Weiszfeld sums, which is what a gated pixel adds too)
    masked = pts.copy()
    masked[conf < 1.0] = np.nan
    assert np.array_equal(FO.median(masked[:1], pp[:1]), FO.median(pts[:1], pp[:1], conf=conf[:1], conf_min=1.0))
    assert np.array_equal(FO.weiszfeld(masked[:1], pp[:1]), FO.weiszfeld(pts[:1], pp[:1], conf=conf[:1], conf_min=1.0))


def test_post_process_resolves_through_the_alias_packages():
    """the reference's commented import (hislam2/track_frontend.py:10) and the model files' `dust3r.*` spelling, compat/ alone on the path"""
    prog = "\n".join([
        f"import sys; sys.path.insert(0, {COMPAT!r})",
        "from src.dust3r.post_process import estimate_focal_knowing_depth as a",
        "from dust3r.post_process import estimate_focal_knowing_depth as b",
        "import inspect, cut3r_slam_amd.self_calib as S",
        "assert a is b is S.estimate_focal_knowing_depth",
        "p = inspect.signature(a).parameters",
        "assert list(p)[:5] == ['pts3d', 'pp', 'focal_mode', 'min_focal', 'max_focal']",
        "assert p['focal_mode'].default == 'median' and p['min_focal'].default == 0.0 and p['max_focal'].default == float('inf')",
        "print('RESOLVED')"])
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    r = subprocess.run([sys.executable, "-c", prog], cwd="/", env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0 and "RESOLVED" in r.stdout, r.stderr[-2000:]


def test_estimate_refuses_bad_modes_and_cpu_tensors():
    from cut3r_slam_amd.self_calib import estimate_focal_knowing_depth
    pts, pp = torch.ones(1, 4, 4, 3), torch.tensor([[2.0, 2.0]])
    with pytest.raises(ValueError, match="bad focal_mode='mean'"):
        estimate_focal_knowing_depth(pts, pp, focal_mode="mean")
    for mode in ("median", "weiszfeld"):
        with pytest.raises(ValueError, match="GPU"):
            estimate_focal_knowing_depth(pts, pp, focal_mode=mode)


def test_policy_defaults_and_config_section():
    from cut3r_slam_amd.self_calib import SelfCalibration, focal_base
    d = SelfCalibration()
    assert (d.mode, d.conf_min, d.min_focal, d.max_focal) == ("weiszfeld", None, 0.25, 4.0)
    c = SelfCalibration({"Tracking": {"calibration": {"mode": "median", "conf_min": 1.5, "max_focal": 8}}})
    assert (c.mode, c.conf_min, c.min_focal, c.max_focal) == ("median", 1.5, 0.25, 8.0)
    assert focal_base(384, 512) == 512 / (2 * np.tan(np.deg2rad(30)))
    with pytest.raises(ValueError):
        SelfCalibration({"Tracking": {"calibration": {"mode": "mean"}}})
    with pytest.raises(ValueError):
        SelfCalibration({"Tracking": {"calibration": {"min_focal": 2, "max_focal": 1}}})


def test_policy_takes_the_lower_median_of_the_finite_views_and_refuses_the_rest():
    from cut3r_slam_amd.self_calib import SelfCalibration
    pol = SelfCalibration()
    H, W = 384, 512
    lo, hi = pol.bounds(H, W)
    assert abs(lo - 0.25 * 443.405) < 0.01 and abs(hi - 4 * 443.405) < 0.05
    assert pol.select(np.float32([500, 300, np.nan, 400, 450]), H, W) == (400.0, 400.0, 256.0, 192.0)          # even count: the lower of the two
    assert pol.select(np.float32([500, 300, 400]), H, W) == (400.0, 400.0, 256.0, 192.0)
    assert pol.select(np.float32([np.nan, np.inf, 321.5]), H, W)[0] == 321.5
    with pytest.raises(RuntimeError, match="no view"):
        pol.select(np.float32([np.nan] * 6), H, W)
    with pytest.raises(RuntimeError, match="bound") as e:
        pol.select(np.float32([lo, lo, 400, lo, lo]), H, W)
    assert "400" in str(e.value)                                       # the per-view values are named
    with pytest.raises(RuntimeError, match="bound"):
        pol.select(np.float32([hi, hi, 400]), H, W)
    assert pol.intrinsics is None and pol.count == 0                   # select is the host half: it records nothing


def test_keyframe_store_without_intrinsics():
    from cut3r_slam_amd.keyframe import KeyFrame
    kf = KeyFrame({}, (32, 64), 12, 2, device="cpu", feat_dim=8, patch=16)
    img = torch.zeros(3, 32, 64, dtype=torch.uint8)
    assert kf.calibrated is False
    for t in range(4):
        kf.append(float(t), img, None, None, None, None, None)
    assert kf.calibrated is False and not kf.intrinsic.any()
    kf.set_intrinsics((50.0, 50.0, 32.0, 16.0))
    assert kf.calibrated is True
    assert torch.equal(kf.intrinsic[:4], torch.tensor([50.0, 50.0, 32.0, 16.0]).expand(4, 4)) and not kf.intrinsic[4:].any()
    kf.append(4.0, img, None, None, None, None, None)                  # later appends copy row 0
    assert torch.equal(kf.intrinsic[4], kf.intrinsic[0]) and not kf.intrinsic[5:].any()
    # a calibrated run is what it was: the flag rises with the first append that carries intrinsics
    kf2 = KeyFrame({}, (32, 64), 4, 2, device="cpu", feat_dim=8, patch=16)
    kf2.append(0.0, img, None, None, None, None, torch.tensor([1.0, 2.0, 3.0, 4.0]))
    assert kf2.calibrated is True and torch.equal(kf2.intrinsic[0], torch.tensor([1.0, 2.0, 3.0, 4.0]))


def test_uncalibrated_stores_are_refused_where_self_calibration_is_out_of_scope():
    import types
    from cut3r_slam_amd.dist import ShardedTracker
    from cut3r_slam_amd.keyframe import KeyFrame
    from cut3r_slam_amd.track_backend import TrackBackend
    kf = KeyFrame({}, (32, 64), 12, 2, device="cpu", feat_dim=8, patch=16)
    slam = types.SimpleNamespace(model=None, graph=None, downsample_ratio=2, keyframes=kf, tracker=types.SimpleNamespace(t1=6))
    with pytest.raises(RuntimeError, match="calibrated"):
        TrackBackend(slam, kf, {"iteration": 0}, "cpu").run()
    with pytest.raises(RuntimeError, match="calibrated"):
        ShardedTracker(slam, 1, 0).step(torch.zeros(100, 1), 0, 10, 5, None)


def test_mono_stream_without_a_calibration(tmp_path, monkeypatch):
    from PIL import Image
    from cut3r_slam_amd import ops, stream
    for i in range(2):
        Image.fromarray(np.full((60, 80, 3), 40 * i, np.uint8)).save(tmp_path / f"frame{i}.png")
    with pytest.raises(ValueError, match="undistort"):
        next(stream.mono_stream(str(tmp_path), None, undistort=True, device="cpu"))
    with pytest.raises(ValueError, match="undistort"):
        next(stream.mono_stream(str(tmp_path), undistort=True, device="cpu"))                 # calib defaults to None
    sizes = []

    def fake_resize(src, h, w, chw_out=False, out=None):               # (the resize itself is a GPU kernel: tests/test_focal_gpu.py)
        sizes.append((tuple(src.shape), h, w))
        return torch.zeros(3, h, w, dtype=torch.uint8)
    monkeypatch.setattr(ops, "resize_linear_u8", fake_resize)
    items = list(stream.mono_stream(str(tmp_path), None, cropborder=4, device="cpu"))
    assert [it[0] for it in items] == [0, 1] and [it[5] for it in items] == [False, True]
    assert all(it[2] is None and it[4] is None for it in items)
    h1, w1 = stream.tracking_size(52, 72)
    assert items[0][3].shape == (1, 3, h1, w1) and items[0][1].shape == (1, 3) + stream.mapping_size(52, 72)
    assert sizes[0] == ((52, 72, 3), h1, w1)                           # the crop comes before both resizes
    assert stream.input_size(str(tmp_path)) == (60, 80)


def test_estimated_calibration_file_round_trip(tmp_path):
    from cut3r_slam_amd import stream
    K = stream.rescale_intrinsics((400.0, 400.0, 256.0, 192.0), (384, 512), (480, 640))
    np.testing.assert_allclose(K, [500.0, 500.0, 320.0, 240.0])
    stream.save_calib(str(tmp_path / "calib_estimated.txt"), K)
    np.testing.assert_allclose(stream.load_calib(str(tmp_path / "calib_estimated.txt")), K)


def test_demo_command_line_without_calib(capsys):
    import demo
    for argv, said in ((["--imagedir", "x", "--undistort"], "--undistort needs --calib"),
                       (["--imagedir", "x", "--calib", "c.txt", "--calib-mode", "median"], "--calib-mode belongs to a run without --calib"),
                       (["--imagedir", "x", "--eval-dense", "--gtdepthdir", "g", "--gt-traj", "t"], "--calib or --gt-calib")):
        with pytest.raises(SystemExit):
            demo.main(argv)
        assert said in capsys.readouterr().err
