"""GPU: self-calibration (csrc/calib.hip, cut3r_slam_amd/self_calib.py).  The Weiszfeld kernel bit for bit against the numpy oracle
(tests/focal_oracle.py), the median select against the reference's own outputs (tests/golden/focal.npz) and against torch.nanmedian on the
CPU; the edges of the launch geometry; the front end and a whole run without a calibration."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import focal_oracle as FO  # noqa: E402
from cut3r_slam_amd import ops, synth  # noqa: E402
from cut3r_slam_amd.config import tiny_config  # noqa: E402
from cut3r_slam_amd.model import Cut3rModel  # noqa: E402
from cut3r_slam_amd.self_calib import SelfCalibration, estimate_focal_knowing_depth, focal_base  # noqa: E402
from cut3r_slam_amd.slam import Cut3rSlam  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
CASES = ("patch", "offcentre", "exact", "large", "noise")


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "focal.npz"))


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def same_values(a, b):
    return np.array_equal(np.asarray(a, np.float32), np.asarray(b, np.float32), equal_nan=True)


def both_modes_equal_the_oracle(pts, pp, conf=None, conf_min=None):
    w = ops.focal_weiszfeld(dev(pts), dev(pp), conf=dev(conf), conf_min=conf_min).cpu().numpy()
    m = ops.focal_median(dev(pts), dev(pp), conf=dev(conf), conf_min=conf_min).cpu().numpy()
    w_ref, m_ref = FO.weiszfeld(pts, pp, conf=conf, conf_min=conf_min), FO.median(pts, pp, conf=conf, conf_min=conf_min)
    print("weiszfeld", w, w_ref, "median", m, m_ref)
    assert same_bits(w, w_ref), (w, w_ref)
    assert same_values(m, m_ref), (m, m_ref)
    return w, m


@pytest.mark.parametrize("name", CASES)
def test_fixture_cases(fixture, name):
    pts, pp = fixture[f"{name}_pts"], fixture[f"{name}_pp"]
    both_modes_equal_the_oracle(pts, pp)
    # through the public function (the reference's signature, its default clip): the median IS the reference's output
    med = estimate_focal_knowing_depth(dev(pts), dev(pp), focal_mode="median")
    assert med.is_cuda and med.dtype == torch.float32 and same_values(med.cpu().numpy(), fixture[f"{name}_median"])
    wz = estimate_focal_knowing_depth(dev(pts), dev(pp), focal_mode="weiszfeld").cpu().numpy()
    ref = FO.weiszfeld(pts, pp)
    assert same_values(wz, np.where(np.isnan(ref), ref, np.maximum(ref, np.float32(0))))
    base = focal_base(*pts.shape[1:3])
    clipped = estimate_focal_knowing_depth(dev(pts), dev(pp), focal_mode="weiszfeld", min_focal=0.25, max_focal=0.5).cpu().numpy()
    assert np.all((clipped >= np.float32(0.25 * base)) & (clipped <= np.float32(0.5 * base)))


def _scene(rng, B, H, W, f=None, noise=0.01):
    f = 0.8 * max(H, W) if f is None else f
    pp = np.tile(np.float32([W / 2, H / 2]), (B, 1)) + rng.uniform(-1, 1, (B, 2)).astype(np.float32)
    col = np.arange(W, dtype=np.float64)[None, None, :] - pp[:, 0, None, None]
    row = np.arange(H, dtype=np.float64)[None, :, None] - pp[:, 1, None, None]
    z = rng.uniform(1.0, 4.0, (B, H, W))
    pts = np.stack([col * z / f, row * z / f, z], -1)
    return (pts + noise * z[..., None] * rng.standard_normal(pts.shape)).astype(np.float32), pp


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (7, 24, 32), (1, 37, 53), (1, 101, 131)])
def test_generated_shapes(B, H, W):
    """1x1x1; fewer pixels than 16 x 256 threads (workgroups that own nothing); ragged ranges; several pixels per thread"""
    pts, pp = _scene(np.random.default_rng(B * 1000 + H), B, H, W)
    both_modes_equal_the_oracle(pts, pp)


def test_gated_views():
    rng = np.random.default_rng(5)
    one, pp1 = _scene(rng, 1, 96, 128)
    pts, pp = np.concatenate([one, one]), np.concatenate([pp1, pp1])
    conf = np.ones((2, 96, 128), np.float32) * 2
    drop = rng.random((96, 128)) < 0.5
    conf[1][drop] = 0.5
    w, m = both_modes_equal_the_oracle(pts, pp, conf, 1.0)
    # view 1 is view 0 on the kept subset: the estimate of a scene whose dropped pixels cast void votes / add nothing
    kept = one.copy()
    kept[0][drop] = np.nan
    assert same_bits(w[1], FO.weiszfeld(kept, pp1)[0]) and same_values(m[1], FO.median(kept, pp1)[0])
    assert not same_bits(w[0], w[1])
    # a view gated out entirely gives NaN and leaves the others alone
    conf3 = np.stack([conf[0], np.zeros_like(conf[0]), conf[1]])
    pts3, pp3 = np.concatenate([one, one, one]), np.concatenate([pp1, pp1, pp1])
    w3, m3 = both_modes_equal_the_oracle(pts3, pp3, conf3, 1.0)
    assert np.isnan(w3[1]) and np.isnan(m3[1])
    assert same_bits(w3[[0, 2]], w) and same_bits(m3[[0, 2]], m)


def _votes_scene(votes, zero_column=False):
    """a 1 x n image whose fy votes are exactly `votes` (pp = (0, -1): v = 1, y = 1, z = vote) and whose fx votes are void (x = NaN), or --
    zero_column -- repeat the vote (x = u) with the NaN vote 0 z / 0 at u = 0, x = 0"""
    votes = np.asarray(votes, np.float32)
    n = len(votes)
    pts = np.empty((1, 1, n, 3), np.float32)
    pts[0, 0, :, 0] = np.arange(n, dtype=np.float32) if zero_column else np.nan
    pts[0, 0, :, 1] = 1.0
    pts[0, 0, :, 2] = votes
    return pts, np.float32([[0.0, -1.0]])


def _crafted():
    rng = np.random.default_rng(9)
    n = 4999
    near = (np.uint32(0x42280000) + rng.integers(0, 256, n).astype(np.uint32)).view(np.float32)
    mixed = (rng.standard_normal(n) * 100).astype(np.float32)
    infs = mixed.copy()
    infs[rng.random(n) < 0.2] = np.inf
    infs[rng.random(n) < 0.2] = -np.inf
    mostly_inf = mixed.copy()
    mostly_inf[rng.random(n) < 0.7] = np.inf
    dup = np.concatenate([np.full(2400, 1.0), np.full(200, 5.0), np.full(2399, 9.0)]).astype(np.float32)
    rng.shuffle(dup)
    dup_edge = np.concatenate([np.full(2499, -3.0), np.full(2501, 7.0)]).astype(np.float32)        # rank 2499 is the first of the upper run
    with_nan = mixed.copy()
    with_nan[rng.random(n) < 0.3] = np.nan
    return {"last_pass_decides": near, "negative_last_pass": -near, "mixed_signs": mixed, "even_n": mixed[:4998], "infinities": infs,
            "median_is_inf": mostly_inf, "duplicates": dup, "duplicates_at_the_rank": dup_edge, "nan_votes": with_nan,
            "two": np.float32([3.0, -2.0]), "all_nan": np.full(17, np.nan, np.float32)}


@pytest.mark.parametrize("name", sorted(_crafted()))
def test_median_select_crafted(name):
    votes = _crafted()[name]
    want = torch.nanmedian(torch.from_numpy(votes)).numpy()              # the reference's own operator, on the CPU
    pts, pp = _votes_scene(votes)
    got = ops.focal_median(dev(pts), dev(pp)).cpu().numpy()
    print(name, got, want)
    assert same_values(got, [want]) and same_values(got, FO.median(pts, pp))
    if name == "last_pass_decides":
        assert len({int(k) >> 8 for k in votes.view(np.uint32)}) == 1 and len(set(votes.view(np.uint32) & 255)) > 100


def test_median_nan_votes_of_the_zero_column():
    """u = 0 with x = 0: the vote (0 z) / 0 is NaN and void; every other pixel votes twice"""
    votes = (np.random.default_rng(2).standard_normal(4000) * 10 + 40).astype(np.float32)
    pts, pp = _votes_scene(votes, zero_column=True)
    got = ops.focal_median(dev(pts), dev(pp)).cpu().numpy()
    u = np.arange(4000, dtype=np.float32)
    with np.errstate(all="ignore"):
        fx = (u * votes).astype(np.float32) / u                          # product rounded, IEEE division; NaN at u = 0
    assert np.isnan(fx[0]) and not np.isnan(fx[1:]).any()
    al = np.concatenate([votes, fx])
    assert same_values(got, [torch.nanmedian(torch.from_numpy(al)).numpy()]) and same_values(got, FO.median(pts, pp))


def test_batch_invariance():
    pts, pp = _scene(np.random.default_rng(3), 7, 24, 32)
    conf = np.random.default_rng(4).uniform(0, 2, (7, 24, 32)).astype(np.float32)
    for gate in (None, conf):
        cm = None if gate is None else 0.7
        w = ops.focal_weiszfeld(dev(pts), dev(pp), conf=dev(gate), conf_min=cm).cpu().numpy()
        m = ops.focal_median(dev(pts), dev(pp), conf=dev(gate), conf_min=cm).cpu().numpy()
        for i in (0, 3, 6):
            g1 = None if gate is None else dev(gate[i:i + 1])
            assert same_bits(w[i:i + 1], ops.focal_weiszfeld(dev(pts[i:i + 1]), dev(pp[i:i + 1]), conf=g1, conf_min=cm).cpu().numpy())
            assert same_bits(m[i:i + 1], ops.focal_median(dev(pts[i:i + 1]), dev(pp[i:i + 1]), conf=g1, conf_min=cm).cpu().numpy())


def test_bad_arguments_are_refused_without_a_launch():
    import ctypes as C
    from cut3r_slam_amd import _lib
    pts, pp = torch.ones(2, 8, 8, 3, device=DEV), torch.full((2, 2), 4.0, device=DEV)
    conf = torch.ones(2, 8, 8, device=DEV)
    for fn in (ops.focal_weiszfeld, ops.focal_median):
        with pytest.raises(ValueError):
            fn(pts.cpu(), pp.cpu())
        with pytest.raises(ValueError):
            fn(pts, pp.cpu())
        with pytest.raises(ValueError):
            fn(pts.half(), pp)
        with pytest.raises(ValueError):
            fn(pts.double(), pp.double())
        with pytest.raises(ValueError):
            fn(torch.ones(2, 8, 8, 6, device=DEV)[..., ::2], pp)            # not contiguous
        with pytest.raises(ValueError):
            fn(pts, pp[:1])
        with pytest.raises(ValueError):
            fn(pts, pp, conf=conf)                                          # a gate without its threshold
        with pytest.raises(ValueError):
            fn(pts, pp, conf=conf[:, :4], conf_min=1.0)
        with pytest.raises(ValueError):
            fn(pts, pp, workspace=torch.empty(64, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        ops.focal_weiszfeld(pts, pp, iters=-1)
    # the C entry points themselves: null pointers, bad sizes, a short workspace -> CUT3R_ERR_ARG (1), nothing launched
    lib = _lib.load()
    need = lib.cut3r_focal_workspace_bytes(2, 8, 8)
    assert need > 0 and lib.cut3r_focal_workspace_bytes(0, 8, 8) == -1 and lib.cut3r_focal_workspace_bytes(1, 0, 8) == -1
    assert lib.cut3r_focal_workspace_bytes(1, 32768, 32768) == -1 and lib.cut3r_focal_workspace_bytes(1, 32768, 32767) > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.full((2,), 7.0, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert lib.cut3r_focal_weiszfeld(None, None, 0.0, p(pp), 2, 8, 8, 10, p(out), p(ws), need, None) == 1
    assert lib.cut3r_focal_weiszfeld(p(pts), None, 0.0, p(pp), 2, 8, 8, 10, p(out), p(ws), need - 1, None) == 1
    assert lib.cut3r_focal_weiszfeld(p(pts), None, 0.0, p(pp), 0, 8, 8, 10, p(out), p(ws), need, None) == 1
    assert lib.cut3r_focal_median(p(pts), None, 0.0, None, 2, 8, 8, p(out), p(ws), need, None) == 1
    assert lib.cut3r_focal_median(p(pts), None, 0.0, p(pp), 2, 8, 8, p(out), None, need, None) == 1
    assert lib.cut3r_focal_median(p(pts), None, 0.0, p(pp), 2, 8, 8, p(out), p(ws), need - 1, None) == 1
    assert lib.cut3r_focal_median(p(pts), None, 0.0, p(pp), 2, 0, 8, p(out), p(ws), need, None) == 1
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.full((2,), 7.0))


# ------------------------------------------------------------------------------------------------------------------------ front end
H, W, V = 32, 48, 6


@pytest.fixture(scope="module")
def model():
    cfg = tiny_config("dpt")
    return Cut3rModel(cfg, synth.tracking_state_dict(cfg, 3), DEV, minimal=True)


def _uncalibrated_slam(model, n_kf, extra=None):
    cfgd = {"Tracking": {"motion_filter": {"thresh": 0.9, "skip": 1, "kf_every": 2}, "frontend": {"iteration": 0}}}
    cfgd["Tracking"].update(extra or {})
    slam = Cut3rSlam(model, cfgd, (H, W), buffer=40, device=DEV)
    img = torch.zeros(3, H, W, dtype=torch.uint8)
    for t in range(n_kf):
        slam.keyframes.append(float(t), img, None, None, None, None, None)
    return slam


def _identity_poses():
    enc = torch.zeros(V, 7)
    enc[:, 3] = 1.0                                                      # (t, q wxyz)
    return enc


def test_front_end_calibrates_an_uncalibrated_store(model):
    slam = _uncalibrated_slam(model, V + 1)
    kf = slam.keyframes
    assert kf.calibrated is False
    f = 32.0                                                             # exact in fp32 at every step: the estimate is 32 exactly
    col, row = np.meshgrid(np.arange(W, dtype=np.float32) - W / 2, np.arange(H, dtype=np.float32) - H / 2, indexing="xy")
    z = np.float32(2.0)
    one = np.stack([col * z / np.float32(f), row * z / np.float32(f), np.full_like(col, z)], -1)
    pts = dev(np.stack([one] * V))
    seen = []
    slam.mapper_factory = lambda *K: seen.append(K)
    slam.tracker.track(0, V, init=True, outputs=(pts, torch.ones(V, H, W, device=DEV), _identity_poses()))
    want = torch.tensor([f, f, W / 2, H / 2])
    assert kf.calibrated is True
    assert torch.equal(kf.intrinsic[:V + 1], want.expand(V + 1, 4)) and not kf.intrinsic[V + 1:].any()
    assert slam.calibration["intrinsics"] == (f, f, W / 2, H / 2) and same_values(slam.calibration["per_view"], [f] * V)
    assert seen == [(f, f, W / 2, H / 2)] and slam.tracker.calibration.count == 1
    kf.append(float(V + 1), torch.zeros(3, H, W, dtype=torch.uint8), None, None, None, None, None)
    assert torch.equal(kf.intrinsic[V + 1], want)
    # a second window on the now calibrated store estimates nothing
    slam.tracker.track(V - 1, V + 1, outputs=(pts[:2], torch.ones(2, H, W, device=DEV), _identity_poses()[:2]))
    assert slam.tracker.calibration.count == 1 and len(seen) == 1


@pytest.mark.parametrize("mode", ["weiszfeld", "median"])
def test_front_end_refuses_pointmaps_without_geometry(model, mode):
    slam = _uncalibrated_slam(model, V + 1, {"calibration": {"mode": mode}})
    pts = torch.randn(V, H, W, 3, generator=torch.Generator().manual_seed(0)).to(DEV)
    with pytest.raises(RuntimeError, match="bound"):
        slam.tracker.track(0, V, init=True, outputs=(pts, torch.ones(V, H, W, device=DEV), _identity_poses()))
    assert slam.keyframes.calibrated is False and not slam.keyframes.intrinsic.any() and slam.calibration is None
    with pytest.raises(RuntimeError, match="no view"):                   # and a window whose every pixel is gated out
        pol = SelfCalibration({"Tracking": {"calibration": {"conf_min": 2.0}}})
        pol.from_window(pts, torch.ones(V, H, W, device=DEV))


def _run(model, frames, intr, window_batch):
    cfgd = {"Tracking": {"motion_filter": {"thresh": 0.9, "skip": 1, "kf_every": 2}, "frontend": {"iteration": 0, "window_batch": window_batch}}}
    slam = Cut3rSlam(model, cfgd, (H, W), buffer=40, device=DEV)
    n = frames.shape[0]
    for t in range(n):
        slam.run(t, frames[t:t + 1], intr, frames[t:t + 1], intr, second_last_frame=(t == n - 2), last_frame=(t == n - 1))
    torch.cuda.synchronize()
    return slam


@pytest.mark.parametrize("window_batch", [1, 2])
def test_run_without_a_calibration_equals_the_run_that_is_handed_its_estimate(model, window_batch):
    frames = synth.pan_stream(48, H, W).to(DEV)
    a = _run(model, frames, None, window_batch)
    assert a.keyframes.calibrated and a.tracker.calibration.count == 1 and a.calibration is not None
    K = a.calibration["intrinsics"]
    lo, hi = a.tracker.calibration.bounds(H, W)
    print("estimated", K, "per view", a.calibration["per_view"], "bounds", lo, hi)
    assert lo < K[0] == K[1] < hi and K[2:] == (W / 2, H / 2)
    b = _run(model, frames, torch.tensor(K, dtype=torch.float32), window_batch)
    assert b.tracker.calibration.count == 0 and b.calibration is None
    n = a.keyframes.counter.value
    assert n == b.keyframes.counter.value and n >= 20 and a.tracker.t1 == b.tracker.t1 >= 16
    assert torch.equal(a.keyframes.intrinsic, b.keyframes.intrinsic) and bool(a.keyframes.intrinsic[:n].all())
    assert torch.equal(a.keyframes.pose, b.keyframes.pose)
    assert torch.equal(a.keyframes.depth[:n], b.keyframes.depth[:n]) and torch.equal(a.keyframes.submap_ds, b.keyframes.submap_ds)
    ea, eb = a.graph.edges_numpy(), b.graph.edges_numpy()
    assert len(ea[0]) > 0 and all(np.array_equal(x, y) for x, y in zip(ea, eb))


def test_mono_stream_without_a_calibration_yields_the_same_images(tmp_path):
    from PIL import Image
    from cut3r_slam_amd import stream
    rng = np.random.default_rng(0)
    for i in range(2):
        Image.fromarray(rng.integers(0, 256, (60, 80, 3), dtype=np.uint8)).save(tmp_path / f"frame{i}.png")
    cal = list(stream.mono_stream(str(tmp_path), np.float64([70.0, 70.0, 40.0, 30.0]), cropborder=2, device=DEV))
    unc = list(stream.mono_stream(str(tmp_path), None, cropborder=2, device=DEV))
    assert len(cal) == len(unc) == 2
    for c, u in zip(cal, unc):
        assert u[2] is None and u[4] is None and c[0] == u[0] and c[5] == u[5]
        assert torch.equal(c[1], u[1]) and torch.equal(c[3], u[3])


def test_demo_without_calib_writes_an_estimate_that_reproduces_the_run(tmp_path, monkeypatch, capsys):
    """demo.py without --calib on the synthetic tiny configuration of tests/test_stream_gpu.py: calib_estimated.txt is the estimate at the
    input resolution, and a second run that is handed the file writes the same trajectory and intrinsics.  Seeded random weights carry
    little geometry (their focal is a few per cent of focal_base), so this test's config widens the policy bounds; the default stays."""
    import demo
    from cut3r_slam_amd import stream
    from tests.test_stream_gpu import _write_sequence
    d = tmp_path / "colors"
    d.mkdir()
    _write_sequence(str(d), 36)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("Tracking:\n  calibration:\n    min_focal: 0.0001\n    max_focal: 1000.0\n")
    base = ["--imagedir", str(d), "--config", str(cfg), "--kf_every", "2", "--synthetic-weights", "--small", "--seed", "1"]
    seen = []
    real = stream.save_trajectory
    monkeypatch.setattr(stream, "save_trajectory", lambda slam, *a, **k: seen.append(slam) or real(slam, *a, **k))
    a = tmp_path / "a"
    assert demo.main(base + ["--output", str(a)]) == 0
    assert "self-calibration (weiszfeld)" in capsys.readouterr().out
    slam = seen[0]
    fx, fy, cx, cy = slam.calibration["intrinsics"]
    assert slam.tracker.calibration.count == 1 and (cx, cy) == (256.0, 192.0) and (slam.keyframes.ht, slam.keyframes.wd) == (384, 512)
    est = stream.load_calib(str(a / "calib_estimated.txt"))
    np.testing.assert_array_equal(est, [fx * 640 / 512, fy * 480 / 384, 320.0, 240.0])
    np.testing.assert_array_equal(np.load(a / "intrinsics.npy"), np.float32([fx, fy, cx, cy]))
    b = tmp_path / "b"
    assert demo.main(base + ["--output", str(b), "--calib", str(a / "calib_estimated.txt")]) == 0
    assert seen[1].calibration is None and not (b / "calib_estimated.txt").exists()
    assert (a / "traj_kf.txt").read_bytes() == (b / "traj_kf.txt").read_bytes()
    np.testing.assert_array_equal(np.load(a / "intrinsics.npy"), np.load(b / "intrinsics.npy"))
