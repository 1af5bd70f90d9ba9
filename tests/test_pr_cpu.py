"""CPU: the precision / recall oracle (tests/pr_oracle.py) against numpy, sim3_from_moments against eval_ate.umeyama, the colour rule, the
command line and the result file the reference's run scripts read."""
import ast
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cut3r_slam_amd import eval_recon as ER  # noqa: E402
from cut3r_slam_amd.eval_ate import umeyama  # noqa: E402
from tests import pr_oracle as PO  # noqa: E402
from tests import recon_oracle as RO  # noqa: E402


@pytest.mark.parametrize("Q", [1, 257, 5000, 70001])
def test_oracle_bins_are_numpys_away_from_the_last_edge(Q):
    rng = np.random.default_rng(Q)
    tau, w, nbins = 0.05, 5e-4, 500
    d2 = (rng.uniform(0, 0.2499, Q).astype(np.float32)) ** 2            # d < 0.2499 < nbins w = 0.25: the last edge is never met
    d2[::7] = np.float32(1.0)                                           # beyond the last edge: no bin
    counts, moments, hist = PO.dist_stats(d2, tau, w, nbins)
    d = np.sqrt(d2.astype(np.float64))
    ref, _ = np.histogram(d, np.arange(0, nbins + 1) * w)
    assert np.array_equal(hist, ref)
    assert counts.tolist() == [Q, int((d < tau).sum()), 0]
    assert moments[2] == d.min() and moments[3] == d.max()
    fs = PO.fsum_sums(d2)
    assert abs(moments[0] - fs[0]) <= (Q - 1) * 2.0 ** -53 * fs[0] and abs(moments[1] - fs[1]) <= (Q - 1) * 2.0 ** -53 * fs[1]


def test_oracle_bin_rule_at_the_edges():
    w, nbins = 2.0 ** -9, 640
    k = np.array([0, 1, 5, 639, 640, 700])
    d = k * w
    got, inside = PO.bin_index(d, w, nbins)
    assert np.array_equal(got[inside], k[:4]) and inside.tolist() == [True] * 4 + [False] * 2
    below = np.nextafter(d[1:], 0)
    got, inside = PO.bin_index(below, w, nbins)
    assert np.array_equal(got[:4], k[1:5] - 1) and inside.tolist() == [True] * 4 + [False]
    # a width that is not a power of two: the bin is the largest k with fl(k w) <= d, which np.histogram's searchsorted over the same
    # products gives as well
    w = 5e-4
    d = np.concatenate([np.arange(500) * w, np.nextafter(np.arange(1, 500) * w, 0)])
    got, inside = PO.bin_index(d, w, 500)
    assert inside.all() and np.array_equal(got, np.searchsorted(np.arange(501) * w, d, side="right") - 1)


@pytest.mark.parametrize("Q", [1, 2, 3, 4, 255, 256, 70001])
def test_oracle_median_is_numpys(Q):
    rng = np.random.default_rng(Q)
    d2 = rng.uniform(0, 4, Q).astype(np.float32)
    m = PO.median_ranks(d2)
    assert 0.5 * (float(m[0]) + float(m[1])) == float(np.median(d2.astype(np.float64)))
    bad = np.concatenate([d2, np.float32([np.nan, -1, np.inf])])
    assert np.array_equal(PO.median_ranks(rng.permutation(bad)), m)
    assert np.isnan(PO.median_ranks(np.float32([np.nan, -2]))).all()


def _moments_of(src, dst):
    m = np.zeros(18)
    m[0] = len(src)
    m[2:5], m[5:8] = src.sum(0), dst.sum(0)
    m[8:17] = (src[:, :, None] * dst[:, None, :]).sum(0).reshape(9)
    m[17] = (src * src).sum()
    return m


@pytest.mark.parametrize("seed", range(6))
def test_sim3_from_moments_is_umeyama_with_scale(seed):
    # centred clouds of extent ~1 and ~10^3 points: fp64 rounding of ~10^3 terms (1e-13) times the O(10) cancellation of the variance
    rng = np.random.default_rng(seed)
    src = rng.uniform(-0.5, 0.5, (1000, 3))
    src -= src.mean(0)
    s, R, t = 0.5 + rng.uniform(0, 1.5), RO.rot(rng.normal(size=3), rng.uniform(0, 3)), rng.uniform(-0.2, 0.2, 3)
    dst = s * src @ R.T + t + rng.normal(scale=0.01, size=src.shape)
    M = ER.sim3_from_moments(_moments_of(src, dst))
    su, Ru, tu = umeyama(src, dst, with_scale=True)
    assert np.abs(M[:3, :3] - su * Ru).max() < 1e-12 and np.abs(M[:3, 3] - tu).max() < 1e-12
    assert abs(np.cbrt(np.linalg.det(M[:3, :3])) - su) < 1e-12 and abs(su - s) < 0.01
    assert np.abs(PO.sim3_fit(src, dst) - M).max() < 1e-12
    # no correspondence: identity; coincident source points: no scale to estimate
    assert np.array_equal(ER.sim3_from_moments(np.zeros(18)), np.eye(4))
    one = np.tile(src[:1], (5, 1))
    assert abs(np.linalg.det(ER.sim3_from_moments(_moments_of(one, dst[:5]))[:3, :3]) - 1) < 1e-9


def test_colour_rule_at_the_ends_and_the_breakpoints():
    tau = 0.05
    x = np.array([0.0, 1 - 0.746032, 1 - 0.365079, 1.0, 2.0])            # 2: clipped to 1
    c = ER.error_colors(x * 3 * tau, tau).numpy()
    assert c.tolist() == [[255, 255, 255], [255, 255, 0], [255, 0, 0], [11, 0, 0], [11, 0, 0]]       # floor(255 * 0.0416 + 0.5) = 11
    mid = ER.error_colors(np.array([0.5 * (1 - 0.746032) * 3 * tau]), tau).numpy()
    assert mid.tolist() == [[255, 255, 128]]


def test_cli_parsing():
    a = ER.parse_args(["rec.ply", "gt.ply"])
    assert (a.pr, a.pr_thresh, a.pr_scale, a.pr_out) == (False, 0.05, False, None)
    a = ER.parse_args(["rec.ply", "gt.ply", "--eval_3d", "--pr", "--pr-thresh", "0.1", "--pr-scale", "--pr-out", "d", "--save", "f.txt"])
    assert (a.pr, a.pr_thresh, a.pr_scale, a.pr_out, a.save) == (True, 0.1, True, "d", "f.txt")
    for bad in (["--pr-scale"], ["--pr-out", "d"], ["--pr", "--pr-thresh", "0"], ["--pr", "--pr-thresh", "nan"]):
        with pytest.raises(SystemExit):
            ER.parse_args(["rec.ply", "gt.ply"] + bad)


def _result():
    edges = np.arange(501) * 5e-4
    cum = np.linspace(0, 1, 500)
    side = (0.011, 0.010, 0.004, 0.0, 0.09)
    return ER.PRResult(0.9, 0.8, 2 * 0.9 * 0.8 / 1.7, *side, *side, edges, cum, cum, None, None, None, None)


def test_result_round_trips_and_feeds_the_run_script():
    result = {"accuracy": 1.0, "completion": 2.0, "completion_ratio": 99.0}
    result.update(ER.pr_dict(_result()))
    assert all(type(v) is float for v in result.values())
    back = ast.literal_eval(f"{result}")
    assert back == result
    # scripts/run_replica.py:54-57
    metrics = {"accu": 0.0, "comp": 0.0, "compr": 0.0}
    metrics['accu'] += back['mean precision']
    metrics['comp'] += back['mean recall']
    metrics['compr'] += back['recall']
    line = f"- acc: {back['mean precision']:.3f}, comp: {back['mean recall']:.3f}, comp rat: {back['recall']:.3f}\n"
    assert line == "- acc: 1.100, comp: 1.100, comp rat: 80.000\n" and metrics["compr"] == 80.0
    assert set(back) >= {"precision", "recall", "f-score", "mean precision", "mean recall", "median precision", "median recall"}
    assert math.isclose(back["f-score"], 200 * 0.72 / 1.7)


def test_oracle_recovers_the_scale_of_a_sphere_pair():
    """the conditions tests/test_pr_e2e_gpu.py puts on run_evaluation, checked on the oracle alone: between 4000 samples of two icospheres
    of radius 1.02 and 1, at PO.SPHERE_TAU, precision = recall = 1 as they come, and the coarse-to-fine ICP with scale recovers 1 / 1.02
    within 1 % (the oracle gives 0.1 %)"""
    (vr, fr), (vg, fg) = RO.icosphere(3, 1.02), RO.icosphere(3, 1.0)
    rec = RO.sample(vr, fr, np.cumsum(RO.face_areas(vr, fr).astype(np.float64)), 4000, seed=0, stream=1)
    gt = RO.sample(vg, fg, np.cumsum(RO.face_areas(vg, fg).astype(np.float64)), 4000, seed=0, stream=2)
    res = PO.precision_recall(rec, gt, PO.SPHERE_TAU)
    assert res["precision"] == 1.0 and res["recall"] == 1.0
    M = PO.align_coarse_to_fine(rec, gt, PO.SPHERE_TAU, with_scaling=True)
    s = np.cbrt(np.linalg.det(M[:3, :3]))
    assert abs(s * 1.02 - 1) < 0.01, s
    res = PO.precision_recall(PO.transform_points(rec, M), gt, PO.SPHERE_TAU)
    assert res["precision"] == 1.0 and res["recall"] == 1.0 and res["rec"]["mean"] < 0.1
