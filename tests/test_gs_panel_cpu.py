"""CPU: the yardstick of the panel kernels.  The committed turbo byte table (csrc/turbo_u8.h) against matplotlib's, and the numpy oracle
(tests/gs_panel_oracle.py) against bytes worked out by hand on a 3 x 3 view."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gs_panel_oracle as O  # noqa: E402


def test_committed_turbo_table_is_matplotlibs():
    matplotlib = pytest.importorskip("matplotlib")
    T = np.asarray(matplotlib.colormaps["turbo"].colors, np.float64)
    assert T.shape == (256, 3)
    assert np.array_equal(O.TURBO_U8, np.floor(T * 255 + 0.5).astype(np.uint8))
    from cut3r_slam_amd import ops
    assert np.array_equal(ops.turbo_u8(), O.TURBO_U8)                     # the package reads the same file


def test_oracle_on_a_3x3_view_by_hand():
    """fx = fy = 1, cx = cy = 1: the rays are (-1, 0, 1) both ways.
    render depth d = 1, 2, 3 along x: at the centre a = p(2,1) - p(0,1) = (3,0,3) - (-1,0,1) = (4,0,2), b = p(1,2) - p(1,0) = (0,2,2) -
    (0,-2,2) = (0,4,0), a x b = (-8, 0, 16), |.| = sqrt(320), n = (-0.44721, 0, 0.89443), (n + 1) / 2 = (0.27639, 0.5, 0.94721) ->
    floor(70.98), floor(128.0), floor(242.04) = (70, 128, 242); every border pixel (0 + 1) / 2 -> 128.
    turbo(d): lo 1, hi 3, den fp32(2 + 1e-10) = 2, q = 0, 0.5, 1 -> index 0, int(127.5) = 127, 255.
    gt depth constant 2: hi == lo, q = 0 / fp32(1e-10) = 0 -> TURBO_U8[0] everywhere.  |2 - d| = 1, 0, 1 -> index 255, 0, 255.
    alpha 0.9 but 0.2 at (0,0), and 0.5 itself at (2,2) is NOT above 0.5: mask 0 there, 1 elsewhere -> index 0 / 255.
    render r = (0.2, 0.4, 0.35); A = [[1,0,0],[.5,1,0],[0,0,2]], b = (.1, 0, -.1): e = (0.2 + 0.2 + 0.1, 0.4, 0.7 - 0.1) = (0.5, 0.4, 0.6).
    gt (0.5, 0.42, 0.95): bytes floor(128.0), floor(107.6), floor(242.75) = (128, 107, 242); error (0, 0.2, 3.5) -> (0, floor(51.5), 255);
    gt (2, -1, 0.25) at (0,0): bytes (255, 0, floor(64.25)) = (255, 0, 64); error (15, 14, 3.5) -> saturated (255, 255, 255).
    render bytes floor(51.5), floor(102.5), floor(89.75) = (51, 102, 89).
    render normal (0, 0, -1) -> (128, 128, 0); (3, -3, 0.5) at (1,2) -> (255, 0, floor(191.75)) = (255, 0, 191)."""
    H = W = 3
    d = np.tile(np.array([1.0, 2.0, 3.0], np.float32), (3, 1))
    gt_depth = np.full((3, 3), 2.0, np.float32)
    alpha = np.full((3, 3), 0.9, np.float32)
    alpha[0, 0], alpha[2, 2] = 0.2, 0.5
    render = np.empty((3, 3, 3), np.float32)
    render[0], render[1], render[2] = 0.2, 0.4, 0.35
    A = np.array([[1, 0, 0], [0.5, 1, 0], [0, 0, 2]], np.float32)
    b = np.array([0.1, 0.0, -0.1], np.float32)
    gt = np.empty((3, 3, 3), np.float32)
    gt[0], gt[1], gt[2] = 0.5, 0.42, 0.95
    gt[:, 0, 0] = (2.0, -1.0, 0.25)
    normal = np.zeros((3, 3, 3), np.float32)
    normal[2] = -1.0
    normal[:, 1, 2] = (3.0, -3.0, 0.5)
    out = O.panel(gt, render, A, b, gt_depth, d, normal, alpha, 1.0, 1.0, 1.0, 1.0)
    assert out.shape == (9, 9, 3) and out.dtype == np.uint8
    cell = lambda r, c: out[3 * r:3 * r + 3, 3 * c:3 * c + 3]
    T0, T127, T255 = (48, 18, 59), (161, 253, 61), (122, 4, 3)            # the table's own entries, literally
    assert tuple(O.TURBO_U8[0]) == T0 and tuple(O.TURBO_U8[127]) == T127 and tuple(O.TURBO_U8[255]) == T255

    def expect(img, default, **special):
        want = np.empty((3, 3, 3), np.uint8)
        want[:] = default
        for k, v in special.items():
            want[int(k[1]), int(k[2])] = v
        assert np.array_equal(img, want), (img.tolist(), want.tolist())
    expect(cell(0, 0), (128, 107, 242), p00=(255, 0, 64))
    expect(cell(0, 1), (51, 102, 89))
    expect(cell(0, 2), (0, 51, 255), p00=(255, 255, 255))
    expect(cell(1, 0), T0)
    assert np.array_equal(cell(1, 1), np.array([[T0, T127, T255]] * 3, np.uint8))
    assert np.array_equal(cell(1, 2), np.array([[T255, T0, T255]] * 3, np.uint8))
    expect(cell(2, 0), (128, 128, 0), p12=(255, 0, 191))
    expect(cell(2, 1), (128, 128, 128), p11=(70, 128, 242))
    expect(cell(2, 2), T255, p00=T0, p22=T0)
    # the frame layers are the same cells; a fixed range clips what lies outside it: (d - 1.5) / fp32(1 + 1e-10) = -0.5, 0.5, 1.5
    assert np.array_equal(O.frame(render, "rgb"), cell(0, 1)) and np.array_equal(O.frame(normal, "normal"), cell(2, 0))
    assert np.array_equal(O.frame(d, "depth"), cell(1, 1))
    assert np.array_equal(O.frame(d[None], "depth", (1.5, 2.5)), np.array([[T0, T127, T255]] * 3, np.uint8))


def test_oracle_depth_normal_is_the_mappers():
    """the oracle's normal is gs_mapper.depth_to_normal (what the normal loss uses), up to the rounding of torch's normalise"""
    import torch
    from cut3r_slam_amd import gs_mapper as GM

    class View:
        fx, fy, cx, cy = 31.5, 29.0, 4.25, 2.75
    g = np.random.default_rng(0)
    d = (1.0 + g.random((6, 9))).astype(np.float32)
    ours = O.depth_normal(d, View.fx, View.fy, View.cx, View.cy)
    ref = GM.depth_to_normal(View(), torch.from_numpy(d)[None]).numpy()
    assert ours.shape == ref.shape == (3, 6, 9)
    assert not ours[:, 0].any() and not ours[:, -1].any() and not ours[:, :, 0].any() and not ours[:, :, -1].any()
    assert np.abs(ours - ref).max() < 1e-6
