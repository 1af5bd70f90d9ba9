"""GPU: the panel, frame and range kernels of csrc/gs_panel.hip against the numpy oracle (tests/gs_panel_oracle.py), every byte.  Shapes: all
border (1x1, 2x2), one interior pixel (3x3), small (5x7), odd unaligned rows (33x47: byte stores, a partly filled last thread of a row),
and rows that are a multiple of four pixels (64x96: the dword stores)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import gs_panel_oracle as O  # noqa: E402
from cut3r_slam_amd import _lib, ops  # noqa: E402

DEV = "cuda:0"
SHAPES = [(1, 1), (2, 2), (3, 3), (5, 7), (33, 47), (64, 96)]
CASES = ["generic", "same_depth", "alpha_low", "alpha_high", "out_of_range", "exposure", "off_centre"]


def _inputs(H, W, case, seed=0):
    g = np.random.default_rng(seed + 1000 * H + W)
    f = lambda *s: g.random(s).astype(np.float32)
    d = {"gt": f(3, H, W), "render": f(3, H, W), "A": np.eye(3, dtype=np.float32), "b": np.zeros(3, np.float32),
         "gt_depth": 0.5 + 4 * f(H, W), "depth": 0.5 + 4 * f(H, W), "normal": 2 * f(3, H, W) - 1, "alpha": f(H, W),
         "K": (0.9 * W, 1.1 * W, 0.5 * W, 0.5 * H)}
    d["gt_depth"][g.random((H, W)) < 0.2] = 0.0                            # some exact zeros (invalid depth) in every case
    d["depth"][g.random((H, W)) < 0.1] = 0.0
    if case == "same_depth":
        d["depth"] = d["gt_depth"].copy()
    elif case == "alpha_low":
        d["alpha"] = (0.5 * d["alpha"]).astype(np.float32)                 # <= 0.5: nothing is above the threshold
    elif case == "alpha_high":
        d["alpha"] = (0.5 + 0.5 * d["alpha"] + np.float32(1e-3)).astype(np.float32)
    elif case == "out_of_range":
        d["render"] = (40 * d["render"] - 20).astype(np.float32)
        d["normal"] = (1e3 * d["normal"]).astype(np.float32)
        d["gt"][0] = -d["gt"][0]
    elif case == "exposure":
        d["A"] = (np.eye(3) + 0.3 * (g.random((3, 3)) - 0.5)).astype(np.float32)
        d["b"] = (0.2 * (g.random(3) - 0.5)).astype(np.float32)
    elif case == "off_centre":
        d["K"] = (0.9 * W, 1.1 * W, 0.31 * W + 0.123, 0.77 * H - 0.456)
    return d


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("H,W", SHAPES)
def test_panel_equals_the_oracle_in_every_byte(H, W, case):
    d = _inputs(H, W, case)
    want = O.panel(d["gt"], d["render"], d["A"], d["b"], d["gt_depth"], d["depth"], d["normal"], d["alpha"], *d["K"])
    got = ops.gs_panel(_gpu(d["gt"]), _gpu(d["render"]), _gpu(d["A"]), _gpu(d["b"]), _gpu(d["gt_depth"]), _gpu(d["depth"])[None],
                       _gpu(d["normal"]), _gpu(d["alpha"])[None], *d["K"]).cpu().numpy()
    assert got.shape == (3 * H, 3 * W, 3) and got.dtype == np.uint8
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} bytes differ, first at (row, col, channel) {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"
    if case == "same_depth":                                               # the difference map is constant: TURBO_U8[0] everywhere
        assert (got[H:2 * H, 2 * W:] == O.TURBO_U8[0]).all()
    if case in ("alpha_low", "alpha_high"):
        assert (got[2 * H:, 2 * W:] == O.TURBO_U8[0]).all()
    if H >= 3 and W >= 3:                                                  # border 128, and the interior is not all border
        cell = got[2 * H:, W:2 * W]
        assert (cell[0] == 128).all() and (cell[-1] == 128).all() and (cell[:, 0] == 128).all() and (cell[:, -1] == 128).all()
        assert H < 5 or (cell[1:-1, 1:-1] != 128).any()


@pytest.mark.parametrize("H,W", [(5, 7), (33, 47)])
def test_frame_layers_equal_the_oracle(H, W):
    d = _inputs(H, W, "out_of_range", seed=5)
    for layer, src in (("rgb", d["render"]), ("normal", d["normal"])):
        got = ops.gs_frame(_gpu(src), layer).cpu().numpy()
        assert np.array_equal(got, O.frame(src, layer)), layer
    depth = d["depth"]
    assert np.array_equal(ops.gs_frame(_gpu(depth), "depth").cpu().numpy(), O.frame(depth, "depth"))
    assert np.array_equal(ops.gs_frame(_gpu(depth)[None], "depth").cpu().numpy(), O.frame(depth, "depth"))
    lo, hi = 1.0, 3.0                                                      # a fixed range with depths on both sides of it
    assert (depth < lo).any() and (depth > hi).any()
    got = ops.gs_frame(_gpu(depth), "depth", (lo, hi)).cpu().numpy()
    assert np.array_equal(got, O.frame(depth, "depth", (lo, hi)))
    assert (got[depth <= lo] == O.TURBO_U8[0]).all() and (got[depth >= hi] == O.TURBO_U8[255]).all()
    const = np.full((H, W), 2.5, np.float32)                               # hi == lo: TURBO_U8[0], as in the reference
    assert (ops.gs_frame(_gpu(const), "depth").cpu().numpy() == O.TURBO_U8[0]).all()


def test_bad_arguments_are_refused_without_a_launch():
    lib = _lib.load()
    t = torch.zeros(3 * 4 * 4, device=DEV)
    r = torch.zeros(8, dtype=torch.int32, device=DEV)
    o = torch.zeros(27 * 16, dtype=torch.uint8, device=DEV)
    p = lambda x: C.c_void_p(x.data_ptr())
    ok = [p(t)] * 8 + [1.0, 1.0, 0.0, 0.0]
    assert lib.cut3r_gs_panel(*ok, 0, 4, p(r), p(o), None) == 1            # H = 0
    assert lib.cut3r_gs_panel(*ok, 4, 0, p(r), p(o), None) == 1
    assert lib.cut3r_gs_panel(*ok, -1, 4, p(r), p(o), None) == 1
    for k in range(8):                                                     # each input pointer
        args = list(ok)
        args[k] = None
        assert lib.cut3r_gs_panel(*args, 4, 4, p(r), p(o), None) == 1
    assert lib.cut3r_gs_panel(*ok, 4, 4, None, p(o), None) == 1
    assert lib.cut3r_gs_panel(*ok, 4, 4, p(r), None, None) == 1
    assert lib.cut3r_gs_frame(None, 0, 4, 4, None, 0.0, 1.0, p(o), None) == 1
    assert lib.cut3r_gs_frame(p(t), 0, 4, 4, None, 0.0, 1.0, None, None) == 1
    assert lib.cut3r_gs_frame(p(t), 3, 4, 4, None, 0.0, 1.0, p(o), None) == 1
    assert lib.cut3r_gs_frame(p(t), 0, 0, 4, None, 0.0, 1.0, p(o), None) == 1
    assert lib.cut3r_gs_panel_ranges(None, None, None, 16, p(r), None) == 1
    assert lib.cut3r_gs_panel_ranges(p(t), None, None, 0, p(r), None) == 1
    assert lib.cut3r_gs_panel_ranges(p(t), None, None, 16, None, None) == 1
    with pytest.raises(ValueError):
        ops.gs_panel(*[torch.zeros(3, 0, 4, device=DEV)] * 8, 1.0, 1.0, 0.0, 0.0)
    with pytest.raises(ValueError):
        ops.gs_frame(torch.zeros(3, 4, 4), "rgb")                          # a CPU tensor


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, 300001])
def test_ranges_equal_numpys_exactly(n):
    """min / max are exact: the four maps' ranges equal numpy's bit for bit (300001 elements: more workgroups than one pass of the grid)"""
    g = np.random.default_rng(n)
    a = (10 * g.standard_normal(n)).astype(np.float32)                     # negative values
    b = np.full(n, -3.25, np.float32)                                      # all equal
    alpha = g.random(n).astype(np.float32)
    r = ops.gs_panel_ranges_decode(ops.gs_panel_ranges(_gpu(a), _gpu(b), _gpu(alpha)))
    diff, mask = np.abs(a - b), (alpha > np.float32(0.5)).astype(np.float32)
    want = np.array([[m.min(), m.max()] for m in (a, b, diff, mask)], np.float32)
    assert np.array_equal(r.view(np.uint32), want.view(np.uint32)), (r, want)
    only = ops.gs_panel_ranges_decode(ops.gs_panel_ranges(_gpu(-np.abs(a))))   # one map, all negative: the other slots stay unset
    assert only[0, 0] == -np.abs(a).max() and only[0, 1] == -np.abs(a).min() and np.isnan(only[1:]).all()
