"""GPU: csrc/consistency.hip (multi-view depth consistency) against the numpy oracle: the counts equal, the averaged depth bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cut3r_slam_amd import _lib, ops  # noqa: E402
from cut3r_slam_amd import depth_consistency as DC  # noqa: E402
from tests import consistency_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _check(depth, w2c, K, ref, src, depth_max, **kw):
    fwd, bwd = DC.relative_rows(w2c, ref, src)
    want = O.consistency(depth, K, ref, src, fwd, bwd, depth_max, **kw)
    d, k = torch.from_numpy(depth).to(DEV), torch.from_numpy(np.ascontiguousarray(K, np.float32)).to(DEV)
    s, v, a = ops.depth_consistency(d, k, ref, src, fwd, bwd, depth_max, average=True, **kw)
    s2, v2, none = ops.depth_consistency(d, k, ref, src, fwd, bwd, depth_max, **kw)
    torch.cuda.synchronize()
    assert none is None and torch.equal(s, s2) and torch.equal(v, v2)            # the average is optional and changes nothing else
    assert s.dtype == torch.uint8 and v.dtype == torch.uint8 and a.dtype == torch.float32 and s.shape == want[0].shape
    assert np.array_equal(s.cpu().numpy(), want[0])
    assert np.array_equal(v.cpu().numpy(), want[1])
    assert np.array_equal(a.cpu().numpy().view(np.int32), want[2].view(np.int32))
    return want


def test_box_room_with_every_kind_of_invalid_pixel():
    """37 x 53 = 1961 pixels a view: 7 full blocks and a partial one.  N = 7, window 2 (S = 4 with -1 padding at the ends), per-view
    intrinsics, floaters, depths that are 0 / NaN / inf / negative / beyond depth_max, and view 5 turned by 180 degrees so that its
    neighbours' points lie behind it (Z <= z_min)"""
    n, H, W = 7, 37, 53
    g = np.random.default_rng(3)
    K = np.stack([g.uniform(38, 46, n), g.uniform(38, 46, n), 26.0 + g.uniform(-2, 2, n), 18.0 + g.uniform(-2, 2, n)], 1).astype(np.float32)
    c, Rm = O.room_cameras(n)
    Rm[5] = Rm[5] @ O.rot_yaw_pitch(np.pi, 0.0)
    depth = O.room_depth(c, Rm, K, H, W)
    depth, mask = O.inject_floaters(depth, 0.03, 1)
    depth_max = 3.2
    assert (depth > depth_max).any() and (depth < depth_max).mean() > 0.5
    flat = depth.reshape(n, -1)
    for b in range(n):
        at = g.choice(H * W, 50, replace=False)
        flat[b, at[:10]], flat[b, at[10:20]], flat[b, at[20:30]], flat[b, at[30:40]] = 0.0, np.nan, np.inf, -1.5
        flat[b, at[40:45]] = np.float32(depth_max)                               # fp32(3.2) > 3.2: beyond
        flat[b, at[45:50]] = np.nextafter(np.float32(depth_max), np.float32(0))
    src = DC.neighbour_table(n, 2)
    s, v, a = _check(depth, O.w2c_rows(c, Rm), K, np.arange(n), src, depth_max)
    ok = O.valid(depth, depth_max)
    assert not s[~ok].any() and not v[~ok].any() and not a[~ok].any()
    assert (s[:4] == 2).any() and (v > 0).any() and (s == 0)[ok].any()
    assert np.array_equal(a[ok & (s == 0)].view(np.int32), depth[ok & (s == 0)].view(np.int32))
    # view 5 looks the other way: nobody supports it, it supports nobody, and its neighbours' rows have Z < 0 there
    assert not s[5].any() and s[6].max() <= 1


def test_sixteen_sources_and_a_sub_range_of_views():
    """N = 19, window 8: S = 16, the most a launch takes; the views 3 .. 15 are checked, so ref is not the identity"""
    n, H, W = 19, 23, 31
    c, Rm = O.room_cameras(n)
    K = np.tile(np.array([24.0, 24.0, 15.0, 11.0], np.float32), (n, 1))
    depth, _ = O.inject_floaters(O.room_depth(c, Rm, K, H, W), 0.03, 2)
    table = DC.neighbour_table(n, 8)
    assert table.shape == (n, 16) and (table[9] >= 0).all()
    s, v, a = _check(depth, O.w2c_rows(c, Rm), K, np.arange(3, 16), table[3:16], 10.0, pix=1.5, rel=0.02, z_min=0.05)
    assert s.shape == (13, H, W) and s.max() > 4 and (v > 0).any()


def test_closed_form_plane_pair():
    """us lands exactly on integer coordinates and on the last column and row"""
    depth, w2c, K = O.plane_pair()
    s, v, a = _check(depth, w2c, K, np.arange(2), DC.neighbour_table(2, 1), 10.0)
    u = np.broadcast_to(np.arange(20), (6, 20))
    assert np.array_equal(s[0], (u >= 8).astype(np.uint8)) and np.array_equal(s[1], (u <= 11).astype(np.uint8)) and not v.any()


def test_refused_arguments_return_an_error_without_a_launch():
    lib = _lib.load()
    buf = torch.zeros(4096, dtype=torch.float64, device=DEV)
    p = C.c_void_p(buf.data_ptr())
    null = C.c_void_p(0)

    def call(depth=p, K=p, N=2, H=4, W=4, ref=p, src=p, R=1, S=1, fwd=p, bwd=p, depth_max=5.0, pix=1.0, rel=0.01, z_min=1e-3, sup=p, vio=p,
             avg=null):
        return lib.cut3r_depth_consistency(depth, K, N, H, W, ref, src, R, S, fwd, bwd, depth_max, pix, rel, z_min, sup, vio, avg, None)
    for name in ("depth", "K", "ref", "src", "fwd", "bwd", "sup", "vio"):
        assert call(**{name: null}) == 1, name
    assert call(S=17) == 1 and call(S=0) == 1
    assert call(R=65536) == 1 and call(R=0) == 1
    assert call(N=0) == 1 and call(H=0) == 1 and call(W=-1) == 1
    assert call(H=2 ** 14, W=2 ** 13) == 1                                      # H W = 2^31 / 16
    assert call(depth_max=0.0) == 1 and call(pix=float("nan")) == 1 and call(rel=1.0) == 1 and call(z_min=-1.0) == 1
    torch.cuda.synchronize()
    assert not buf.any()                                                         # nothing ran
    # the tables live in device memory for the kernel, so their indices are refused on the host
    d, k = torch.ones(3, 4, 4, device=DEV), torch.ones(3, 4, device=DEV)
    rows = np.zeros((1, 2, 12))
    for ref, src in (([0], [[0, 1]]), ([3], [[0, 1]]), ([0], [[1, 3]]), ([0], [[1, -2]])):
        with pytest.raises(ValueError):
            ops.depth_consistency(d, k, ref, src, rows, rows, 5.0)
    with pytest.raises(ValueError):
        ops.depth_consistency(d, k, [0], [[1] * 17], np.zeros((1, 17, 12)), np.zeros((1, 17, 12)), 5.0)
    with pytest.raises(ValueError):
        ops.depth_consistency(d.double(), k, [0], [[1, 2]], rows, rows, 5.0)
