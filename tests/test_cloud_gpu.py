"""GPU: csrc/cloud.hip (depth maps -> world point cloud, voxel downsample) against the numpy oracle, bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cut3r_slam_amd import _lib, ops  # noqa: E402
from tests import cloud_oracle as CO  # noqa: E402
from tests import recon_oracle as RO  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRUNC = 4.5


def _poses(B, seed, scale=1.7, shift=1e3):
    g = np.random.default_rng(seed)
    out = np.zeros((B, 12))
    for b in range(B):
        out[b] = np.concatenate([scale * RO.rot(g.normal(size=3), g.uniform(0, 3)), g.uniform(-shift, shift, (3, 1))], 1).reshape(-1)
    return out


def _views(B, H, W, seed):
    """depths in (0.3, 6) with every kind of invalid pixel, colours, scaled poses far from the origin, per-view intrinsics"""
    g = np.random.default_rng(seed)
    d = g.uniform(0.3, 6.0, (B, H, W)).astype(np.float32)
    flat = d.reshape(B, -1)
    for b in range(B):
        at = g.choice(H * W, 60, replace=False)
        flat[b, at[:10]] = 0.0
        flat[b, at[10:20]] = -1.5
        flat[b, at[20:30]] = np.nan
        flat[b, at[30:40]] = np.inf
        flat[b, at[40:50]] = np.float32(TRUNC)
        flat[b, at[50:60]] = np.nextafter(np.float32(TRUNC), np.float32(0))
    rgb = g.integers(0, 256, (B, 3, H, W), dtype=np.uint8)
    K = np.stack([g.uniform(40, 60, B), g.uniform(40, 60, B), g.uniform(0.4, 0.6, B) * W, g.uniform(0.4, 0.6, B) * H], 1)
    return d, rgb, _poses(B, seed + 1), K


def _run(d, c2w, K, size=None, rgb=None, trunc=TRUNC):
    p, c, n = ops.depth_cloud(torch.from_numpy(d).to(DEV), c2w, K, trunc, size=size, rgb=None if rgb is None else torch.from_numpy(rgb).to(DEV))
    torch.cuda.synchronize()
    return p.cpu().numpy(), None if c is None else c.cpu().numpy(), n.cpu().numpy()


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                                                        b.view(np.uint32) if b.dtype == np.float32 else b)


@pytest.mark.parametrize("size", [None, (7, 9), (50, 71), (37, 53)])
def test_depth_cloud_matches_the_oracle(size):
    d, rgb, c2w, K = _views(3, 37, 53, 0)                    # 1961 pixels a view: 8 blocks, the last one partial
    d[1] = np.where(np.arange(37 * 53).reshape(37, 53) % 2 == 0, 0.0, np.float32(TRUNC))     # a view without a valid pixel
    want = CO.backproject(d, c2w, K, TRUNC, size=size, rgb=rgb)
    got = _run(d, c2w, K, size=size, rgb=rgb)
    assert want[2][1] == 0 and want[2][0] > 0 and want[2][2] > 0
    assert all(_same(a, b) for a, b in zip(got, want))
    assert got[2].sum() == len(got[0]) and got[2].dtype == np.int64
    no_rgb = _run(d, c2w, K, size=size)
    assert no_rgb[1] is None and _same(no_rgb[0], want[0]) and _same(no_rgb[2], want[2])
    again = _run(d, c2w, K, size=size, rgb=rgb)
    assert all(_same(a, b) for a, b in zip(got, again))
    if size is None:
        # the pixels at exactly depth_trunc are out, the float just below is in
        assert got[2][0] == np.count_nonzero(np.isfinite(d[0]) & (d[0] > 0) & (d[0] < np.float32(TRUNC)))
        assert np.count_nonzero(d[0] == np.nextafter(np.float32(TRUNC), np.float32(0))) == 10


def test_sixteen_views_in_one_launch_equal_sixteen_launches_and_seventeen_go_through():
    d, rgb, c2w, K = _views(17, 12, 20, 2)
    one = _run(d[:16], c2w[:16], K[:16], rgb=rgb[:16])
    parts = [_run(d[b:b + 1], c2w[b:b + 1], K[b:b + 1], rgb=rgb[b:b + 1]) for b in range(16)]
    assert _same(one[0], np.concatenate([p[0] for p in parts])) and _same(one[1], np.concatenate([p[1] for p in parts]))
    assert _same(one[2], np.concatenate([p[2] for p in parts]))
    all17 = _run(d, c2w, K, rgb=rgb)
    want = CO.backproject(d, c2w, K, TRUNC, rgb=rgb)
    assert all(_same(a, b) for a, b in zip(all17, want)) and len(all17[2]) == 17 and all17[2][16] > 0
    shared_K = _run(d, c2w, K[0])
    assert _same(shared_K[0], CO.backproject(d, c2w, K[0], TRUNC)[0])


def test_all_views_empty():
    p, c, n = _run(np.zeros((2, 5, 6), np.float32), _poses(2, 0), [50.0, 50.0, 3.0, 2.0], rgb=np.zeros((2, 3, 5, 6), np.uint8))
    assert p.shape == (0, 3) and c.shape == (0, 3) and n.tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------------------------ downsample
def _down(p, voxel, col=None):
    out = ops.voxel_downsample(torch.from_numpy(p).to(DEV), voxel, None if col is None else torch.from_numpy(col).to(DEV))
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in out)


def _check_down(p, voxel, col=None):
    want = CO.voxel_downsample(p, voxel, col)
    got = _down(p, voxel, col)
    assert got[2].dtype == np.int32 and got[2].sum() == len(p)
    for a, b in zip(got, want):
        assert (a is None and b is None) or _same(a, b)
    again = _down(p, voxel, col)
    for a, b in zip(got, again):
        assert (a is None and b is None) or _same(a, b)
    return got


def test_downsample_one_point():
    p = np.array([[0.3, -2.0, 7.5]], np.float32)
    out, col, cnt = _check_down(p, 0.05, np.array([[1, 2, 255]], np.uint8))
    assert _same(out, p) and col.tolist() == [[1, 2, 255]] and cnt.tolist() == [1]


def test_downsample_a_run_longer_than_a_block():
    g = np.random.default_rng(0)
    p = np.concatenate([g.uniform(0.02, 0.06, (3000, 3)), [[-0.01, -0.01, -0.01], [0.3, 0.3, 0.3]]]).astype(np.float32)   # cells start at -0.035
    out, _, cnt = _check_down(p, 0.05, g.integers(0, 256, (3002, 3), dtype=np.uint8))
    assert sorted(cnt.tolist()) == [1, 1, 3000]


def test_downsample_points_on_voxel_faces_and_negative_coordinates():
    g = np.random.default_rng(1)
    k = g.integers(-40, 40, (2000, 3))
    p = (k * 0.05).astype(np.float32)                        # on the faces of the 0.05 grid, half of them negative
    p = np.concatenate([p, p[:300] + np.float32(1e-7), -np.abs(g.normal(size=(200, 3))).astype(np.float32)])
    _check_down(p, 0.05)
    _check_down(p, 0.1)


def test_downsample_seeded_cloud_with_colours():
    g = np.random.default_rng(2)
    centres = g.uniform(-1, 1, (60, 3))
    n = g.integers(1, 100, 60)
    p = np.concatenate([c + g.uniform(-0.02, 0.02, (m, 3)) for c, m in zip(centres, n)])
    p = np.concatenate([p, g.uniform(-1, 1, (5000 - len(p), 3))]).astype(np.float32)[g.permutation(5000)]
    col = g.integers(0, 256, (5000, 3), dtype=np.uint8)
    out, c, cnt = _check_down(p, 0.05, col)
    assert cnt.min() == 1 and cnt.max() > 30 and len(cnt) > 1000
    # a shuffled input: the same voxels and counts; the means are sums in another order and may differ in the last bit
    perm = g.permutation(5000)
    out2, c2, cnt2 = _down(p[perm], 0.05, col[perm])
    assert np.array_equal(cnt, cnt2) and np.abs(out.astype(np.float64) - out2).max() <= 2.0 ** -22 and np.abs(c.astype(int) - c2).max() <= 1
    print(f"shuffled: {np.count_nonzero(out != out2)} of {out.size} mean coordinates differ in the last bit")


def test_downsample_index_limit():
    voxel = 0.5
    top = lambda x: np.array([[0.0, 0.0, 0.0], [x, 0.0, 0.0]], np.float32)
    ok = np.float32((2 ** 21 - 1.25) * voxel)                # floor((x + voxel / 2) / voxel) = 2^21 - 1
    bad = np.float32((2 ** 21 - 0.5) * voxel)                # ... = 2^21
    assert CO.voxel_keys(top(ok), voxel)[0].max() == 2 ** 21 - 1
    out, _, cnt = _check_down(top(ok), voxel)
    assert len(out) == 2
    with pytest.raises(ValueError, match="2\\^21"):
        _down(top(bad), voxel)
    for axis in (1, 2):
        with pytest.raises(ValueError, match="2\\^21"):
            _down(np.roll(top(bad), axis, 1), voxel)


# ------------------------------------------------------------------------------------------------------------------- refusals
def test_ops_refuse_bad_arguments():
    d = torch.ones(2, 4, 5, device=DEV)
    c2w, K = _poses(2, 0), np.array([50.0, 50.0, 2.0, 2.0])
    bad_pose = c2w.copy()
    bad_pose[1, 3] = np.nan
    cases = [lambda: ops.depth_cloud(d.cpu(), c2w, K, TRUNC), lambda: ops.depth_cloud(d, c2w, K, 0.0), lambda: ops.depth_cloud(d, c2w, K, -1.0),
             lambda: ops.depth_cloud(d, bad_pose, K, TRUNC), lambda: ops.depth_cloud(d, c2w, [50.0, np.inf, 2.0, 2.0], TRUNC),
             lambda: ops.depth_cloud(d, c2w, [0.0, 50.0, 2.0, 2.0], TRUNC), lambda: ops.depth_cloud(d, c2w, [50.0, -1.0, 2.0, 2.0], TRUNC),
             lambda: ops.depth_cloud(d, c2w, K, TRUNC, size=(0, 5)), lambda: ops.depth_cloud(d, c2w[:1], K, TRUNC),
             lambda: ops.depth_cloud(d.double(), c2w, K, TRUNC), lambda: ops.depth_cloud(d, c2w, K, TRUNC, rgb=torch.zeros(2, 3, 4, 5, dtype=torch.uint8)),
             lambda: ops.depth_cloud(d, c2w, K, TRUNC, rgb=torch.zeros(2, 4, 5, 3, dtype=torch.uint8, device=DEV))]
    p = torch.rand(10, 3, device=DEV)
    nan = p.clone()
    nan[3, 1] = float("nan")
    inf = p.clone()
    inf[0, 2] = float("inf")
    cases += [lambda: ops.voxel_downsample(p.cpu(), 0.05), lambda: ops.voxel_downsample(p, 0.0), lambda: ops.voxel_downsample(p, -0.05),
              lambda: ops.voxel_downsample(p, float("inf")), lambda: ops.voxel_downsample(p, float("nan")),
              lambda: ops.voxel_downsample(nan, 0.05), lambda: ops.voxel_downsample(inf, 0.05), lambda: ops.voxel_downsample(p[:0], 0.05),
              lambda: ops.voxel_downsample(p.double(), 0.05), lambda: ops.voxel_downsample(p, 0.05, torch.zeros(9, 3, dtype=torch.uint8, device=DEV))]
    for k, f in enumerate(cases):
        with pytest.raises((ValueError, RuntimeError)):
            f()
            pytest.fail(f"case {k} was accepted")


def test_abi_refuses_bad_arguments_without_a_launch():
    lib = _lib.load()
    H, W = 4, 5
    d = torch.ones(2, H, W, device=DEV)
    nbytes = lib.cut3r_depth_cloud_workspace_bytes(16, H, W)
    assert nbytes > 0 and lib.cut3r_depth_cloud_workspace_bytes(17, H, W) == -1 and lib.cut3r_depth_cloud_workspace_bytes(0, H, W) == -1
    assert lib.cut3r_depth_cloud_workspace_bytes(1, 0, W) == -1
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    counts = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    P = lambda t: C.c_void_p(t.data_ptr())
    count = lambda depth=P(d), B=2, h=H, w=W, h1=H, w1=W, tr=TRUNC, wsp=P(ws), nb=nbytes, out=P(counts): lib.cut3r_depth_cloud_count(
        depth, B, h, w, h1, w1, tr, wsp, nb, out, None)
    for bad in (dict(depth=None), dict(wsp=None), dict(out=None), dict(B=0), dict(B=17), dict(h=0), dict(w1=-1), dict(tr=0.0), dict(tr=float("nan")),
                dict(nb=8)):
        assert count(**bad) == 1, bad
    torch.cuda.synchronize()
    assert counts.tolist() == [-7, -7]
    assert count() == 0
    torch.cuda.synchronize()
    assert counts.tolist() == [H * W, H * W]
    c2w = np.ascontiguousarray(_poses(2, 0))
    K = np.ascontiguousarray(np.tile([50.0, 50.0, 2.0, 2.0], (2, 1)))
    n = 2 * H * W
    pts = torch.full((n, 3), -7.0, device=DEV)
    H_ = lambda a: a.ctypes.data_as(C.c_void_p)
    emit = lambda depth=P(d), B=2, pose=c2w, k=K, tr=TRUNC, wsp=P(ws), nb=nbytes, out=P(pts), cnt=n, cap=n, rgb=None, col=None: \
        lib.cut3r_depth_cloud_emit(depth, rgb, B, H, W, H, W, None if pose is None else H_(pose), None if k is None else H_(k), tr, wsp, nb, out, col,
                                   cnt, cap, None)
    nan_pose, inf_K, zero_fx = c2w.copy(), K.copy(), K.copy()
    nan_pose[1, 11], inf_K[0, 2], zero_fx[1, 0] = np.nan, np.inf, 0.0
    col = torch.zeros(n, 3, dtype=torch.uint8, device=DEV)
    for bad in (dict(depth=None), dict(pose=None), dict(k=None), dict(wsp=None), dict(out=None), dict(B=0), dict(B=17), dict(pose=nan_pose),
                dict(k=inf_K), dict(k=zero_fx), dict(tr=-1.0), dict(cap=n - 1), dict(cnt=-1), dict(nb=8), dict(col=P(col))):
        assert emit(**bad) == 1, bad
    torch.cuda.synchronize()
    assert bool((pts == -7.0).all())
    assert emit() == 0
    torch.cuda.synchronize()
    assert _same(pts.cpu().numpy(), CO.backproject(np.ones((2, H, W), np.float32), c2w, K, TRUNC)[0])

    N = 10
    p = torch.rand(N, 3, device=DEV)
    lo = np.zeros(3, np.float32)
    hi = np.ones(3, np.float32)
    vb = lib.cut3r_voxel_downsample_workspace_bytes(N)
    assert vb > 0 and lib.cut3r_voxel_downsample_workspace_bytes(0) == -1 and lib.cut3r_cloud_bounds_workspace_bytes(0) == -1
    vws = torch.zeros(vb, dtype=torch.uint8, device=DEV)
    total = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    vcount = lambda pp=P(p), nn=N, v=0.05, a=lo, b=hi, wsp=P(vws), nb=vb, out=P(total): lib.cut3r_voxel_downsample_count(
        pp, nn, v, None if a is None else H_(a), None if b is None else H_(b), wsp, nb, out, None)
    far = np.array([1.0, 0.05 * 2 ** 21, 1.0], np.float32)
    for bad in (dict(pp=None), dict(a=None), dict(b=None), dict(wsp=None), dict(out=None), dict(nn=0), dict(nn=-3), dict(v=0.0), dict(v=-1.0),
                dict(v=float("inf")), dict(v=float("nan")), dict(b=far), dict(a=np.array([0, np.nan, 0], np.float32)),
                dict(b=np.array([np.inf, 1, 1], np.float32)), dict(a=hi, b=lo), dict(nb=8)):
        assert vcount(**bad) == 1, bad
    torch.cuda.synchronize()
    assert total.tolist() == [-7]
    out = torch.zeros(N, 3, device=DEV)
    cnt = torch.zeros(N, dtype=torch.int32, device=DEV)
    vemit = lambda pp=P(p), nn=N, wsp=P(vws), nb=vb, o=P(out), c=P(cnt), M=1, cap=N, cin=None, cout=None: lib.cut3r_voxel_downsample_emit(
        pp, cin, nn, wsp, nb, o, cout, c, M, cap, None)
    for bad in (dict(pp=None), dict(wsp=None), dict(o=None), dict(c=None), dict(nn=0), dict(M=0), dict(M=N + 1), dict(M=5, cap=4), dict(nb=8),
                dict(cout=P(col))):
        assert vemit(**bad) == 1, bad
    b7 = torch.zeros(7, device=DEV)
    bws = torch.zeros(lib.cut3r_cloud_bounds_workspace_bytes(N), dtype=torch.uint8, device=DEV)
    assert lib.cut3r_cloud_bounds(None, N, P(b7), P(bws), bws.numel(), None) == 1
    assert lib.cut3r_cloud_bounds(P(p), 0, P(b7), P(bws), bws.numel(), None) == 1
    assert lib.cut3r_cloud_bounds(P(p), N, P(b7), P(bws), 4, None) == 1


@pytest.mark.parametrize("N", [70001, 300007])
def test_cloud_bounds_are_exact(N):
    """70001 points: 274 blocks, one point a thread.  300007 points: more than the 1024 x 256 threads of the largest grid, so threads
    run the grid-stride loop a second time, some of them not; the extremes of each axis are put into the part only that second pass reads"""
    g = np.random.default_rng(4)
    p = g.normal(size=(N, 3)).astype(np.float32)
    if N > 1024 * 256:
        p[1024 * 256 + 5] = [-9.0, 0.0, 9.5]
        p[N - 1] = [8.0, -7.5, 0.0]
    lo, hi = ops.cloud_bounds(torch.from_numpy(p).to(DEV))
    assert _same(lo.numpy(), p.min(0)) and _same(hi.numpy(), p.max(0))
