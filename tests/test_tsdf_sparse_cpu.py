"""CPU: the sparse brick TSDF volume's contract on its numpy restatement (tests/tsdf_sparse_oracle.py): the brick allocation covers every
negative voxel of the dense volume and its 26 neighbours, the mesh of the volume restricted to the allocated bricks is the dense mesh
as a set of triangles, the windowed oracle is the dense one, the grid limits of SparseTSDFVolume, and the plumbing of
fuse_*(sparse=True)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from cut3r_slam_amd import ops
from cut3r_slam_amd import tsdf as T
from tests import tsdf_oracle as O
from tests import tsdf_sparse_oracle as S
from tests.test_tsdf_gpu import _hard_scene

VOXEL = 0.02


def _allocation(depth, w2c, K, origin, dims, trunc, depth_max):
    flags = np.zeros(S.brick_dims(dims)[::-1], np.uint8)
    S.mark(flags, origin, VOXEL, dims, depth, w2c, K, trunc, depth_max)
    return flags, S.voxel_mask(flags, dims)


def _check_superset_and_mesh(vol, vm, origin, thresholds):
    neg = vol[0] < 0
    assert neg.any()
    need = S.dilate26(neg)
    assert not (need & ~vm).any(), f"{int((need & ~vm).sum())} voxels the mesh needs are not allocated"
    sparse = S.masked(vol, vm)
    for thr in thresholds:
        ref = O.extract(vol, origin, VOXEL, thr)
        got = O.extract(sparse, origin, VOXEL, thr)
        assert len(ref[2]) > 1000 and len(got[2]) == len(ref[2])
        assert np.array_equal(S.soup(*got), S.soup(*ref))


def test_allocation_covers_the_sphere_and_its_mesh_is_the_dense_mesh():
    depth, rgb, w2c, K = O.sphere_scene(n_views=24, H=192, W=256, f=220.0)
    origin, dims, trunc = O.sphere_grid(VOXEL)
    vol = O.integrate(O.new_volume(dims), origin, VOXEL, depth, w2c, K, trunc, 5.0, rgb=rgb)
    flags, vm = _allocation(depth, w2c, K, origin, dims, trunc, 5.0)
    _check_superset_and_mesh(vol, vm, origin, (1.0, 4.0))
    # the inside of the sphere and the far corners of the grid stay empty
    assert flags.sum() < 0.8 * flags.size


def test_allocation_covers_invalid_depths_and_cameras_inside_the_grid():
    depth, rgb, w2c, K, conf, origin, dims = _hard_scene()
    trunc = float(np.float32(6.0 * np.float32(VOXEL)))
    # the allocation ignores the confidence gate: a superset (the random background depths of this scene fill most of the small grid)
    _, vm = _allocation(depth, w2c, K, origin, dims, trunc, 5.0)
    for gate in (None, 0.3):
        vol = O.integrate(O.new_volume(dims), origin, VOXEL, depth, w2c, K, trunc, 5.0, rgb=rgb, conf=conf, conf_ds=2, conf_min=gate)
        _check_superset_and_mesh(vol, vm, origin, (1.0, 2.0))


def test_soup_ignores_order_and_keeps_winding():
    g = np.random.default_rng(0)
    v = g.normal(size=(30, 3)).astype(np.float32)
    c = g.integers(0, 256, (30, 3), dtype=np.uint8)
    f = g.integers(0, 30, (50, 3)).astype(np.int32)
    perm = g.permutation(30)
    inv = np.argsort(perm)
    f2 = inv[f][g.permutation(50)].astype(np.int32)
    f2 = np.stack([np.roll(row, g.integers(0, 3)) for row in f2])
    assert np.array_equal(S.soup(v, c, f), S.soup(v[perm], c[perm], f2))
    flipped = f.copy()
    flipped[0] = flipped[0, ::-1]
    assert flipped[0, 0] != flipped[0, 2] and not np.array_equal(S.soup(v, c, f), S.soup(v, c, flipped))
    moved = v.copy()
    moved[f[3, 1], 2] = np.nextafter(moved[f[3, 1], 2], np.float32(9))
    assert not np.array_equal(S.soup(v, c, f), S.soup(moved, c, f))
    assert S.soup(v, c, f[:0]).shape == (0, 18)


def test_windowed_oracle_is_the_dense_oracle():
    depth, rgb, w2c, K = O.sphere_scene(n_views=6)
    origin, dims, trunc = O.sphere_grid(0.04)
    full = O.integrate(O.new_volume(dims), origin, 0.04, depth, w2c, K, trunc, 5.0, rgb=rgb)
    for a, b in zip(O.extract(full, origin, 0.04, 1.0), S.extract_window(full, origin, 0.04, (0, 0, 0), 1.0)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    # a window of the grid holds the grid's values at its voxels, and its mesh is the part of the mesh whose cells it contains
    off, wd = (3, 5, 20), (30, 28, 14)
    win = S.integrate_window(O.new_volume(wd), origin, 0.04, off, depth, w2c, K, trunc, 5.0, rgb=rgb)
    sl = (slice(off[2], off[2] + wd[2]), slice(off[1], off[1] + wd[1]), slice(off[0], off[0] + wd[0]))
    assert np.array_equal(win[0].view(np.uint32), full[0][sl].view(np.uint32)) and np.array_equal(win[1], full[1][sl])
    assert np.array_equal(win[2].view(np.uint32), full[2][(slice(None),) + sl].view(np.uint32))
    wv, wc, wf = S.extract_window(win, origin, 0.04, off, 1.0)
    assert len(wf) > 100
    fs, ws = S.soup(*O.extract(full, origin, 0.04, 1.0)), S.soup(wv, wc, wf)
    assert {r.tobytes() for r in ws} <= {r.tobytes() for r in fs}


def test_grid_limits_and_error_text():
    origin, dims = T.SparseTSDFVolume.grid_for((0, 0, 0), (1.0, 0.5, 0.25), 0.05, pad=0.1)
    assert (origin, dims) == T.TSDFVolume.grid_for((0, 0, 0), (1.0, 0.5, 0.25), 0.05, pad=0.1)
    # 30 m cubed at 0.02 m: beyond the dense limit, well inside the table's
    with pytest.raises(ValueError, match="GB"):
        T.TSDFVolume.grid_for((0, 0, 0), (30, 30, 30), 0.02, pad=0.16)
    origin, dims = T.SparseTSDFVolume.grid_for((0, 0, 0), (30, 30, 30), 0.02, pad=0.16)
    assert dims[0] * dims[1] * dims[2] > 2 ** 31 and np.prod(ops.tsdf_brick_dims(dims)) < 2 ** 28
    with pytest.raises(ValueError, match=r"bricks needs a .* GB table"):
        T.SparseTSDFVolume.grid_for((0, 0, 0), (200, 200, 200), 0.02, pad=0.16)          # 1253^3 bricks
    with pytest.raises(ValueError, match="bricks"):
        T.SparseTSDFVolume.grid_for((0, 0, 0), (30, 30, 30), 0.02, pad=0.16, max_bricks=10 ** 6)
    with pytest.raises(ValueError, match="per axis"):
        T.SparseTSDFVolume.grid_for((0, 0, 0), (30000, 0.1, 0.1), 0.02, pad=0.16)         # 1.5 M voxels along x
    with pytest.raises(ValueError, match="not a box"):
        T.SparseTSDFVolume.grid_for((0, 0, 0), (np.nan, 1, 1), 0.02, pad=0.16)
    for bad in ((0, 8, 8), (2 ** 20 + 1, 8, 8), (2 ** 20, 2 ** 20, 64)):
        with pytest.raises(ValueError):
            T.SparseTSDFVolume((0, 0, 0), 0.02, bad, device="cpu")
    with pytest.raises(ValueError):
        T.SparseTSDFVolume((0, 0, 0), 0.0, (8, 8, 8), device="cpu")
    vol = T.SparseTSDFVolume((0, 0, 0), 0.02, (20, 9, 8), device="cpu")
    assert vol.brick_dims == (3, 2, 1) and vol.n_bricks == 0 and vol.nbytes == 5 * 6 and vol.table.shape == (1, 2, 3)
    d = vol.to_dense()
    assert d[0].shape == (8, 9, 20) and bool((d[0] == 1).all()) and d[2].shape == (3, 8, 9, 20) and not bool(vol.allocated_mask().any())
    m = vol.extract_mesh(1.0)
    assert m.vertices.shape == (0, 3) and m.faces.shape == (0, 3)
    big = T.SparseTSDFVolume((0, 0, 0), 0.02, (1600, 1600, 1600), device="cpu")
    with pytest.raises(ValueError, match="dense"):
        big.to_dense()


def test_c2w_rows_invert_the_views():
    w2c = O.sphere_poses(5, 1.6)[:, :3, :].reshape(-1, 12).astype(np.float32)
    c2w = T.c2w_rows(w2c)
    assert c2w.dtype == np.float32 and np.array_equal(c2w, S.c2w_rows(w2c))
    for a, b in zip(w2c.reshape(-1, 3, 4).astype(np.float64), c2w.reshape(-1, 3, 4).astype(np.float64)):
        assert np.allclose(b[:, :3] @ a[:, :3], np.eye(3), atol=1e-6) and np.allclose(b[:, :3] @ a[:, 3] + b[:, 3], 0, atol=1e-6)


def _fake_ops(monkeypatch, calls):
    """the four kernels' wrappers replaced by recorders: mark flags two bricks, assign numbers them as the kernel does"""
    def mark(flags, dims, origin, voxel, depth, c2w, K, trunc, depth_max):
        calls.append(("mark", depth.shape[0], tuple(c2w.shape), tuple(K.shape), dims))
        flags.reshape(-1)[[1, 4]] = 1

    def assign(flags, table, dims):
        f = flags.reshape(-1).to(torch.int32)
        table.reshape(-1).copy_(torch.where(f > 0, torch.cumsum(f, 0, dtype=torch.int32) - f, torch.full_like(f, -1)))
        calls.append(("assign", int(f.sum())))
        return int(f.sum())

    def integrate(tsdf, weight, color, bricks, dims, origin, voxel, depth, w2c, K, trunc, depth_max, rgb=None, conf=None, conf_ds=1,
                  conf_min=0.0):
        calls.append(("integrate", depth.shape[0], bricks.tolist(), tuple(tsdf.shape), rgb is not None, None if conf is None else tuple(conf.shape),
                      conf_ds, conf_min))
        weight += 1

    monkeypatch.setattr(ops, "tsdf_sparse_mark", mark)
    monkeypatch.setattr(ops, "tsdf_sparse_assign", assign)
    monkeypatch.setattr(ops, "tsdf_sparse_integrate", integrate)


def test_fuse_keyframes_sparse_allocates_all_views_then_integrates(monkeypatch):
    calls = []
    _fake_ops(monkeypatch, calls)
    n, H, W = 20, 6, 8
    g = torch.Generator().manual_seed(0)
    w2c = torch.tensor([1.0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]).repeat(25, 1)
    kf = SimpleNamespace(device=torch.device("cpu"), depth=torch.rand(25, H, W, generator=g) + 1.0,
                         image=torch.randint(0, 256, (25, 3, H, W), generator=g, dtype=torch.uint8), w2c=w2c,
                         intrinsic=torch.tensor([5.0, 5.0, 3.5, 2.5]).repeat(25, 1), conf_ds=torch.rand(5, 5, H // 2, W // 2, generator=g),
                         downsample_ratio=2)
    vol = T.fuse_keyframes(kf, n, 0.05, trunc_voxels=4.0, depth_max=5.0, conf_min=0.25, sparse=True)
    assert isinstance(vol, T.SparseTSDFVolume) and vol.n_bricks == 2 and vol.bricks.tolist() == [1, 4]
    assert vol.trunc == pytest.approx(0.2) and vol.tsdf.shape == (2, 512) and vol.color.shape == (3, 2, 512)
    # one allocation pass over all 20 views, then the integration in launches of 16 + 4, none of which allocates again
    assert [c[0] for c in calls] == ["mark", "assign", "integrate", "integrate"]
    assert calls[0][1:4] == (20, (20, 12), (20, 4)) and calls[0][4] == vol.dims
    assert calls[2][1:] == (16, [1, 4], (2, 512), True, (16, H // 2, W // 2), 2, 0.25)
    assert calls[3][1] == 4 and calls[3][5] == (4, H // 2, W // 2)
    assert float(vol.weight.min()) == 2.0
    # the dense default is untouched by the keyword
    dense = []
    monkeypatch.setattr(ops, "tsdf_integrate", lambda *a, **k: dense.append(a[5].shape[0]))
    d = T.fuse_keyframes(kf, n, 0.05, trunc_voxels=4.0)
    assert isinstance(d, T.TSDFVolume) and dense == [16, 4] and [c[0] for c in calls].count("mark") == 1
    # without a gate no confidence is passed
    del calls[:]
    T.fuse_keyframes(kf, 3, 0.05, sparse=True)
    assert calls[2][5] is None and calls[2][7] == 0.0


def test_growing_the_pool_keeps_what_the_bricks_held(monkeypatch):
    calls = []
    _fake_ops(monkeypatch, calls)
    vol = T.SparseTSDFVolume((0, 0, 0), 0.05, (24, 16, 8), device="cpu")
    d, w, K = torch.ones(1, 4, 4), torch.eye(4)[:3].reshape(1, 12), torch.tensor([4.0, 4.0, 1.5, 1.5])
    assert vol.allocate(d, w, K) == 2 and vol.allocate(d, w, K) == 0
    vol.tsdf[0], vol.tsdf[1] = 0.25, -0.5
    vol.color[2, 1] = 7.0
    monkeypatch.setattr(ops, "tsdf_sparse_mark", lambda flags, *a: flags.reshape(-1).__setitem__([0, 3], 1))
    assert vol.allocate(d, w, K) == 2 and vol.bricks.tolist() == [0, 1, 3, 4] and vol.table.reshape(-1).tolist() == [0, 1, -1, 2, 3, -1]
    assert vol.tsdf[:, 0].tolist() == [1.0, 0.25, 1.0, -0.5] and vol.color[2, :, 5].tolist() == [0.0, 0.0, 0.0, 7.0]
    dense = vol.to_dense()
    assert dense[0].shape == (8, 16, 24) and float(dense[0][0, 0, 8]) == 0.25 and float(dense[0][3, 9, 12]) == -0.5
    assert float(dense[2][2, 7, 15, 15]) == 7.0 and float(dense[0][0, 0, 16]) == 1.0
    assert vol.allocated_mask()[0].tolist() == [[True] * 16 + [False] * 8] * 8 + [[True] * 16 + [False] * 8] * 8
    assert vol.nbytes == 4 * (20 * 512 + 4) + 5 * 6
    # integrate(allocate=True) allocates for the views it is given before it fuses them
    del calls[:]
    _fake_ops(monkeypatch, calls)
    fresh = T.SparseTSDFVolume((0, 0, 0), 0.05, (24, 16, 8), device="cpu").integrate(d, w, K)
    assert [c[0] for c in calls] == ["mark", "assign", "integrate"] and fresh.n_bricks == 2


def test_fuse_mapper_and_the_driver_pass_sparse_through(monkeypatch):
    calls = []
    _fake_ops(monkeypatch, calls)
    H, W = 6, 8
    views = (torch.ones(3, H, W), torch.zeros(3, 3, H, W, dtype=torch.uint8), torch.eye(4)[:3].reshape(1, 12).repeat(3, 1),
             torch.tensor([5.0, 5.0, 3.5, 2.5]).repeat(3, 1))
    monkeypatch.setattr(T, "render_mapper_views", lambda m: views)
    vol = T.fuse_mapper(SimpleNamespace(viewpoints={0: None}, device=torch.device("cpu")), 0.05, sparse=True)
    assert isinstance(vol, T.SparseTSDFVolume) and [c[0] for c in calls] == ["mark", "assign", "integrate"] and calls[2][4] is True
    from cut3r_slam_amd.slam import Cut3rSlam
    seen = []
    monkeypatch.setattr(T, "fuse_keyframes", lambda kf, n, voxel, **k: seen.append(("tracker", k["sparse"])) or SimpleNamespace(
        extract_mesh=lambda w: ("mesh", w)))
    monkeypatch.setattr(T, "fuse_mapper", lambda m, voxel, **k: seen.append(("mapper", k["sparse"])))
    s = SimpleNamespace(keyframes=SimpleNamespace(counter=SimpleNamespace(value=12)), tracked_only=False, tracker=SimpleNamespace(t1=7),
                        mapper=None)
    s.fuse = lambda *a, **k: Cut3rSlam.fuse(s, *a, **k)
    Cut3rSlam.fuse(s, 0.05)
    Cut3rSlam.fuse(s, 0.05, sparse=True)
    assert Cut3rSlam.reconstruct(s, 0.05, weight_threshold=3.0, sparse=True) == ("mesh", 3.0)
    s.mapper = SimpleNamespace(viewpoints={0: None})
    Cut3rSlam.fuse(s, 0.05, sparse=True)
    assert seen == [("tracker", False), ("tracker", True), ("tracker", True), ("mapper", True)]
