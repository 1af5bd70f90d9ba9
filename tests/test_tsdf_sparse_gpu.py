"""GPU: the sparse brick TSDF volume (csrc/tsdf_sparse.hip) against the numpy oracles, bit for bit: the mark kernel's flags, the fused
pool on its allocated voxels, the mesh as a set of triangles (against the dense oracle and the dense GPU volume); batch invariance,
determinism, a scene whose virtual grid is beyond the dense limit, refused arguments."""
import numpy as np
import pytest
import torch

from cut3r_slam_amd import _lib, ops
from cut3r_slam_amd import tsdf as T
from tests import tsdf_oracle as O
from tests import tsdf_sparse_oracle as S
from tests.test_tsdf_gpu import _hard_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VOXEL = 0.02


def _dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)


def _assert_same_soup(mesh, ref):
    assert len(mesh.faces) == len(ref[2]) and len(mesh.vertices) == len(ref[0]), (mesh.faces.shape, ref[2].shape, mesh.vertices.shape, ref[0].shape)
    assert np.array_equal(S.soup(*mesh), S.soup(*ref))


def _assert_dense_identical_where_allocated(vol, ref):
    """to_dense() against the dense oracle's planes: bit for bit on allocated voxels, the initial state elsewhere; every negative
    voxel allocated"""
    vm = vol.allocated_mask().cpu().numpy()
    got = [a.cpu().numpy() for a in vol.to_dense()]
    init = (np.float32(1), np.float32(0), np.float32(0))
    for name, a, b, i0 in zip(("tsdf", "weight", "color"), got, ref, init):
        m = vm if a.ndim == 3 else np.broadcast_to(vm, a.shape)
        assert np.array_equal(a.view(np.uint32)[m], b.view(np.uint32)[m]), f"{name}: {np.count_nonzero(a[m] != b[m])} allocated voxels differ"
        assert np.all(a[~m] == i0), name
    assert not ((ref[0] < 0) & ~vm).any(), "a voxel with tsdf < 0 is not allocated"
    return vm


@pytest.fixture(scope="module")
def sphere():
    return O.sphere_scene(n_views=24, H=192, W=256, f=220.0)


def test_mark_kernel_flags_equal_the_oracle(sphere):
    depth, rgb, w2c, K = sphere
    origin, dims, _ = O.sphere_grid(VOXEL)
    vol = T.SparseTSDFVolume(origin, VOXEL, dims, device=DEV)
    assert vol.allocate(*_dev(depth, w2c), torch.from_numpy(K)) == vol.n_bricks > 0
    ref = S.mark(np.zeros(vol.flags.shape, np.uint8), vol.origin, vol.voxel_size, dims, depth, w2c, K, vol.trunc, vol.depth_max)
    assert 0 < ref.sum() < ref.size
    assert np.array_equal(vol.flags.cpu().numpy(), ref)
    # the table numbers the flagged bricks in ascending order
    t = vol.table.cpu().numpy().reshape(-1)
    assert np.array_equal(np.nonzero(t >= 0)[0], np.nonzero(ref.reshape(-1))[0]) and np.array_equal(t[t >= 0], np.arange(ref.sum()))
    assert np.array_equal(vol.bricks.cpu().numpy(), np.nonzero(ref.reshape(-1))[0])
    # invalid depths, cameras inside the grid, a grid that is not a multiple of the brick, per-view intrinsics
    depth, rgb, w2c, K, conf, origin, dims = _hard_scene()
    Kb = np.repeat(K[None], len(depth), 0) * np.linspace(0.9, 1.1, len(depth), dtype=np.float32)[:, None]
    for org, dm, vx in ((origin, dims, VOXEL), ((-2.0, -1.5, -1.0), (333, 250, 181), 0.0125)):
        vol = T.SparseTSDFVolume(org, vx, dm, trunc_voxels=6.0, device=DEV)
        vol.allocate(*_dev(depth, w2c, Kb))
        ref = S.mark(np.zeros(vol.flags.shape, np.uint8), vol.origin, vol.voxel_size, dm, depth, w2c, Kb, vol.trunc, vol.depth_max)
        assert np.array_equal(vol.flags.cpu().numpy(), ref), (org, int(ref.sum()), int(vol.flags.sum()))
    assert 0 < ref.sum() < ref.size


def test_sphere_matches_the_dense_oracle_and_the_dense_volume(sphere):
    depth, rgb, w2c, K = sphere
    origin, dims, _ = O.sphere_grid(VOXEL)
    d, c, w = _dev(depth, rgb, w2c)
    vol = T.SparseTSDFVolume(origin, VOXEL, dims, device=DEV).integrate(d, w, torch.from_numpy(K), rgb=c)
    ref = O.integrate(O.new_volume(dims), vol.origin, vol.voxel_size, depth, w2c, K, vol.trunc, vol.depth_max, rgb=rgb)
    vm = _assert_dense_identical_where_allocated(vol, ref)
    assert 0.05 < vm.mean() < 0.9
    dense = T.TSDFVolume(origin, VOXEL, dims, device=DEV).integrate(d, w, torch.from_numpy(K), rgb=c)
    for thr in (1.0, 4.0):
        mesh = vol.extract_mesh(thr)
        assert len(mesh.faces) > 10000 and mesh.faces.min() == 0 and mesh.faces.max() == len(mesh.vertices) - 1
        _assert_same_soup(mesh, O.extract(ref, vol.origin, vol.voxel_size, thr))
        _assert_same_soup(mesh, dense.extract_mesh(thr))


def test_hard_scene_with_a_confidence_gate_matches_the_dense_oracle_and_the_dense_volume():
    depth, rgb, w2c, K, conf, origin, dims = _hard_scene()
    B = depth.shape[0]
    d, c, w, cf = _dev(depth, rgb, w2c, conf)
    Kb = torch.from_numpy(K).expand(B, 4)
    vol = T.SparseTSDFVolume(origin, VOXEL, dims, trunc_voxels=6.0, depth_max=5.0, device=DEV)
    vol.integrate(d, w, Kb, rgb=c, conf=cf, conf_ds=2, conf_min=0.3)
    ref = O.integrate(O.new_volume(dims), vol.origin, vol.voxel_size, depth, w2c, K, vol.trunc, vol.depth_max, rgb=rgb, conf=conf, conf_ds=2,
                      conf_min=0.3)
    _assert_dense_identical_where_allocated(vol, ref)
    dense = T.TSDFVolume(origin, VOXEL, dims, trunc_voxels=6.0, depth_max=5.0, device=DEV)
    dense.integrate(d, w, Kb, rgb=c, conf=cf, conf_ds=2, conf_min=0.3)
    for thr in (1.0, 4.0):
        mesh = vol.extract_mesh(thr)
        assert len(mesh.faces) > 1000
        _assert_same_soup(mesh, O.extract(ref, vol.origin, vol.voxel_size, thr))
        _assert_same_soup(mesh, dense.extract_mesh(thr))
    # without colour the colour pool stays as it was
    v2 = T.SparseTSDFVolume(origin, VOXEL, dims, trunc_voxels=6.0, device=DEV).integrate(d, w, Kb)
    ref2 = O.integrate(O.new_volume(dims), v2.origin, v2.voxel_size, depth, w2c, K, v2.trunc, v2.depth_max)
    _assert_dense_identical_where_allocated(v2, ref2)
    assert float(v2.color.abs().max()) == 0.0


def test_a_brick_far_from_every_surface_still_takes_the_free_space_updates(sphere):
    """the volume is the dense one restricted to its bricks, whatever made them: bricks flagged by hand (free space, behind the
    cameras, the far corner of the grid) hold the dense values too"""
    depth, rgb, w2c, K = sphere
    origin, dims, _ = O.sphere_grid(VOXEL)
    vol = T.SparseTSDFVolume(origin, VOXEL, dims, device=DEV)
    vol.flags.reshape(-1)[::7] = 1
    d, c, w = _dev(depth, rgb, w2c)
    vol.integrate(d, w, torch.from_numpy(K), rgb=c)                       # allocates the marked bricks on top of those
    ref = O.integrate(O.new_volume(dims), vol.origin, vol.voxel_size, depth, w2c, K, vol.trunc, vol.depth_max, rgb=rgb)
    _assert_dense_identical_where_allocated(vol, ref)


def _pool_bits(vol):
    return [a.cpu().numpy().view(np.uint32) for a in (vol.tsdf, vol.weight, vol.color)]


def test_batch_invariance():
    depth, rgb, w2c, K, _, origin, dims = _hard_scene()
    B = depth.shape[0]
    d, c, w = _dev(depth, rgb, w2c)
    Kb = torch.from_numpy(K).to(DEV).expand(B, 4).contiguous()

    def fresh():
        v = T.SparseTSDFVolume(origin, VOXEL, dims, device=DEV)
        v.allocate(d, w, Kb)
        return v

    def raw(v, a, b):
        ops.tsdf_sparse_integrate(v.tsdf, v.weight, v.color, v.bricks, v.dims, v.origin, v.voxel_size, d[a:b], w[a:b], Kb[a:b], v.trunc,
                                  v.depth_max, rgb=c[a:b])

    one, batch = fresh(), fresh()
    for b in range(16):
        raw(one, b, b + 1)
    raw(batch, 0, 16)
    for a, b_ in zip(_pool_bits(one), _pool_bits(batch)):
        assert np.array_equal(a, b_)
    assert float(batch.weight.max()) > 4
    # 37 views: chunks of 16 + 16 + 5 against one view at a time
    chunked = fresh().integrate(d, w, Kb, rgb=c, allocate=False)
    single = fresh()
    for b in range(B):
        raw(single, b, b + 1)
    assert B == 37
    for a, b_ in zip(_pool_bits(single), _pool_bits(chunked)):
        assert np.array_equal(a, b_)


def test_two_runs_give_identical_arrays(sphere):
    depth, rgb, w2c, K = sphere
    origin, dims, _ = O.sphere_grid(VOXEL)
    d, c, w = _dev(depth, rgb, w2c)
    runs = []
    for _ in range(2):
        vol = T.SparseTSDFVolume(origin, VOXEL, dims, device=DEV).integrate(d, w, torch.from_numpy(K), rgb=c)
        runs.append((vol.bricks.cpu().numpy(), vol.extract_mesh(1.0), vol.extract_mesh(1.0)))
    assert np.array_equal(runs[0][0], runs[1][0])
    for m in (runs[0][2], runs[1][1], runs[1][2]):
        assert np.array_equal(m.vertices.view(np.uint32), runs[0][1].vertices.view(np.uint32))
        assert np.array_equal(m.colors, runs[0][1].colors) and np.array_equal(m.faces, runs[0][1].faces)
    # the documented order: vertices by (pool voxel, mask), faces by pool cell -- both ascend along the pool, so along z of a brick column
    assert len(runs[0][1].faces) > 10000


def test_two_spheres_fifty_metres_apart_fuse_where_the_dense_grid_refuses():
    H, W, f, radius = 96, 128, 110.0, 0.5
    K = np.asarray((f, f, (W - 1) / 2, (H - 1) / 2), np.float32)
    centres = (np.zeros(3), np.array([29.0, 30.0, 31.0]))
    assert 49 < np.linalg.norm(centres[1]) < 53
    depth, rgb, w2c = [], [], []
    for c, seed in zip(centres, (0, 1)):
        for P in O.sphere_poses(12, 1.6, seed):
            P = P.copy()
            P[:3, 3] -= P[:3, :3] @ c                                   # the same camera, moved with its sphere
            dd, cc = O.render_sphere(P, K, H, W, radius, center=c)
            depth.append(dd)
            rgb.append(cc)
            w2c.append(P[:3].reshape(12))
    depth, rgb, w2c = np.stack(depth).astype(np.float32), np.stack(rgb), np.stack(w2c).astype(np.float32)
    lo, hi = centres[0] - radius, centres[1] + radius
    with pytest.raises(ValueError, match="GB"):
        T.TSDFVolume.from_bounds(lo, hi, VOXEL, max_voxels=2 ** 31 - 1, device=DEV)
    vol = T.SparseTSDFVolume.from_bounds(lo, hi, VOXEL, device=DEV)
    X, Y, Z = vol.dims
    assert X * Y * Z > 2 ** 31 and vol.table.numel() <= 2 ** 28 and max(vol.dims) <= 2 ** 20            # 1516 x 1566 x 1616 voxels
    d, c, w = _dev(depth, rgb, w2c)
    vol.integrate(d, w, torch.from_numpy(K), rgb=c)
    assert 0 < vol.n_bricks < 0.05 * vol.table.numel()
    assert vol.nbytes < 0.5e9
    with pytest.raises(ValueError, match="dense"):
        vol.to_dense()
    mesh = vol.extract_mesh(1.0)
    near = np.linalg.norm(mesh.vertices.astype(np.float64), axis=1) < 25            # which sphere a vertex belongs to
    fnear = near[mesh.faces]
    assert np.all(fnear.all(1) | ~fnear.any(1))
    half = int(round((radius + vol.trunc) / VOXEL)) + 16                             # the window: the sphere, the truncation band, two bricks
    total = 0
    for c_, sel in zip(centres, (fnear.all(1), ~fnear.any(1))):
        mid = [int(round((c_[a] - vol.origin[a]) / vol.voxel_size)) for a in range(3)]
        off = tuple(max(0, m - half) for m in mid)                                   # cut at the grid's faces, where the grid ends too
        wd = tuple(min(n, m + half + 1) - o for m, o, n in zip(mid, off, vol.dims))
        assert min(wd) > 2 * (half - 16)
        win = S.integrate_window(O.new_volume(wd), vol.origin, vol.voxel_size, off, depth, w2c, K, vol.trunc, vol.depth_max, rgb=rgb)
        ref = S.extract_window(win, vol.origin, vol.voxel_size, off, 1.0)
        assert len(ref[2]) > 10000
        idx, inv = np.unique(mesh.faces[sel], return_inverse=True)
        _assert_same_soup(T.Mesh(mesh.vertices[idx], mesh.colors[idx], inv.reshape(-1, 3).astype(np.int32)), ref)
        total += len(ref[2])
    assert total == len(mesh.faces)


def test_bad_arguments_are_refused():
    lib = _lib.load()
    vol = T.SparseTSDFVolume((0, 0, 0), VOXEL, (16, 16, 8), device=DEV)
    vol.flags.fill_(1)
    d = torch.ones(2, 4, 5, device=DEV) * 9                                # beyond depth_max: the calls that run change nothing
    w2c = torch.eye(4, device=DEV)[:3].reshape(1, 12).repeat(2, 1).contiguous()
    K = torch.ones(2, 4, device=DEV)
    assert vol.allocate(d, w2c, K) == 4 and vol.n_bricks == 4
    p, s = ops._p, ops._stream()
    big = 2 ** 20

    def mark(flags=vol.flags, X=16, Y=16, Z=8, voxel=VOXEL, B=2, H=4, W=5, depth=d, c2w=w2c, trunc=0.1):
        return lib.cut3r_tsdf_sparse_mark(p(flags), X, Y, Z, 0.0, 0.0, 0.0, voxel, p(depth), B, H, W, p(c2w), p(K), trunc, 5.0, s)

    assert mark() == 0
    for kw in ({"flags": None}, {"depth": None}, {"c2w": None}, {"X": 0}, {"Y": big + 1}, {"X": big, "Y": big, "Z": 64}, {"voxel": 0.0},
               {"trunc": -1.0}, {"B": 0}, {"H": 0}, {"B": 2 ** 15, "H": 2 ** 8, "W": 2 ** 8}):
        assert mark(**kw) == 1, kw
    ws = torch.empty(max(lib.cut3r_tsdf_sparse_assign_workspace_bytes(16, 16, 8), 1), dtype=torch.uint8, device=DEV)
    total = torch.empty(1, dtype=torch.int64, device=DEV)
    assert lib.cut3r_tsdf_sparse_assign_workspace_bytes(0, 8, 8) == -1 and lib.cut3r_tsdf_sparse_assign_workspace_bytes(big, big, 64) == -1
    assert lib.cut3r_tsdf_sparse_assign(None, p(vol.table), 16, 16, 8, p(ws), ws.numel(), p(total), s) == 1
    assert lib.cut3r_tsdf_sparse_assign(p(vol.flags), None, 16, 16, 8, p(ws), ws.numel(), p(total), s) == 1
    assert lib.cut3r_tsdf_sparse_assign(p(vol.flags), p(vol.table), 16, 16, 8, p(ws), ws.numel(), None, s) == 1
    assert lib.cut3r_tsdf_sparse_assign(p(vol.flags), p(vol.table), 16, 16, 8, p(ws), -1, p(total), s) == 1
    assert lib.cut3r_tsdf_sparse_assign(p(vol.flags), p(vol.table), 16, big + 8, 8, p(ws), ws.numel(), p(total), s) == 1

    def integ(tsdf=vol.tsdf, bricks=vol.bricks, nb=4, B=2, X=16, Y=16, Z=8, voxel=VOXEL, trunc=0.1, H=4, W=5):
        return lib.cut3r_tsdf_sparse_integrate(p(tsdf), p(vol.weight), p(vol.color), p(bricks), nb, X, Y, Z, 0.0, 0.0, 0.0, voxel, p(d), None,
                                               None, B, H, W, 0, 0, 1, 0.0, p(w2c), p(K), trunc, 5.0, s)

    assert integ() == 0
    torch.cuda.synchronize()
    for kw in ({"tsdf": None}, {"bricks": None}, {"nb": 0}, {"nb": 5}, {"nb": 2 ** 22}, {"B": 0}, {"B": 17}, {"X": 0}, {"Y": -1}, {"Z": big + 1},
               {"voxel": 0.0}, {"trunc": 0.0}, {"H": 0}):
        assert integ(**kw) == 1, kw
    nbytes = lib.cut3r_tsdf_sparse_mesh_workspace_bytes(4)
    assert nbytes >= 18 * 4 * 512
    assert lib.cut3r_tsdf_sparse_mesh_workspace_bytes(0) == -1 and lib.cut3r_tsdf_sparse_mesh_workspace_bytes(2 ** 22) == -1
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    totals = torch.empty(2, dtype=torch.int64, device=DEV)

    def count(tsdf=vol.tsdf, table=vol.table, bricks=vol.bricks, nb=4, Z=8, nbytes=nbytes, totals=totals):
        return lib.cut3r_tsdf_sparse_mesh_count(p(tsdf), p(vol.weight), p(table), p(bricks), nb, 16, 16, Z, 1.0, p(ws), nbytes, p(totals), s)

    assert count() == 0
    assert [int(v) for v in totals.cpu()] == [0, 0]
    for kw in ({"tsdf": None}, {"table": None}, {"bricks": None}, {"nb": 0}, {"nb": 5}, {"Z": 0}, {"nbytes": nbytes - 1}, {"totals": None}):
        assert count(**kw) == 1, kw

    def emit(color=vol.color, table=vol.table, nb=4, voxel=VOXEL, nbytes=nbytes, nv=0, nf=0):
        return lib.cut3r_tsdf_sparse_mesh_emit(p(vol.tsdf), p(color), p(table), p(vol.bricks), nb, 16, 16, 8, 0.0, 0.0, 0.0, voxel, p(ws), nbytes,
                                               None, None, None, nv, nf, s)

    assert emit() == 0
    for kw in ({"color": None}, {"table": None}, {"nb": 0}, {"voxel": 0.0}, {"nbytes": nbytes - 1}, {"nv": 5}, {"nf": 5}, {"nv": -1},
               {"nv": 2 ** 31}):
        assert emit(**kw) == 1, kw
    # the wrappers
    args = (vol.tsdf, vol.weight, vol.color, vol.bricks, vol.dims, vol.origin, VOXEL)
    with pytest.raises(ValueError):
        ops.tsdf_sparse_integrate(*args, torch.ones(17, 4, 5, device=DEV), torch.zeros(17, 12, device=DEV), torch.ones(17, 4, device=DEV), 0.1, 5.0)
    with pytest.raises(ValueError):
        ops.tsdf_sparse_integrate(*args[:6], 0.0, d, w2c, K, 0.1, 5.0)
    with pytest.raises(ValueError):
        ops.tsdf_sparse_integrate(*args, d, w2c, K, 0.0, 5.0)
    with pytest.raises(ValueError):
        ops.tsdf_sparse_integrate(vol.tsdf.cpu(), *args[1:], d, w2c, K, 0.1, 5.0)
    with pytest.raises(ValueError):
        ops.tsdf_sparse_integrate(*args, d, w2c[:1], K, 0.1, 5.0)
    with pytest.raises(ValueError):
        ops.tsdf_sparse_integrate(vol.tsdf, vol.weight, vol.color, vol.bricks[:3], vol.dims, vol.origin, VOXEL, d, w2c, K, 0.1, 5.0)
    with pytest.raises(ValueError):
        ops.tsdf_sparse_integrate(vol.tsdf, vol.weight, vol.color, vol.bricks, (big + 1, 16, 8), vol.origin, VOXEL, d, w2c, K, 0.1, 5.0)
    with pytest.raises(ValueError):
        ops.tsdf_sparse_mark(vol.flags, (24, 16, 8), vol.origin, VOXEL, d, w2c, K, 0.1, 5.0)         # flags of another grid
    with pytest.raises(ValueError):
        ops.tsdf_sparse_mark(vol.flags.cpu(), vol.dims, vol.origin, VOXEL, d, w2c, K, 0.1, 5.0)
    with pytest.raises(ValueError):
        ops.tsdf_sparse_assign(vol.flags, vol.table.long(), vol.dims)
    with pytest.raises(ValueError):
        ops.tsdf_sparse_extract_mesh(vol.tsdf, vol.weight, vol.color[:2], vol.table, vol.bricks, vol.dims, vol.origin, VOXEL)
    with pytest.raises(ValueError):
        ops.tsdf_sparse_extract_mesh(vol.tsdf, vol.weight, vol.color, vol.table[:, :1], vol.bricks, vol.dims, vol.origin, VOXEL)
    with pytest.raises(ValueError):
        T.SparseTSDFVolume((0, 0, 0), VOXEL, (0, 8, 8), device=DEV)
    with pytest.raises(ValueError, match="GB table"):
        T.SparseTSDFVolume.from_bounds((0, 0, 0), (200, 200, 200), 0.02, device=DEV)
    # nothing above changed the volume
    assert float(vol.weight.abs().max()) == 0.0 and bool((vol.tsdf == 1).all()) and vol.table.reshape(-1).tolist() == [0, 1, 2, 3]
