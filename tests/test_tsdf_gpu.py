"""GPU: cut3r_tsdf_integrate and the marching-tetrahedra extraction (csrc/tsdf.hip) against their numpy restatement
(tests/tsdf_oracle.py), bit for bit: the fused planes, the vertices, colours and faces; batch invariance of the integration; refused
arguments."""
import numpy as np
import pytest
import torch

from cut3r_slam_amd import _lib, ops
from cut3r_slam_amd import tsdf as T
from tests import tsdf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VOXEL = 0.02


def _host(vol):
    return vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(), vol.color.cpu().numpy()


def _assert_same_volume(vol, ref):
    got = _host(vol)
    for name, a, b in zip(("tsdf", "weight", "color"), got, ref):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{name}: {np.count_nonzero(a != b)} voxels differ"


def _assert_same_mesh(mesh, ref):
    v, c, f = ref
    assert mesh.vertices.shape == v.shape and mesh.faces.shape == f.shape, (mesh.vertices.shape, v.shape, mesh.faces.shape, f.shape)
    assert np.array_equal(mesh.vertices.view(np.uint32), v.view(np.uint32))
    assert np.array_equal(mesh.colors, c)
    assert np.array_equal(mesh.faces, f)


@pytest.fixture(scope="module")
def sphere():
    return O.sphere_scene(n_views=24, H=192, W=256, f=220.0)


def test_integration_matches_the_oracle_on_the_sphere(sphere):
    depth, rgb, w2c, K = sphere
    origin, dims, _ = O.sphere_grid(VOXEL)
    vol = T.TSDFVolume(origin, VOXEL, dims, device=DEV)                   # the 8-voxel default truncation
    vol.integrate(torch.from_numpy(depth).to(DEV), torch.from_numpy(w2c).to(DEV), torch.from_numpy(K), rgb=torch.from_numpy(rgb).to(DEV))
    ref = O.integrate(O.new_volume(dims), vol.origin, vol.voxel_size, depth, w2c, K, vol.trunc, vol.depth_max, rgb=rgb)
    assert (ref[1] > 0).mean() > 0.3
    _assert_same_volume(vol, ref)
    for thr in (1.0, 4.0):
        _assert_same_mesh(vol.extract_mesh(thr), O.extract(ref, vol.origin, vol.voxel_size, thr))


def _hard_scene():
    """invalid depths (0, NaN, beyond depth_max), a grid that covers only part of what the views see, cameras inside the grid (voxels
    behind them), an odd image size with a confidence map at stride 2 (its last row / column clamp), 37 views"""
    H, W, f = 95, 127, 100.0
    K = (f, f, 63.0, 47.0)
    g = np.random.default_rng(5)
    poses = list(O.sphere_poses(30, 1.4, seed=3))
    for eye, tgt in (((0.3, 0.0, 0.0), (2.0, 0.1, 0.0)), ((0.0, -0.2, 0.1), (0.0, -2.0, 0.5)), ((0.1, 0.1, 0.1), (-1.0, 1.0, 1.0)),
                     ((0.9, 0.9, 0.0), (0.0, 0.0, 0.0)), ((-1.2, 0.0, 0.0), (0.0, 1.0, 0.0)), ((0.0, 0.0, 0.2), (0.0, 0.0, -3.0)),
                     ((0.0, 1.5, 0.0), (0.0, 0.0, 0.3))):
        poses.append(O.look_at(eye, tgt))
    depth, rgb = [], []
    for P in poses:
        d, c = O.render_sphere(P, K, H, W, 0.5)
        d = np.where(d > 0, d, g.uniform(0.2, 3.0, d.shape))         # a background at random depths where the sphere is missed
        m = g.uniform(size=d.shape)
        d[m < 0.05] = 0.0
        d[(m >= 0.05) & (m < 0.1)] = np.nan
        d[(m >= 0.1) & (m < 0.13)] = 7.5                              # > depth_max
        depth.append(d)
        rgb.append(c)
    depth = np.stack(depth).astype(np.float32)
    rgb = np.stack(rgb)
    w2c = np.ascontiguousarray(np.stack(poses)[:, :3, :].reshape(-1, 12), dtype=np.float32)
    conf = g.uniform(0, 1, (len(poses), H // 2, W // 2)).astype(np.float32)
    origin, dims = (-0.45, -0.7, -0.3), (40, 61, 50)                  # not the whole sphere, not centred
    return depth, rgb, w2c, np.asarray(K, np.float32), conf, origin, dims


def test_integration_matches_the_oracle_on_invalid_depths_partial_views_and_a_confidence_gate():
    depth, rgb, w2c, K, conf, origin, dims = _hard_scene()
    B = depth.shape[0]
    vol = T.TSDFVolume(origin, VOXEL, dims, trunc_voxels=6.0, depth_max=5.0, device=DEV)
    vol.integrate(torch.from_numpy(depth).to(DEV), torch.from_numpy(w2c).to(DEV), torch.from_numpy(K).expand(B, 4),
                  rgb=torch.from_numpy(rgb).to(DEV), conf=torch.from_numpy(conf).to(DEV), conf_ds=2, conf_min=0.3)
    ref = O.integrate(O.new_volume(dims), vol.origin, vol.voxel_size, depth, w2c, K, vol.trunc, vol.depth_max, rgb=rgb, conf=conf,
                      conf_ds=2, conf_min=0.3)
    assert 0.05 < (ref[1] > 0).mean() < 1.0
    _assert_same_volume(vol, ref)
    _assert_same_mesh(vol.extract_mesh(2.0), O.extract(ref, vol.origin, vol.voxel_size, 2.0))
    # without colour: the colour planes stay as they were
    v2 = T.TSDFVolume(origin, VOXEL, dims, trunc_voxels=6.0, device=DEV).integrate(torch.from_numpy(depth).to(DEV),
                                                                                   torch.from_numpy(w2c).to(DEV), torch.from_numpy(K))
    ref2 = O.integrate(O.new_volume(dims), v2.origin, v2.voxel_size, depth, w2c, K, v2.trunc, v2.depth_max)
    _assert_same_volume(v2, ref2)
    assert float(v2.color.abs().max()) == 0.0


def _raw_integrate(vol, depth, w2c, K, rgb):
    ops.tsdf_integrate(vol.tsdf, vol.weight, vol.color, vol.origin, vol.voxel_size, depth, w2c, K, vol.trunc, vol.depth_max, rgb=rgb)


def test_batch_invariance():
    depth, rgb, w2c, K, _, origin, dims = _hard_scene()
    B = depth.shape[0]
    d, c, w = (torch.from_numpy(a).to(DEV) for a in (depth, rgb, w2c))
    Kb = torch.from_numpy(K).to(DEV).expand(B, 4).contiguous()
    one = T.TSDFVolume(origin, VOXEL, dims, device=DEV)
    batch = T.TSDFVolume(origin, VOXEL, dims, device=DEV)
    for b in range(16):
        _raw_integrate(one, d[b:b + 1], w[b:b + 1], Kb[b:b + 1], c[b:b + 1])
    _raw_integrate(batch, d[:16], w[:16], Kb[:16], c[:16])
    for a, b_ in zip(_host(one), _host(batch)):
        assert np.array_equal(a.view(np.uint32), b_.view(np.uint32))
    # 37 views: chunks of 16 + 16 + 5 (TSDFVolume.integrate) against one view at a time
    chunked = T.TSDFVolume(origin, VOXEL, dims, device=DEV).integrate(d, w, Kb, rgb=c)
    single = T.TSDFVolume(origin, VOXEL, dims, device=DEV)
    for b in range(B):
        _raw_integrate(single, d[b:b + 1], w[b:b + 1], Kb[b:b + 1], c[b:b + 1])
    assert B == 37
    for a, b_ in zip(_host(single), _host(chunked)):
        assert np.array_equal(a.view(np.uint32), b_.view(np.uint32))


def test_extraction_edge_cases_match_the_oracle():
    """a grid of one cell, a flat grid with no cell, an empty volume, a threshold of 0 (every cell valid, initial tsdf = 1: no surface)"""
    g = np.random.default_rng(2)
    for dims in ((2, 2, 2), (7, 1, 5), (9, 8, 7)):
        vol = T.TSDFVolume((0.1, -0.2, 0.3), 0.05, dims, device=DEV)
        Z, Y, X = vol.tsdf.shape
        vol.tsdf.copy_(torch.from_numpy(g.uniform(-1, 1, (Z, Y, X)).astype(np.float32)))
        vol.weight.copy_(torch.from_numpy(g.integers(0, 3, (Z, Y, X)).astype(np.float32)))
        vol.color.copy_(torch.from_numpy(g.uniform(0, 255, (3, Z, Y, X)).astype(np.float32)))
        for thr in (0.0, 1.0, 2.0):
            _assert_same_mesh(vol.extract_mesh(thr), O.extract(_host(vol), vol.origin, vol.voxel_size, thr))
    empty = T.TSDFVolume((0, 0, 0), 0.05, (10, 10, 10), device=DEV)
    m = empty.extract_mesh(0.0)
    assert m.vertices.shape == (0, 3) and m.faces.shape == (0, 3)


def test_bad_arguments_are_refused():
    lib = _lib.load()
    vol = T.TSDFVolume((0, 0, 0), VOXEL, (8, 8, 8), device=DEV)
    d = torch.ones(2, 4, 5, device=DEV)
    w2c = torch.zeros(2, 12, device=DEV)
    K = torch.ones(2, 4, device=DEV)
    p = ops._p
    s = ops._stream()

    def integ(tsdf=vol.tsdf, B=2, X=8, Y=8, Z=8, voxel=VOXEL, trunc=0.1, H=4, W=5):
        return lib.cut3r_tsdf_integrate(p(tsdf), p(vol.weight), p(vol.color), X, Y, Z, 0.0, 0.0, 0.0, voxel, p(d), None, None, B, H, W, 0,
                                        0, 1, 0.0, p(w2c), p(K), trunc, 5.0, s)

    assert integ() == 0
    torch.cuda.synchronize()
    for kw in ({"tsdf": None}, {"B": 0}, {"B": 17}, {"X": 0}, {"Y": -1}, {"X": 2048, "Y": 1024, "Z": 1024}, {"voxel": 0.0},
               {"voxel": -1.0}, {"trunc": 0.0}, {"H": 0}):
        assert integ(**kw) == 1, kw
    ws = torch.empty(lib.cut3r_tsdf_mesh_workspace_bytes(8, 8, 8), dtype=torch.uint8, device=DEV)
    totals = torch.empty(2, dtype=torch.int64, device=DEV)
    assert lib.cut3r_tsdf_mesh_workspace_bytes(0, 8, 8) == -1 and lib.cut3r_tsdf_mesh_workspace_bytes(2048, 1024, 1024) == -1
    assert lib.cut3r_tsdf_mesh_count(None, p(vol.weight), 8, 8, 8, 1.0, p(ws), ws.numel(), p(totals), s) == 1
    assert lib.cut3r_tsdf_mesh_count(p(vol.tsdf), p(vol.weight), 8, 8, 0, 1.0, p(ws), ws.numel(), p(totals), s) == 1
    assert lib.cut3r_tsdf_mesh_count(p(vol.tsdf), p(vol.weight), 8, 8, 8, 1.0, p(ws), ws.numel() - 1, p(totals), s) == 1
    assert lib.cut3r_tsdf_mesh_emit(p(vol.tsdf), None, 8, 8, 8, 0.0, 0.0, 0.0, VOXEL, p(ws), ws.numel(), None, None, None, 0, 0, s) == 1
    assert lib.cut3r_tsdf_mesh_emit(p(vol.tsdf), p(vol.color), 8, 8, 8, 0.0, 0.0, 0.0, 0.0, p(ws), ws.numel(), None, None, None, 0, 0, s) == 1
    assert lib.cut3r_tsdf_mesh_emit(p(vol.tsdf), p(vol.color), 8, 8, 8, 0.0, 0.0, 0.0, VOXEL, p(ws), ws.numel(), None, None, None, 5, 0, s) == 1
    # the wrappers
    with pytest.raises(ValueError):
        ops.tsdf_integrate(vol.tsdf, vol.weight, vol.color, vol.origin, VOXEL, torch.ones(17, 4, 5, device=DEV), torch.zeros(17, 12, device=DEV),
                           torch.ones(17, 4, device=DEV), 0.1, 5.0)
    with pytest.raises(ValueError):
        ops.tsdf_integrate(vol.tsdf, vol.weight, vol.color, vol.origin, 0.0, d, w2c, K, 0.1, 5.0)
    with pytest.raises(ValueError):
        ops.tsdf_integrate(vol.tsdf, vol.weight, vol.color, vol.origin, VOXEL, d, w2c, K, 0.0, 5.0)
    with pytest.raises(ValueError):
        ops.tsdf_integrate(vol.tsdf.cpu(), vol.weight, vol.color, vol.origin, VOXEL, d, w2c, K, 0.1, 5.0)
    with pytest.raises(ValueError):
        ops.tsdf_integrate(vol.tsdf, vol.weight, vol.color, vol.origin, VOXEL, d, w2c[:1], K, 0.1, 5.0)
    with pytest.raises(ValueError):
        ops.tsdf_extract_mesh(vol.tsdf[:, :, :4], vol.weight, vol.color, vol.origin, VOXEL)
    with pytest.raises(ValueError):
        T.TSDFVolume((0, 0, 0), VOXEL, (0, 8, 8), device=DEV)
    with pytest.raises(ValueError, match="GB"):
        T.TSDFVolume.from_bounds((0, 0, 0), (20, 20, 20), 0.006, device=DEV)
    # nothing above changed the volume
    assert float(vol.weight.abs().max()) == 0.0 and bool((vol.tsdf == 1).all())
