"""GPU: cut3r_tsdf_ray_cast / cut3r_tsdf_sparse_ray_cast (csrc/tsdf_raycast.hip) against the plain march of tests/raycast_oracle.py, bit
for bit on depth and normal (as uint32) and colour: the kernel's clipping and brick skipping must not show.  The oracle always runs on
the planes the volume under test holds, so nothing here depends on the fusion."""
import numpy as np
import pytest
import torch

from cut3r_slam_amd import _lib, ops
from cut3r_slam_amd import tsdf as T
from tests import raycast_oracle as R
from tests import tsdf_oracle as O
from tests.test_tsdf_gpu import _hard_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
H, W = R.CAST_HW


def _planes(vol):
    t, w, c = vol.to_dense() if isinstance(vol, T.SparseTSDFVolume) else (vol.tsdf, vol.weight, vol.color)
    return t.cpu().numpy(), w.cpu().numpy(), c.cpu().numpy()


def _oracle(vol, w2c, K, h, w, weight_threshold=1.0, depth_min=0.0, depth_max=None, step_voxels=0.5):
    step = float(f32(step_voxels * vol.voxel_size))
    return R.ray_cast(_planes(vol), vol.origin, vol.voxel_size, w2c, K, h, w, depth_min, vol.depth_max if depth_max is None else depth_max,
                      step, weight_threshold)


def _same(rc, ref, what=""):
    d, n, c = ref
    got_d, got_n, got_c = rc.depth.cpu().numpy(), rc.normal.cpu().numpy(), rc.color.cpu().numpy()
    assert got_d.shape == d.shape and got_n.shape == n.shape and got_c.shape == c.shape
    assert np.array_equal(got_d.view(np.uint32), d.view(np.uint32)), f"{what} depth: {np.count_nonzero(got_d != d)} pixels differ"
    assert np.array_equal(got_n.view(np.uint32), n.view(np.uint32)), f"{what} normal: {np.count_nonzero(got_n != n)} values differ"
    assert np.array_equal(got_c, c), f"{what} colour: {np.count_nonzero(got_c != c)} values differ"


def _fuse(cls, views, origin, dims, **kw):
    depth, rgb, w2c, K = views
    vol = cls(origin, R.VOXEL, dims, device=DEV, **kw)
    return vol.integrate(torch.from_numpy(depth).to(DEV), torch.from_numpy(w2c).to(DEV), torch.from_numpy(K),
                         rgb=None if rgb is None else torch.from_numpy(rgb).to(DEV))


def _poses():
    """the three poses of the CPU tests, an axis-aligned camera (with cx, cy on a pixel centre its centre ray runs along +x: two direction
    components are exactly 0) and a camera whose image only partly meets the grid"""
    eye = np.array([-1.3, 0.013, 0.007])
    return np.concatenate([R.pose_rows(list(R.POSES.values())), R.pose_rows([eye], target=eye + (1.0, 0.0, 0.0)),
                           R.pose_rows([(1.1, 0.9, 0.7)], target=(0.5, -0.9, 0.3))])


K_CENTRE = np.asarray((55.0, 55.0, 32.0, 24.0), f32)


@pytest.fixture(scope="module")
def sphere():
    views = O.sphere_scene(n_views=24, H=96, W=128, f=110.0, radius=R.RADIUS)
    origin, dims, _ = O.sphere_grid(R.VOXEL, R.RADIUS)
    assert dims == (67, 67, 67)
    dense = _fuse(T.TSDFVolume, views, origin, dims)
    sparse = _fuse(T.SparseTSDFVolume, views, origin, dims)
    assert 0 < sparse.n_bricks < sparse.table.numel()
    return dense, sparse, views


def test_dense_cast_matches_the_oracle_on_the_sphere(sphere):
    dense = sphere[0]
    w2c = _poses()
    K = np.stack([R.cast_K()] * 3 + [K_CENTRE, R.cast_K()])
    c2w = T.c2w_rows(w2c[3:4])[0].reshape(3, 4)
    assert np.count_nonzero(c2w[:, 2] == 0) == 2                        # the centre ray of the axis-aligned camera
    rc = dense.ray_cast(w2c, K, H, W)
    ref = _oracle(dense, w2c, K, H, W)
    hits = (ref[0] > 0).reshape(5, -1).sum(1)
    assert hits[0] > 900 and hits[1] > 300 and hits[2] == H * W and hits[3] > 300 and 0 < hits[4] < hits[0]
    _same(rc, ref)


def test_hard_scene_with_gate_and_holes_matches_the_oracle():
    depth, rgb, w2c, K, conf, origin, dims = _hard_scene()
    B = depth.shape[0]
    vol = T.TSDFVolume(origin, R.VOXEL, dims, trunc_voxels=6.0, depth_max=5.0, device=DEV)
    vol.integrate(torch.from_numpy(depth).to(DEV), torch.from_numpy(w2c).to(DEV), torch.from_numpy(K).expand(B, 4),
                  rgb=torch.from_numpy(rgb).to(DEV), conf=torch.from_numpy(conf).to(DEV), conf_ds=2, conf_min=0.3)
    cast = np.concatenate([w2c[[1, 12]], w2c[30:33], R.pose_rows([(1.0, -1.1, 0.8)])])      # around, inside the grid, outside
    any_hit = 0
    for thr in (1.0, 3.0):
        rc = vol.ray_cast(cast, R.cast_K(), H, W, weight_threshold=thr)
        ref = _oracle(vol, cast, R.cast_K(), H, W, weight_threshold=thr)
        _same(rc, ref, f"threshold {thr}")
        any_hit += int((ref[0] > 0).sum())
    assert any_hit > 500


def test_sparse_cast_matches_the_oracle_and_the_dense_cast(sphere):
    dense, sparse, _ = sphere
    w2c = _poses()
    K = np.stack([R.cast_K()] * 3 + [K_CENTRE, R.cast_K()])
    rs = sparse.ray_cast(w2c, K, H, W)
    _same(rs, _oracle(sparse, w2c, K, H, W), "sparse")
    rd = dense.ray_cast(w2c, K, H, W)
    hs, hd = (rs.depth > 0), (rd.depth > 0)
    assert bool((hd | ~hs).all())                                       # wherever the sparse cast hits, the dense cast hits ...
    for a, b in ((rs.depth, rd.depth), (rs.normal, rd.normal)):         # ... with the same bits
        m = hs if a.dim() == 3 else hs[..., None].expand_as(a)
        assert torch.equal(a[m].view(torch.int32), b[m].view(torch.int32))
    assert torch.equal(rs.color[hs[:, None].expand_as(rs.color)], rd.color[hs[:, None].expand_as(rd.color)])
    lost = int((hd & ~hs).sum())
    print(f"dense hits {int(hd.sum())}, of which the sparse cast misses {lost}")
    assert lost < 0.01 * int(hd.sum())


def test_odd_image_seventeen_views_batch_invariance_and_repeatability(sphere):
    dense, sparse, _ = sphere
    h, w = 37, 53
    w2c = np.ascontiguousarray(O.sphere_poses(17, 1.5, seed=7)[:, :3].reshape(-1, 12), dtype=f32)
    K = np.asarray((50.0, 48.0, 25.3, 18.9), f32)
    for vol in (dense, sparse):
        rc = vol.ray_cast(w2c, K, h, w)
        assert rc.depth.shape == (17, h, w) and int((rc.depth > 0).sum()) > 17 * 200
        _same(rc, _oracle(vol, w2c, K, h, w))
        again = vol.ray_cast(w2c, K, h, w)
        for a, b in zip(rc, again):
            assert torch.equal(a, b)
        for b in (5, 16):                                               # a view of the first launch, and the one of the second
            one = vol.ray_cast(w2c[b:b + 1], K, h, w)
            for a, q in zip(one, rc):
                assert torch.equal(a[0], q[b])
        bare = vol.ray_cast(w2c, K, h, w, normals=False, colors=False)
        assert bare.normal is None and bare.color is None and torch.equal(bare.depth, rc.depth)
        full, samples = vol.ray_cast(w2c[:2], K, h, w, count=True)
        assert torch.equal(full.depth, rc.depth[:2]) and samples.dtype == torch.int32 and int(samples.min()) >= 0
        assert int(samples[full.depth > 0].min()) >= 2                  # a hit has looked at two samples at least


def test_step_range_and_threshold_options_match_the_oracle(sphere):
    dense, sparse, _ = sphere
    w2c = _poses()[:2]
    for vol in (dense, sparse):
        for kw in ({"depth_min": 0.4, "step_voxels": 1.0}, {"depth_max": 2.3, "step_voxels": 0.3, "weight_threshold": 4.0}):
            _same(vol.ray_cast(w2c, R.cast_K(), H, W, **kw), _oracle(vol, w2c, R.cast_K(), H, W, **kw), str(kw))


def test_a_volume_fused_without_colour_casts_colour_zero(sphere):
    depth, _, w2c, K = sphere[2]
    origin, dims, _ = O.sphere_grid(R.VOXEL, R.RADIUS)
    for cls in (T.TSDFVolume, T.SparseTSDFVolume):
        vol = _fuse(cls, (depth[:8], None, w2c[:8], K), origin, dims)
        rc = vol.ray_cast(w2c[:1], K, 96, 128)
        assert int((rc.depth > 0).sum()) > 1000 and not bool(rc.color.any())
    empty = T.SparseTSDFVolume(origin, R.VOXEL, dims, device=DEV)
    rc = empty.ray_cast(w2c[:1], K, 8, 9)
    assert rc.depth.shape == (1, 8, 9) and not bool(rc.depth.any()) and not bool(rc.normal.any()) and not bool(rc.color.any())


def test_bad_arguments_are_refused(sphere):
    lib = _lib.load()
    dense, sparse, _ = sphere
    p, s = ops._p, ops._stream()
    c2w = torch.from_numpy(T.c2w_rows(_poses()[:2])).to(DEV)
    K = torch.from_numpy(np.stack([R.cast_K()] * 2)).to(DEV)
    depth = torch.zeros(2, 8, 9, device=DEV)
    o = dense.origin

    def cast(tsdf=dense.tsdf, weight=dense.weight, color=dense.color, X=67, Y=67, Z=67, voxel=R.VOXEL, c2w=c2w, K=K, B=2, H=8, W=9, t_min=0.0,
             t_max=5.0, step=0.01, out=depth):
        return lib.cut3r_tsdf_ray_cast(p(tsdf), p(weight), p(color), X, Y, Z, o[0], o[1], o[2], voxel, p(c2w), p(K), B, H, W, t_min, t_max,
                                       step, 1.0, p(out), None, None, None, s)

    def scast(tsdf=sparse.tsdf, table=sparse.table, bricks=sparse.bricks, nb=sparse.n_bricks, X=67, B=2, H=8, step=0.01, t_min=0.0, t_max=5.0):
        return lib.cut3r_tsdf_sparse_ray_cast(p(tsdf), p(sparse.weight), p(sparse.color), p(table), p(bricks), nb, X, 67, 67, o[0], o[1], o[2],
                                              R.VOXEL, p(c2w), p(K), B, H, 9, t_min, t_max, step, 1.0, p(depth), None, None, None, s)

    assert cast() == 0 and scast() == 0
    torch.cuda.synchronize()
    for kw in ({"tsdf": None}, {"weight": None}, {"color": None}, {"c2w": None}, {"K": None}, {"out": None}, {"B": 0}, {"B": 17}, {"H": 0},
               {"W": -1}, {"voxel": 0.0}, {"step": 0.0}, {"step": -0.01}, {"t_min": -0.1}, {"t_max": -1.0}, {"t_min": 2.0, "t_max": 1.0},
               {"X": 0}, {"X": 2048, "Y": 1024, "Z": 1024}):
        assert cast(**kw) == 1, kw
    for kw in ({"tsdf": None}, {"table": None}, {"bricks": None}, {"nb": 0}, {"nb": sparse.table.numel() + 1}, {"X": 0}, {"X": 2 ** 20 + 1},
               {"B": 17}, {"H": 0}, {"step": 0.0}, {"t_min": -1.0}, {"t_min": 2.0, "t_max": 1.0}):
        assert scast(**kw) == 1, kw
    # the wrappers
    with pytest.raises(ValueError):
        ops.tsdf_ray_cast(dense.tsdf, dense.weight, dense.color, o, R.VOXEL, c2w.repeat(9, 1), K.repeat(9, 1), 8, 9, 0.0, 5.0, 0.01)
    with pytest.raises(ValueError):
        ops.tsdf_ray_cast(dense.tsdf, dense.weight, dense.color, o, R.VOXEL, c2w, K, 8, 9, 0.0, 5.0, 0.0)
    with pytest.raises(ValueError):
        ops.tsdf_ray_cast(dense.tsdf, dense.weight, dense.color, o, R.VOXEL, c2w, K, 8, 9, 3.0, 1.0, 0.01)
    with pytest.raises(ValueError):
        ops.tsdf_ray_cast(dense.tsdf, dense.weight, dense.color, o, R.VOXEL, c2w.cpu(), K, 8, 9, 0.0, 5.0, 0.01)
    with pytest.raises(ValueError):
        ops.tsdf_sparse_ray_cast(sparse.tsdf, sparse.weight, sparse.color, sparse.table[:1], sparse.bricks, sparse.dims, o, R.VOXEL, c2w, K, 8, 9,
                                 0.0, 5.0, 0.01)
    with pytest.raises(ValueError):
        dense.ray_cast(_poses()[:2], np.stack([R.cast_K()] * 3), 8, 9)
