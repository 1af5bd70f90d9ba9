"""GPU: the live TSDF volume (csrc/tsdf_live.hip, tsdf.LiveTSDFVolume) against its numpy oracle (tests/tsdf_live_oracle.py), bit for bit:
the integer accumulators after adds that cross the 16-view launch boundary, the tie of the restated gates to the fp32 kernels, the
independence of order and of late allocation, update as an exact inverse, a rewritten history against a fresh fusion of the final
views (accumulators and meshes), the resolved planes, the ray cast, and refused arguments."""
import numpy as np
import pytest
import torch

from cut3r_slam_amd import ops
from cut3r_slam_amd import tsdf as T
from tests import raycast_oracle as R
from tests import tsdf_live_oracle as L
from tests import tsdf_oracle as O
from tests import tsdf_sparse_oracle as S
from tests.test_tsdf_gpu import _hard_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VOXEL = 0.02
f32 = np.float32


def _dev(*arrays):
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)


def _add(vol, ids, depth, rgb, w2c, K, **gate):
    ids = list(ids)
    d, c, w = _dev(depth[ids], None if rgb is None else rgb[ids], w2c[ids])
    Kt = torch.from_numpy(np.ascontiguousarray(K[ids] if K.ndim == 2 else K))
    gate = {k: (_dev(v[ids])[0] if k == "conf" else v) for k, v in gate.items()}
    return vol.add(ids, d, w, Kt, rgb=c, **gate)


def _assert_acc(vol, ref, offset=(0, 0, 0)):
    """to_dense_acc() (or its window at `offset` of the shape of ref) against the oracle: equal on allocated voxels, zero elsewhere,
    every voxel the oracle gives sum_q < 0 allocated"""
    i0, j0, k0 = offset
    Z, Y, X = ref.shape[1:]
    win = (slice(k0, k0 + Z), slice(j0, j0 + Y), slice(i0, i0 + X))
    got = vol.to_dense_acc()[(slice(None),) + win].cpu().numpy()
    vm = vol.allocated_mask()[win].cpu().numpy()
    for p, name in enumerate(("sum_q", "count", "sum_r", "sum_g", "sum_b")):
        assert np.array_equal(got[p][vm], ref[p][vm]), f"{name}: {np.count_nonzero(got[p][vm] != ref[p][vm])} allocated voxels differ"
    assert not got[:, ~vm].any()
    assert not ((ref[0] < 0) & ~vm).any(), "a voxel with sum_q < 0 is not allocated"
    return vm


@pytest.fixture(scope="module")
def sphere():
    """the 24 views, the grid, and the oracle's accumulators of all 24 (computed once, never written to)"""
    depth, rgb, w2c, K = O.sphere_scene()
    origin, dims, _ = O.sphere_grid(VOXEL)
    probe = T.LiveTSDFVolume(origin, VOXEL, dims, device=DEV)
    ref = L.integrate(L.new_acc(dims), probe.origin, probe.voxel_size, depth, w2c, K, probe.trunc, probe.depth_max, rgb=rgb)
    ref.setflags(write=False)
    return depth, rgb, w2c, K, origin, dims, ref


@pytest.fixture(scope="module")
def sphere_volume(sphere):
    """all 24 views, added in groups of 5, 17 (across the 16-view launch boundary) and 2"""
    depth, rgb, w2c, K, origin, dims, _ = sphere
    vol = T.LiveTSDFVolume(origin, VOXEL, dims, device=DEV)
    for ids in (range(0, 5), range(5, 22), range(22, 24)):
        _add(vol, ids, depth, rgb, w2c, K)
    return vol


def test_accumulators_equal_the_oracle_on_the_sphere(sphere, sphere_volume):
    ref = sphere[-1]
    vol = sphere_volume
    assert sorted(vol.records) == list(range(24)) and 0 < vol.n_bricks < vol.table.numel()
    vm = _assert_acc(vol, ref)
    assert 0.05 < vm.mean() < 0.9 and (ref[0] < 0).sum() > 10000 and ref[1].max() > 8
    assert vol.nbytes == (20 * 512 + 4) * vol.n_bricks + 5 * vol.table.numel() + sum(r.nbytes for r in vol.records.values())


def test_accumulators_equal_the_oracle_on_the_hard_scene():
    """per-view intrinsics, a confidence gate at stride 2, invalid depths, cameras inside the grid, 37 views in groups of 5, 17 and 15:
    the small grid of _hard_scene whole, and the virtual grid (333, 250, 181) at 0.0125 -- no multiple of the brick -- on four windows of
    48^3 voxels (its first and its last, clipped bricks, the cameras inside, one off centre), since the oracle over its 15 M voxels and
    37 views would take minutes"""
    depth, rgb, w2c, K, conf, origin, dims = _hard_scene()
    B = len(depth)
    Kb = (np.repeat(K[None], B, 0) * np.linspace(0.9, 1.1, B, dtype=f32)[:, None]).astype(f32)
    gate = dict(conf=conf, conf_ds=2, conf_min=0.3)
    cases = ((origin, dims, VOXEL, [((0, 0, 0), dims)]),
             ((-2.0, -1.5, -1.0), (333, 250, 181), 0.0125, [((0, 0, 0), (48,) * 3), ((285, 202, 133), (48,) * 3), ((140, 100, 60), (48,) * 3),
                                                            ((200, 40, 100), (48,) * 3)]))
    for org, dm, vx, windows in cases:
        vol = T.LiveTSDFVolume(org, vx, dm, trunc_voxels=6.0, depth_max=5.0, device=DEV)
        for ids in (range(0, 5), range(5, 22), range(22, B)):
            _add(vol, ids, depth, rgb, w2c, Kb, **gate)
        seen = 0
        for off, wd in windows:
            ref = L.integrate(L.new_acc(wd), vol.origin, vol.voxel_size, depth, w2c, Kb, vol.trunc, vol.depth_max, rgb=rgb, offset=off, **gate)
            vm = _assert_acc(vol, ref, off)
            seen += int((ref[1][vm] > 0).sum())
        assert seen > 5000, (dm, seen)


def test_single_views_hold_what_the_fp32_kernels_hold(sphere):
    """the gates restated in tsdf_view_sample against tsdf_fuse_voxel: one view alone in a live and in a sparse volume"""
    depth, rgb, w2c, K, origin, dims, _ = sphere
    for b in (0, 9, 23):
        live = _add(T.LiveTSDFVolume(origin, VOXEL, dims, device=DEV), [b], depth, rgb, w2c, K)
        d, c, w = _dev(depth[b:b + 1], rgb[b:b + 1], w2c[b:b + 1])
        sparse = T.SparseTSDFVolume(origin, VOXEL, dims, device=DEV).integrate(d, w, torch.from_numpy(K), rgb=c)
        assert torch.equal(live.bricks, sparse.bricks) and torch.equal(live.table, sparse.table) and live.n_bricks > 0
        acc = live.acc
        one = sparse.weight == 1
        assert int(one.sum()) > 10000 and bool(((sparse.weight == 0) | one).all())
        assert torch.equal(acc[1], sparse.weight.to(torch.int32))
        assert torch.equal(acc[0][one], torch.round(sparse.tsdf[one] * 32768.0).to(torch.int32)) and not bool(acc[0][~one].any())
        assert bool((acc[0] < 0).any())
        assert torch.equal(acc[2:].float(), sparse.color) and bool((acc[2:] > 0).any())


def test_any_order_with_late_allocation_gives_the_same_bits(sphere):
    depth, rgb, w2c, K, origin, dims, ref = sphere
    once = _add(T.LiveTSDFVolume(origin, VOXEL, dims, device=DEV), range(24), depth, rgb, w2c, K)
    late = T.LiveTSDFVolume(origin, VOXEL, dims, device=DEV)
    grew = []
    for b in np.random.default_rng(11).permutation(24):
        n0 = late.n_bricks
        _add(late, [int(b)], depth, rgb, w2c, K)
        grew.append(late.n_bricks - n0)
    assert sum(g > 0 for g in grew[1:]) >= 3, grew                        # bricks that come late and have earlier views to catch up on
    for name in ("flags", "table", "bricks", "acc"):
        assert torch.equal(getattr(late, name), getattr(once, name)), name
    _assert_acc(late, ref)


def _perturbed(w2c, ids, seed):
    """the rows of w2c with the views `ids` moved rigidly by at most 3 degrees and 5 cm (seeded), as fp32 rows"""
    g = np.random.default_rng(seed)
    out = w2c.copy()
    for b in ids:
        axis = g.normal(size=3)
        axis /= np.linalg.norm(axis)
        a = np.deg2rad(g.uniform(-3, 3))
        Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        D = np.eye(4)
        D[:3, :3] = np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx
        t = g.normal(size=3)
        D[:3, 3] = t / np.linalg.norm(t) * g.uniform(0, 0.05)
        P = np.eye(4)
        P[:3] = w2c[b].reshape(3, 4).astype(np.float64)
        out[b] = (D @ P)[:3].reshape(12).astype(f32)
    return out


MOVED = [1, 4, 7, 10, 13, 16, 19]


def _moved(depth, w2c, seed=3):
    w2 = _perturbed(w2c, MOVED, seed)
    d2 = depth.copy()
    for k, b in enumerate(MOVED):
        d2[b] = depth[b] * f32(1 + 0.03 * k)
    return d2, w2


def test_update_and_update_back_is_the_exact_inverse(sphere):
    """On the bricks of the snapshot the accumulators return to the snapshot's bits.  The bricks allocated since (for the moved views)
    are not empty: they have caught up on all 24 views, which see them in free space, so they hold what a volume that had those bricks
    from the start would hold -- the oracle of the 24 original views, checked on every allocated voxel."""
    depth, rgb, w2c, K, origin, dims, ref = sphere
    vol = _add(T.LiveTSDFVolume(origin, VOXEL, dims, device=DEV), range(24), depth, rgb, w2c, K)
    snap, bricks0 = vol.acc.clone(), vol.bricks.clone()
    d2, w2 = _moved(depth, w2c)
    vol.update(MOVED, *_dev(w2[MOVED], d2[MOVED]))
    assert vol.n_bricks > bricks0.shape[0]
    slot = vol.table.reshape(-1)[bricks0.long()].long()
    assert not torch.equal(vol.acc[:, slot], snap)
    vol.update(MOVED, *_dev(w2c[MOVED], depth[MOVED]))
    assert torch.equal(vol.acc[:, slot], snap)
    _assert_acc(vol, ref)
    # w2c alone, depth alone, and taking everything out: all zero
    vol.update(MOVED[:3], w2c=_dev(w2[MOVED[:3]])[0])
    vol.update(MOVED[:3], depth=_dev(d2[MOVED[:3]])[0])
    vol.update(MOVED[:3], *_dev(w2c[MOVED[:3]], depth[MOVED[:3]]))
    assert torch.equal(vol.acc[:, slot], snap)
    vol.remove(range(24))
    assert not vol.records and not bool(vol.acc.any()) and vol.n_bricks > bricks0.shape[0]


REMOVED = [2, 11, 22]
REPLACED = 20


def _rewritten_history(origin, voxel, dims, depth, rgb, w2c, K, d2, w2):
    vol = _add(T.LiveTSDFVolume(origin, voxel, dims, device=DEV), range(24), depth, rgb, w2c, K)
    n0 = vol.n_bricks
    vol.update(MOVED, *_dev(w2[MOVED], d2[MOVED]))
    vol.update([REPLACED], depth=_dev(d2[REPLACED:REPLACED + 1])[0])
    vol.remove(REMOVED)
    return vol, n0


def test_a_rewritten_history_equals_a_fresh_fusion_of_the_final_views(sphere):
    depth, rgb, w2c, K = sphere[:4]
    voxel = 0.03
    grid = T.LiveTSDFVolume.from_bounds((-0.5, -0.5, -0.5), (0.8, 0.5, 0.5), voxel, device=DEV)       # holds the shifted sphere too
    origin, dims = grid.origin, grid.dims
    d2, w2 = _moved(depth, w2c, seed=5)
    P = np.eye(4)
    P[:3] = w2c[REPLACED].reshape(3, 4)
    d2[REPLACED] = O.render_sphere(P, K, depth.shape[1], depth.shape[2], 0.5, center=(0.3, 0.0, 0.0))[0].astype(f32)
    assert (d2[REPLACED] > 0).sum() > 500
    vol, n0 = _rewritten_history(origin, voxel, dims, depth, rgb, w2c, K, d2, w2)
    assert vol.n_bricks > n0 and sorted(vol.records) == [b for b in range(24) if b not in REMOVED]
    final = sorted(vol.records)
    ref = L.integrate(L.new_acc(dims), vol.origin, vol.voxel_size, d2[final], w2[final], K, vol.trunc, vol.depth_max, rgb=rgb[final])
    _assert_acc(vol, ref)
    fresh = _add(T.LiveTSDFVolume(origin, voxel, dims, device=DEV), final, d2, rgb, w2, K)
    assert fresh.n_bricks <= vol.n_bricks
    again = _rewritten_history(origin, voxel, dims, depth, rgb, w2c, K, d2, w2)[0]
    assert torch.equal(again.acc, vol.acc) and torch.equal(again.bricks, vol.bricks)
    planes = L.resolve(ref)
    for thr in (1.0, 4.0):
        mesh = vol.extract_mesh(thr)
        assert len(mesh.faces) > 1000 and mesh.faces.min() == 0 and mesh.faces.max() == len(mesh.vertices) - 1
        soup = S.soup(*mesh)
        for name, other in (("fresh", fresh.extract_mesh(thr)), ("oracle", O.extract(planes, vol.origin, vol.voxel_size, thr)),
                            ("again", again.extract_mesh(thr))):
            assert len(other[2]) == len(mesh.faces) and np.array_equal(S.soup(*other), soup), (thr, name)


def test_resolved_planes_equal_the_oracle_and_stay_near_the_fp32_average(sphere, sphere_volume):
    """|tsdf_live - tsdf_fp32| <= 2^-16 + 3 n 2^-24 after n views: every q is within 2^-16 of its t and a mean does not increase that;
    the running average commits three roundings per step (the product, the sum, the quotient), each worth at most 2^-24 in the result,
    whose magnitude is at most 1, and carries the earlier error with the factor w / (w + 1) <= 1"""
    depth, rgb, w2c, K, origin, dims, ref = sphere
    vol = sphere_volume
    vm = vol.allocated_mask().cpu().numpy()
    got = [a.cpu().numpy() for a in vol.to_dense()]
    for name, a, b, init in zip(("tsdf", "weight", "color"), got, L.resolve(ref), (1, 0, 0)):
        m = vm if a.ndim == 3 else np.broadcast_to(vm, a.shape)
        assert a.dtype == np.float32 and np.array_equal(a.view(np.uint32)[m], b.view(np.uint32)[m]), name
        assert np.all(a[~m] == init), name
    n = len(depth)
    d, c, w = _dev(depth, rgb, w2c)
    dense = T.TSDFVolume(origin, VOXEL, dims, device=DEV).integrate(d, w, torch.from_numpy(K), rgb=c)
    tsdf, weight = dense.tsdf.cpu().numpy(), dense.weight.cpu().numpy()
    both = (got[1] >= 1) & (weight >= 1)
    assert both.sum() > 20000 and np.array_equal(both, vm & (weight >= 1))
    assert np.array_equal(got[1][both], weight[both])
    err = np.abs(got[0][both].astype(np.float64) - tsdf[both].astype(np.float64)).max()
    print(f"max |tsdf_live - tsdf_fp32| over {both.sum()} voxels: {err:.3e} (bound {2.0 ** -16 + 3 * n * 2.0 ** -24:.3e})")
    assert err <= 2.0 ** -16 + 3 * n * 2.0 ** -24


def test_ray_cast_equals_the_oracle_over_the_resolved_planes(sphere_volume):
    vol = sphere_volume
    H, W = R.CAST_HW
    assert (H, W) == (48, 64)
    w2c = R.pose_rows(list(R.POSES.values()))[[0, 2]]
    rc = vol.ray_cast(w2c, R.cast_K(), H, W)
    planes = tuple(a.cpu().numpy() for a in vol.to_dense())
    d, nrm, col = R.ray_cast(planes, vol.origin, vol.voxel_size, w2c, R.cast_K(), H, W, 0.0, vol.depth_max, float(f32(0.5 * vol.voxel_size)), 1.0)
    assert (d > 0).sum() > 2 * H * W // 4
    assert np.array_equal(rc.depth.cpu().numpy().view(np.uint32), d.view(np.uint32))
    assert np.array_equal(rc.normal.cpu().numpy().view(np.uint32), nrm.view(np.uint32))
    assert np.array_equal(rc.color.cpu().numpy(), col)


def test_refusals(sphere, sphere_volume):
    depth, rgb, w2c, K, origin, dims, _ = sphere
    vol = sphere_volume
    acc0 = vol.acc.clone()
    d, c, w = _dev(depth, rgb, w2c)
    Kt = torch.from_numpy(K)
    with pytest.raises(ValueError, match="already in"):
        vol.add([3], d[3:4], w[3:4], Kt, rgb=c[3:4])
    with pytest.raises(ValueError, match="not in"):
        vol.remove([24])
    with pytest.raises(ValueError, match="not in"):
        vol.update([99], w2c=w[:1])
    with pytest.raises(ValueError, match="rgb"):
        vol.add([24], d[:1], w[:1], Kt)
    with pytest.raises(ValueError, match="recorded size"):
        vol.update([0], depth=d[:1, :50])
    with pytest.raises(ValueError, match=str(ops.TSDF_SPARSE_MAX_TABLE)):
        T.LiveTSDFVolume.around((0, 0, 0), 60.0, 0.01, device=DEV)
    Kb = Kt.to(DEV).expand(24, 4).contiguous()
    args = (vol.acc, vol.bricks, vol.dims, vol.origin, vol.voxel_size)
    nb = vol.n_bricks
    with pytest.raises(ValueError, match="views per launch"):
        ops.tsdf_live_integrate(*args, d[:17], w[:17], Kb[:17], vol.trunc, vol.depth_max, rgb=c[:17])
    for bad in (torch.zeros(0, dtype=torch.int32, device=DEV), torch.arange(nb + 1, dtype=torch.int32, device=DEV),
                torch.tensor([0, nb], dtype=torch.int32, device=DEV), torch.tensor([-1, 0], dtype=torch.int32, device=DEV),
                torch.tensor([1, 1], dtype=torch.int32, device=DEV), torch.arange(2, device=DEV)):
        with pytest.raises(ValueError, match="slots"):
            ops.tsdf_live_integrate(*args, d[:2], w[:2], Kb[:2], vol.trunc, vol.depth_max, rgb=c[:2], slots=bad)
    for mask in (4, 1 << 16, -1):
        with pytest.raises(ValueError, match="subtract_mask"):
            ops.tsdf_live_integrate(*args, d[:2], w[:2], Kb[:2], vol.trunc, vol.depth_max, rgb=c[:2], subtract_mask=mask)
    # the C entry points refuse the same on their own
    from cut3r_slam_amd import _lib
    lib = _lib.load()
    p = lambda t: None if t is None else t.data_ptr()
    X, Y, Z = vol.dims

    def raw(B=2, slots=None, ns=0, mask=0, acc=vol.acc):
        return lib.cut3r_tsdf_live_integrate(p(acc), p(vol.bricks), nb, p(slots), ns, X, Y, Z, *vol.origin, vol.voxel_size, p(d), p(c), None, B,
                                             depth.shape[1], depth.shape[2], 0, 0, 1, 0.0, p(w), p(Kb), mask, vol.trunc, vol.depth_max, None)

    some = torch.arange(2, dtype=torch.int32, device=DEV)
    for kw in (dict(B=17), dict(B=0), dict(slots=some, ns=0), dict(slots=some, ns=nb + 1), dict(mask=4), dict(acc=None)):
        assert raw(**kw) != 0, kw
    assert lib.cut3r_tsdf_live_resolve(p(vol.acc), nb, p(some), nb + 1, *(p(t) for t in vol.resolve()), None) != 0
    assert lib.cut3r_tsdf_live_resolve(p(vol.acc), nb, None, 0, None, None, None, None) != 0
    torch.cuda.synchronize()
    assert torch.equal(vol.acc, acc0)
