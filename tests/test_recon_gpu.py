"""GPU: the reconstruction-metric kernels of csrc/recon.hip against the numpy oracle (tests/recon_oracle.py) -- samples and NN results bit
for bit, ICP against a known motion and the numpy loop, the metrics on analytic cases, refused arguments."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cut3r_slam_amd import _lib, ops  # noqa: E402
from cut3r_slam_amd import eval_recon as ER  # noqa: E402
from cut3r_slam_amd import tsdf as T  # noqa: E402
from tests import recon_oracle as O  # noqa: E402
from tests import tsdf_oracle as TO  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _g(a, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dt).contiguous()


def _sphere_mesh():
    depth, rgb, w2c, K = TO.sphere_scene(n_views=12, H=64, W=96, f=80.0)
    origin, dims, _ = TO.sphere_grid(voxel=0.03)
    vol = T.TSDFVolume(origin, 0.03, dims, trunc_voxels=8.0, device=DEV).integrate(depth, w2c, K, rgb=rgb)
    return vol.extract_mesh(1.0)


def _check_sampling(v, f, n, seed, stream):
    area, cdf = ops.mesh_area_cdf(_g(v), _g(f, torch.int32))
    cdf_h = cdf.cpu().numpy()
    ref = np.cumsum(O.face_areas(v, f).astype(np.float64))
    assert np.abs(cdf_h - ref).max() <= 1e-12 * ref[-1]
    assert np.array_equal(area.cpu().numpy(), O.face_areas(v, f))
    s = ops.mesh_sample(_g(v), _g(f, torch.int32), cdf, n, seed=seed, stream_id=stream).cpu().numpy()
    o = O.sample(v, f, cdf_h, n, seed=seed, stream=stream)
    assert np.array_equal(s.view(np.uint32), o.view(np.uint32)), f"{np.count_nonzero(np.any(s != o, 1))} samples differ"
    return s


def test_sampling_matches_the_oracle_bit_for_bit():
    mesh = _sphere_mesh()
    assert len(mesh.faces) > 1000
    s = _check_sampling(mesh.vertices, mesh.faces, 50000, seed=7, stream=1)
    # prefix stability on the GPU as well
    area, cdf = ops.mesh_area_cdf(_g(mesh.vertices), _g(mesh.faces, torch.int32))
    short = ops.mesh_sample(_g(mesh.vertices), _g(mesh.faces, torch.int32), cdf, 777, seed=7, stream_id=1).cpu().numpy()
    assert np.array_equal(short, s[:777])
    # degenerate faces (repeated vertices, collinear) are never picked
    v, f = O.icosphere(1)
    v = np.concatenate([v, np.float32([[0, 0, 0], [1, 1, 1], [2, 2, 2]])])
    nv = len(v)
    f = np.concatenate([f[:20], np.int32([[nv - 3, nv - 2, nv - 1], [0, 0, 1], [5, 5, 5]]), f[20:]])
    s = _check_sampling(v, f, 20000, seed=1, stream=2)
    assert np.abs(np.linalg.norm(s.astype(np.float64), axis=1) - 1).max() < 0.25   # all on the sphere's faces, none on the diagonal


def _check_nn(ref, q, max_dist=None, T=None):
    d2, idx = ops.nn_query(_g(ref), _g(q), max_dist=max_dist, transform=T)
    od2, oidx = O.nn(ref, q, max_dist, T)
    d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
    assert np.array_equal(idx, oidx), f"{np.count_nonzero(idx != oidx)} indices differ"
    assert np.array_equal(d2.view(np.uint32), od2.view(np.uint32))
    return d2, idx


def test_nn_matches_the_oracle_bit_for_bit():
    rng = np.random.default_rng(0)
    v, f = O.box_room((2.0, 1.6, 1.2), 0.05)
    ref = O.sample(v, f, np.cumsum(O.face_areas(v, f).astype(np.float64)), 20000, seed=1, stream=1)
    ref[100:200] = ref[:100]                                               # duplicates: the tie goes to the smaller index
    q = O.sample(v, f, np.cumsum(O.face_areas(v, f).astype(np.float64)), 20000, seed=1, stream=2)
    q[:50] = ref[150:200]                                                  # queries on duplicated points
    far = 50 + rng.choice(len(q) - 50, 2000, replace=False)
    q[far] = (rng.uniform(-100, 100, (2000, 3)) * 2.0).astype(np.float32)  # 10 % at ~100 x the extent, outside the grid
    d2, idx = _check_nn(ref, q)
    assert np.all(idx[:50] == np.arange(50, 100))
    _check_nn(ref, q, max_dist=0.01)
    d2e, idxe = _check_nn(ref, q, max_dist=0.0)
    assert np.all(idxe[50:][d2e[50:] > 0] == -1)
    # a transform applied on load
    M = np.eye(4)
    M[:3, :3] = O.rot([1, 1, 0.3], 0.2)
    M[:3, 3] = [0.1, -0.2, 0.05]
    _check_nn(ref, q, max_dist=0.3, T=M)
    # R with ten outliers at 100 x its extent (the robust box leaves them out of the grid), queries among them
    ref2 = ref.copy()
    ref2[rng.choice(len(ref2), 10, replace=False)] = rng.uniform(-200, 200, (10, 3)).astype(np.float32)
    q2 = q.copy()
    q2[:10] = ref2[np.flatnonzero(np.abs(ref2).max(1) > 5)][:10] + np.float32(0.5)
    _check_nn(ref2, q2)
    _check_nn(ref2, q2, max_dist=1.0)
    # Q = 1, P = 1
    _check_nn(ref[:1], q)
    _check_nn(ref, q[:1])
    _check_nn(ref[:1], q[far[:1]])


def test_nn_is_exact_at_a_million_points():
    from scipy.spatial import cKDTree
    v, f = O.box_room((4.0, 3.0, 2.5), 0.1)
    cdf = np.cumsum(O.face_areas(v, f).astype(np.float64))
    ref = O.sample(v, f, cdf, 1000000, seed=2, stream=1)
    q = O.sample(v, f, cdf, 1000000, seed=2, stream=2)
    d2, idx = ops.nn_query(_g(ref), _g(q))
    d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
    # the kd-tree's 8 nearest candidates (fp64) restated in fp32: the fp32 minimum, smallest index among ties
    _, cand = cKDTree(ref.astype(np.float64)).query(q.astype(np.float64), k=8, workers=16)
    r = ref[cand]
    dx, dy, dz = r[..., 0] - q[:, None, 0], r[..., 1] - q[:, None, 1], r[..., 2] - q[:, None, 2]
    cd = dx * dx + dy * dy + dz * dz
    best = cd.min(1)
    assert np.array_equal(d2.view(np.uint32), best.view(np.uint32))
    tie = np.where(cd == best[:, None], cand, np.iinfo(np.int64).max).min(1)
    assert np.count_nonzero(idx != tie) == 0


def test_icp_recovers_a_known_motion_and_matches_the_numpy_loop():
    v, f = O.box_room((2.0, 1.5, 1.2), 0.05)
    cdf = np.cumsum(O.face_areas(v, f).astype(np.float64))
    dst = O.sample(v, f, cdf, 6000, seed=4, stream=1)
    R = O.rot([0.3, -0.5, 0.8], np.deg2rad(2.0))
    t = np.array([0.03, -0.02, 0.04])
    src = ((O.sample(v, f, cdf, 5000, seed=4, stream=2).astype(np.float64) - t) @ R).astype(np.float32)   # M @ src on the surface
    res = ER.icp_point_to_point(src, dst, 0.1)                           # two independent samplings: the numpy loop's result
    Tn, fit, rmse, it = O.icp(src, dst, 0.1)
    assert res.iterations == it and abs(res.fitness - fit) < 1e-12 and abs(res.inlier_rmse - rmse) < 1e-9
    assert np.abs(res.transformation - Tn).max() < 1e-6
    # same points, exact correspondence: the motion itself to 1e-4
    src2 = ((dst.astype(np.float64) - t) @ R).astype(np.float32)
    res2 = ER.icp_point_to_point(src2, dst, 0.1)
    dR = res2.transformation[:3, :3] @ R.T
    assert np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1)) < 1e-4 and np.abs(res2.transformation[:3, 3] - t).max() < 1e-4
    # the moments are the same bits on every run
    g = ops.NNGrid(_g(dst), 5000)
    d2, idx = g.query(_g(src), 0.1)
    a, b = g.moments(_g(src), d2, idx).cpu().numpy(), g.moments(_g(src), d2, idx).cpu().numpy()
    assert np.array_equal(a, b)


def _plane(offset=0.0, n=100):
    v, f = O.grid_quad([0, 0, offset], [1, 0, 0], [0, 1, 0], n, n)
    return T.Mesh(v.astype(np.float32), np.zeros((len(v), 3), np.uint8), f.astype(np.int32))


def test_metrics_on_analytic_planes():
    base = _plane()
    r = ER.calc_3d_metric(_plane(0.01), base, align=False)
    assert 1.00 <= r["accuracy"] <= 1.02 and 1.00 <= r["completion"] <= 1.02 and r["completion_ratio"] == 100.0
    assert ER.calc_3d_metric(_plane(0.049), base, align=False)["completion_ratio"] == 100.0
    assert ER.calc_3d_metric(_plane(0.051), base, align=False)["completion_ratio"] == 0.0
    # GPU metrics == oracle metrics on the same samples
    rec = ER.sample_surface(_plane(0.02), 20000, stream=1)
    gt = ER.sample_surface(base, 20000, stream=2)
    rh, gh = rec.cpu().numpy(), gt.cpu().numpy()
    acc = np.sqrt(O.nn(gh, rh)[0].astype(np.float64)).mean()
    dc = np.sqrt(O.nn(rh, gh)[0].astype(np.float64))
    assert abs(ER.accuracy(gt, rec) - acc) <= 1e-12 * acc
    assert abs(ER.completion(gt, rec) - dc.mean()) <= 1e-12 * dc.mean()
    ratio = float((dc < 0.0201).mean())
    assert 0.05 < ratio < 0.95 and abs(ER.completion_ratio(gt, rec, 0.0201) - ratio) <= 1e-12 * ratio
    cd, d1, d2 = ER.chamfer_distance(gh, rh, 0.015)
    assert np.all(d1 == 0.015) and np.all(d2 == 0.015) and abs(cd - 0.015) < 1e-15
    cdr, r1, r2, _, _ = ER.chamfer_distance_RMSE(gh, rh, 0.5)
    d1o = np.minimum(np.sqrt(O.nn(gh, rh)[0].astype(np.float64)), 0.5)
    assert abs(r1 - np.sqrt((d1o * d1o).mean())) <= 1e-12 * r1 and cdr == 0.5 * r1 + 0.5 * r2


def test_refused_arguments():
    lib = _lib.load()
    p = _g(np.zeros((4, 3), np.float32))
    with pytest.raises(ValueError):
        ops.nn_query(p, p, max_dist=-1.0)
    with pytest.raises(ValueError):
        ops.nn_query(p, _g(np.float32([[np.nan, 0, 0]])))
    with pytest.raises(ValueError):
        ops.nn_query(_g(np.zeros((0, 3), np.float32)), p)
    with pytest.raises(ValueError):
        ops.mesh_area_cdf(p, _g(np.int32([[0, 1, 4]]), torch.int32))
    with pytest.raises(ValueError):
        ops.mesh_sample(p, _g(np.int32([[0, 1, 2]]), torch.int32), _g(np.zeros(1), torch.float64), 0)
    assert lib.cut3r_nn_workspace_bytes(0, 5) == -1 and lib.cut3r_nn_workspace_bytes(5, -1) == -1
    nb = lib.cut3r_nn_workspace_bytes(4, 4)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    out = torch.empty(4, device=DEV)
    idx = torch.empty(4, dtype=torch.int32, device=DEV)
    s = ops._stream()
    assert lib.cut3r_nn_build(ops._p(p), 0, ops._p(ws), nb, s) == 1
    assert lib.cut3r_nn_build(ops._p(p), 4, ops._p(ws), 16, s) == 1
    assert lib.cut3r_nn_build(ops._p(p), 4, ops._p(ws), nb, s) == 0
    assert lib.cut3r_nn_query(4, ops._p(p), 4, None, -1.0, ops._p(out), ops._p(idx), ops._p(ws), nb, s) == 1
    assert lib.cut3r_nn_query(4, ops._p(p), 4, None, float("nan"), ops._p(out), ops._p(idx), ops._p(ws), nb, s) == 1
    assert lib.cut3r_nn_query(4, ops._p(p), 0, None, 1.0, ops._p(out), ops._p(idx), ops._p(ws), nb, s) == 1
    assert lib.cut3r_nn_query(4, ops._p(p), 4, None, 1.0, ops._p(out), ops._p(idx), ops._p(ws), nb - 1, s) == 1
    assert lib.cut3r_mesh_area_cdf(ops._p(p), 4, None, 0, None, None, None, 0, s) == 1
    assert lib.cut3r_mesh_cdf_workspace_bytes(0) == -1
    assert lib.cut3r_mesh_sample(ops._p(p), 4, ops._p(idx), 1, ops._p(out), 0, 0, 0, ops._p(out), s) == 1
    assert lib.cut3r_icp_moments_workspace_bytes(0) == -1
    assert lib.cut3r_icp_moments(ops._p(p), 4, ops._p(p), 4, None, ops._p(out), ops._p(idx), None, ops._p(ws), nb, s) == 1
    torch.cuda.synchronize()
