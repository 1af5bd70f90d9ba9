"""GPU: the mesh depth rasteriser of csrc/raster.hip against the numpy oracle (tests/raster_oracle.py) bit for bit, one room too large for
the oracle against geometry, the depth-L1 sums, points_in_view, the 2-D metric on analytic planes, vertex visibility and culling, refused
arguments."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cut3r_slam_amd import _lib, ops  # noqa: E402
from cut3r_slam_amd import eval_recon as ER  # noqa: E402
from cut3r_slam_amd import mesh_render as MR  # noqa: E402
from cut3r_slam_amd import tsdf as T  # noqa: E402
from tests import raster_oracle as R  # noqa: E402
from tests import recon_oracle as O  # noqa: E402
from tests.test_raster_cpu import depth_bound  # noqa: E402
from tests.test_recon_gpu import _sphere_mesh  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _g(a, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dt).contiguous()


def _render(v, f, w2c, K, H, W, **kw):
    d, i = ops.mesh_raster(_g(v), _g(f, torch.int32), w2c, K, H, W, face_id=True, **kw)
    return d.cpu().numpy(), i.cpu().numpy()


def _check(v, f, w2c, K, H, W, **kw):
    d, i = _render(v, f, w2c, K, H, W, **kw)
    od, oi = R.render(v, f, w2c, K, H, W, **kw)
    assert np.array_equal(d.view(np.uint32), od.view(np.uint32)), f"{np.count_nonzero(d != od)} depths differ"
    assert np.array_equal(i, oi), f"{np.count_nonzero(i != oi)} face ids differ"
    only = ops.mesh_raster(_g(v), _g(f, torch.int32), w2c, K, H, W, **kw).cpu().numpy()          # without the face-id image
    assert np.array_equal(only.view(np.uint32), d.view(np.uint32))
    return d, i


def _orbit(n, dist, seed=0):
    rng = np.random.default_rng(seed)
    return np.stack([R.look_at(dist * e / np.linalg.norm(e), rng.normal(size=3) * 0.1, up=rng.normal(size=3)) for e in rng.normal(size=(n, 3))])


def test_sphere_mesh_matches_the_oracle_bit_for_bit():
    mesh = _sphere_mesh()
    assert len(mesh.faces) > 1000
    w2c = _orbit(3, 1.4)
    K = np.float32([[70, 70, 31.5, 23.5], [55, 60, 30.0, 25.0], [90, 80, 35.5, 20.0]])       # a K per view, H != W
    d, i = _check(mesh.vertices, mesh.faces, w2c, K, 48, 64)
    assert np.count_nonzero(d) > 1500
    # seen from the centre of the sphere (faces all around, behind and across the camera plane)
    _check(mesh.vertices, mesh.faces, R.look_at([0.02, -0.01, 0.03], [1, 0.2, 0.1])[None], K[:1], 48, 64)
    # B = 5 equals five single launches, a second run gives the same bits
    w5 = _orbit(5, 1.2, seed=3)
    K5 = [66.0, 66.0, 31.5, 23.5]
    d5, i5 = _render(mesh.vertices, mesh.faces, w5, K5, 48, 64)
    for b in range(5):
        d1, i1 = _render(mesh.vertices, mesh.faces, w5[b:b + 1], K5, 48, 64)
        assert np.array_equal(d1[0].view(np.uint32), d5[b].view(np.uint32)) and np.array_equal(i1[0], i5[b])
    d5b, i5b = _render(mesh.vertices, mesh.faces, w5, K5, 48, 64)
    assert np.array_equal(d5.view(np.uint32), d5b.view(np.uint32)) and np.array_equal(i5, i5b)
    # more views than one launch takes
    w20 = _orbit(20, 1.3, seed=4)
    d20, _ = _render(mesh.vertices, mesh.faces, w20, K5, 24, 32)
    d17, _ = _render(mesh.vertices, mesh.faces, w20[17:18], K5, 24, 32)
    assert np.array_equal(d20[17], d17[0]) and np.count_nonzero(d20[19]) > 100
    # a face-permuted copy: the same depth, and the same faces wherever the minimum is unique
    perm = np.random.default_rng(1).permutation(len(mesh.faces))
    dp, ip = _render(mesh.vertices, mesh.faces[perm], w5, K5, 48, 64)
    assert np.array_equal(dp.view(np.uint32), d5.view(np.uint32))
    mapped = np.where(ip >= 0, perm[np.maximum(ip, 0)], -1)
    assert np.array_equal(mapped == -1, i5 == -1)
    differ = mapped != i5
    if differ.any():                                  # two faces at the very same z (a pixel centre on a shared edge): both hit it
        v = mesh.vertices
        for b, y, x in zip(*np.nonzero(differ)):
            two = np.int32([mesh.faces[mapped[b, y, x]], mesh.faces[i5[b, y, x]]])
            od, _ = R.render(v, two[:1], w5[b:b + 1], K5, 48, 64)
            od2, _ = R.render(v, two[1:], w5[b:b + 1], K5, 48, 64)
            assert od[0, y, x] == od2[0, y, x] == d5[b, y, x]
    assert np.count_nonzero(differ) < 0.01 * differ.size


def test_rooms_and_planes_match_the_oracle_bit_for_bit():
    v, f = O.box_room((4.0, 3.0, 2.5), 0.1)
    rng = np.random.default_rng(2)
    eyes = rng.uniform(0.2, 0.8, (2, 3)) * (4.0, 3.0, 2.5)
    w2c = np.stack([R.look_at(e, e + rng.normal(size=3), up=rng.normal(size=3)) for e in eyes])
    d, _ = _check(v, f, w2c, [40.0, 44.0, 39.5, 31.5], 64, 80)
    assert np.count_nonzero(d == 0) == 0
    # pixel centres on the lattice of a wall (ties between the faces that share an edge or a vertex)
    eye = np.array([2.0, 1.0, 1.25])
    vd, fd = O.box_room((4.0, 3.0, 2.5), 0.125)
    d, _ = _check(vd, fd, R.look_at(eye, eye + [0.0, 1.0, 0.0])[None], [64.0, 64.0, 47.0, 47.0], 96, 96)
    assert np.count_nonzero(d == 0) == 0 and np.all(d[0, 27:68, 7:88] == np.float32(2.0))
    # a coarse room: every triangle is large, most cross the camera plane
    vc, fc = O.box_room((4.0, 3.0, 2.5), 2.0)
    d, _ = _check(vc, fc, w2c, [40.0, 44.0, 39.5, 31.5], 64, 80)
    assert np.count_nonzero(d == 0) == 0
    # the floor that passes under and behind the camera; z_near / z_far
    fv = np.float32([[-50, 1.2, -50], [50, 1.2, -50], [50, 1.2, 50], [-50, 1.2, 50]])
    ff = np.int32([[0, 1, 2], [0, 2, 3]])
    d, _ = _check(fv, ff, np.eye(4)[None], [58.0, 58.0, 47.5, 47.5], 96, 96, z_far=100.0)
    assert np.count_nonzero(d[0, :48]) == 0 and np.count_nonzero(d[0, 48:]) > 3000
    _check(fv, ff, np.eye(4)[None], [58.0, 58.0, 47.5, 47.5], 96, 96, z_near=2.0, z_far=7.5)
    # duplicated and zero-area faces
    n = len(vc)
    vz = np.concatenate([vc, np.float32([[1.2, 1.0, 1.0], [1.4, 1.06, 0.92], [1.6, 1.12, 0.84]])])
    fz = np.concatenate([np.int32([[0, 0, 5], [7, 7, 7], [n, n + 1, n + 1], [n, n + 1, n + 2]]), fc, fc])
    _, i = _check(vz, fz, w2c, [40.0, 44.0, 39.5, 31.5], 64, 80)
    assert i.min() >= 4 and i.max() < 4 + len(fc)


def test_ten_million_faces_leave_no_empty_pixel():
    size = (6.0, 5.0, 3.0)
    v, f = O.box_room(size, 0.005)
    assert len(f) > 9_000_000
    rng = np.random.default_rng(5)
    eyes = rng.uniform(0.15, 0.85, (3, 3)) * size
    w2c = np.stack([R.look_at(e, e + rng.normal(size=3), up=rng.normal(size=3)) for e in eyes])
    K = [300.0, 300.0, 249.5, 249.5]
    d = ops.mesh_raster(_g(v), _g(f, torch.int32), w2c, K, 500, 500).cpu().numpy()
    assert np.count_nonzero(d == 0) == 0
    worst = max(float(np.abs(d[b] - R.box_depth(w2c[b], K, 500, 500, (0, 0, 0), size)).max()) for b in range(3))
    print(f"worst |depth - analytic| {worst:.3e} m, bound {depth_bound(size):.3e} m")
    assert worst <= depth_bound(size)


def test_depth_l1_and_points_in_view_match_the_oracle():
    mesh = _sphere_mesh()
    w2c = _orbit(4, 1.4, seed=7)
    K = [70.0, 70.0, 31.5, 23.5]
    gt, _ = R.render(mesh.vertices, mesh.faces, w2c, K, 48, 64)
    v2, f2 = O.icosphere(3, radius=0.52)
    ours, _ = R.render(v2, f2, w2c, K, 48, 64)
    ours[3] = 0                                       # a view the reconstruction is empty in
    ref = R.depth_l1(gt, ours)
    a = ops.depth_l1(_g(gt), _g(ours)).cpu().numpy()
    b = ops.depth_l1(_g(gt), _g(ours)).cpu().numpy()
    assert np.array_equal(a, b)
    assert np.array_equal(a[:, 0], ref[:, 0]) and a[3, 0] == 0 and a[3, 1] == 0 and ref[0, 0] > 500
    assert np.abs(a[:, 1] - ref[:, 1]).max() <= 1e-12 * ref[:, 1].max()
    # points in view: 20 cameras (more than a launch takes) over the room's surface samples, points behind and on the border included
    rv, rf = O.box_room((4.0, 3.0, 2.5), 0.1)
    pts = O.sample(rv, rf, np.cumsum(O.face_areas(rv, rf).astype(np.float64)), 30000, seed=3, stream=1)
    rng = np.random.default_rng(8)
    eyes = rng.uniform(0.2, 0.8, (20, 3)) * (4.0, 3.0, 2.5)
    cams = np.stack([R.look_at(e, e + rng.normal(size=3), up=rng.normal(size=3)) for e in eyes])
    Kp = [300.0, 300.0, 249.5, 249.5]
    got = ops.points_in_view(_g(pts), cams, Kp, 500, 500).cpu().numpy()
    want = R.points_in_view(pts, cams, Kp, 500, 500)
    assert np.array_equal(got, want) and want.min() > 100
    assert np.array_equal(ops.points_in_view(_g(pts), cams, Kp, 500, 500, edge=120.5).cpu().numpy(), R.points_in_view(pts, cams, Kp, 500, 500, 120.5))
    c2w = np.linalg.inv(cams[0])
    assert ER.check_proj(pts, 500, 500, 300.0, 300.0, 249.5, 249.5, c2w) is True
    behind = (c2w @ np.array([0.0, 0.0, -1.0, 1.0]))[:3][None].astype(np.float32)
    assert ER.check_proj(behind, 500, 500, 300.0, 300.0, 249.5, 249.5, c2w) is False


def test_sample_views_equals_the_oracle():
    v, f = O.box_room((6.0, 5.0, 3.0), 0.5)
    mesh = T.Mesh(v, np.zeros_like(v, dtype=np.uint8), f)
    ext, M = ER.get_cam_position(mesh)
    oext, oM = R.get_cam_position(v)
    assert np.array_equal(ext, oext) and np.array_equal(M, oM)
    unseen = np.float32([[3.0, 2.5, 0.0], [0.5, 0.5, 3.0]])
    a = ER.sample_views(ext, M, 40, unseen=unseen, seed=1)
    assert np.array_equal(a, R.sample_views(ext, M, 40, unseen=unseen, seed=1))
    assert np.array_equal(a[:9], ER.sample_views(ext, M, 9, unseen=unseen, seed=1))
    assert np.array_equal(ER.sample_views(ext, M, 5, seed=2), R.sample_views(ext, M, 5, seed=2))
    cloud, _ = O.icosphere(3, radius=20.0, center=(3.0, 2.5, 1.9))
    with pytest.raises(RuntimeError):
        ER.sample_views(ext, M, 2, unseen=cloud, max_tries=20)


def _plane(z, half, n=20):
    v, f = O.grid_quad([-half, -half, z], [2 * half, 0, 0], [0, 2 * half, 0], n, n)
    return T.Mesh(v.astype(np.float32), np.zeros((len(v), 3), np.uint8), f.astype(np.int32))


def test_calc_2d_metric_on_analytic_planes():
    views = np.eye(4)[None].repeat(2, 0)
    views[1, :3, 3] = [0.05, -0.03, 0.0]              # a second head-on camera, shifted sideways
    r = ER.calc_2d_metric(_plane(2.01, 2.0), _plane(2.0, 2.0), align=False, views=views)
    assert set(r) == {"depth l1"} and abs(r["depth l1"] - 1.0) < 1e-3
    # a reconstruction smaller than the GT: the pixels it does not cover are left out
    r = ER.calc_2d_metric(_plane(2.01, 0.5), _plane(2.0, 2.0), align=False, views=views)
    assert abs(r["depth l1"] - 1.0) < 1e-3
    # larger than the GT: the overhang counts with gt = 0.  Head-on from the origin the GT covers |j - 249.5| <= 75: 150 x 150 pixels
    r = ER.calc_2d_metric(_plane(2.01, 2.0), _plane(2.0, 0.5), align=False, views=views[:1])
    want = 100 * (150 * 150 * 0.01 + (250000 - 150 * 150) * 2.01) / 250000
    assert abs(r["depth l1"] - want) < 1e-3
    # a mesh against itself: exactly 0, with and without the alignment, with sampled views as well
    v, f = O.box_room((4.0, 3.0, 2.5), 0.1)
    room = T.Mesh(v, np.zeros_like(v, dtype=np.uint8), f)
    assert ER.calc_2d_metric(room, room, align=False, n_imgs=5)["depth l1"] == 0.0
    assert ER.calc_2d_metric(room, room, align=True, n_imgs=5)["depth l1"] == 0.0
    assert ER.calc_2d_metric(_plane(2.0, 2.0), _plane(2.0, 2.0), views=views)["depth l1"] == 0.0
    # a reconstruction no view sees: nan; one view of two sees it: that view alone
    assert math.isnan(ER.calc_2d_metric(_plane(-2.0, 2.0), _plane(2.0, 2.0), align=False, views=views)["depth l1"])
    turned = views.copy()
    turned[1, :3, :3] = np.diag([1.0, -1.0, -1.0])    # looks the other way
    r = ER.calc_2d_metric(_plane(2.01, 2.0), _plane(2.0, 2.0), align=False, views=turned)
    assert abs(r["depth l1"] - 1.0) < 1e-3
    # eval_recon: the 3-D keys alone by default, 'depth l1' with eval_2d
    assert set(ER.eval_recon(room, room, samples=2000)) == {"accuracy", "completion", "completion_ratio"}
    assert set(ER.eval_recon(room, room, samples=2000, eval_2d=True, n_imgs=2)) == {"accuracy", "completion", "completion_ratio", "depth l1"}


def test_visible_vertices_cull_mesh_and_unseen_points(tmp_path):
    nv, nf = O.grid_quad([-1, -1, 2], [2, 0, 0], [0, 2, 0], 8, 8)
    fv, ff = O.grid_quad([-3, -3, 3], [6, 0, 0], [0, 6, 0], 24, 24)
    v = np.concatenate([nv, fv]).astype(np.float32)
    f = np.concatenate([nf, ff + len(nv)]).astype(np.int32)
    mesh = T.Mesh(v, np.zeros_like(v, dtype=np.uint8), f)
    K, H, W = [58.0, 58.0, 47.5, 47.5], 96, 96
    w2c = np.eye(4)[None]
    seen = MR.visible_vertices(mesh, w2c, K, H, W)
    depth, _ = R.render(v, f, w2c, K, H, W)
    assert np.array_equal(seen, R.vertex_visible(v, depth, w2c, K))
    far = v[len(nv):]
    hidden = (np.abs(far[:, :2]) < 1.4).all(1)        # behind the near wall (its shadow at 3 m is +-1.5 m)
    outside = (np.abs(far[:, :2]) > 2.6).any(1)       # outside the image (+-2.46 m at 3 m)
    beside = (np.abs(far[:, :2]) > 1.6).any(1) & (np.abs(far[:, :2]) < 2.4).all(1)
    assert seen[:len(nv)].all() and not seen[len(nv):][hidden].any() and not seen[len(nv):][outside].any() and seen[len(nv):][beside].all()
    culled = MR.cull_mesh(mesh, w2c, K, H, W)
    keep = seen[f].any(1)
    assert len(culled.faces) == keep.sum() and 0 < keep.sum() < len(f)
    assert np.array_equal(culled.vertices[culled.faces], v[f[keep]])          # the same triangles, in order
    pts = MR.unseen_points(mesh, w2c, K, H, W, count=3000, seed=1)
    assert pts.shape == (3000, 3) and np.all(pts[:, 2] == 3.0)                 # on the far wall only
    cell = 0.25                                                                # each point lies in a dropped cell of the far wall
    dropped = {tuple(np.floor((v[t].mean(0)[:2] + 3) / cell).astype(int)) for t in f[~keep]}
    assert all(tuple(np.floor((p[:2] + 3) / cell).astype(int)) in dropped for p in pts[:500])
    # views that see everything: the mesh unchanged, no unseen points
    both = np.stack([np.eye(4), R.look_at([0, 0, 2.5], [0, 0, 3.0], up=(0, -1, 0)), R.look_at([0, 0, 9.0], [0, 0, 3.0], up=(0, -1, 0))])
    all_seen = MR.cull_mesh(mesh, both, [20.0, 20.0, 47.5, 47.5], H, W)
    assert np.array_equal(all_seen.vertices, v) and np.array_equal(all_seen.faces, f)
    assert MR.unseen_points(mesh, both, [20.0, 20.0, 47.5, 47.5], H, W, count=10).shape == (0, 3)
    # render_depth takes c2w; the CLI writes the culled mesh and the unseen cloud
    d = MR.render_depth(mesh, np.eye(4)[None], K, H, W).cpu().numpy()
    assert np.array_equal(d, depth)
    T.write_ply(str(tmp_path / "gt.ply"), mesh)
    (tmp_path / "traj.txt").write_text("0.0 0 0 0 0 0 0 1\n")
    assert MR.main(["cull", str(tmp_path / "gt.ply"), str(tmp_path / "traj.txt"), "--calib", "58 58 47.5 47.5", "--size", "96", "96", "--out",
                    str(tmp_path / "out"), "--count", "1000"]) == 0
    got = T.read_ply(str(tmp_path / "out" / "gt_culled.ply"))
    assert np.array_equal(got.vertices, culled.vertices) and np.array_equal(got.faces, culled.faces)
    cloud = np.load(tmp_path / "out" / "gt_pc_unseen.npy")
    assert cloud.shape == (1000, 3) and np.array_equal(cloud, MR.unseen_points(mesh, w2c, K, H, W, count=1000))
    # the cloud next to the GT is what calc_2d_metric picks up: no sampled view sees it
    os.replace(tmp_path / "out" / "gt_pc_unseen.npy", tmp_path / "gt_pc_unseen.npy")
    assert np.array_equal(ER._unseen_next_to(str(tmp_path / "gt.ply")), cloud)


def test_refused_arguments():
    lib = _lib.load()
    v = _g(np.float32([[0, 0, 2], [1, 0, 2], [0, 1, 2], [1, 1, 2]]))
    f = _g(np.int32([[0, 1, 2], [1, 3, 2]]), torch.int32)
    w2c, K = np.eye(4)[None], [50.0, 50.0, 15.5, 15.5]
    for bad in (dict(z_near=-1.0), dict(z_near=2.0, z_far=2.0), dict(z_far=float("nan")), dict(z_far=float("inf"))):
        with pytest.raises(ValueError):
            ops.mesh_raster(v, f, w2c, K, 32, 32, **bad)
    with pytest.raises(ValueError):
        ops.mesh_raster(v, _g(np.int32([[0, 1, 4]]), torch.int32), w2c, K, 32, 32)
    with pytest.raises(ValueError):
        ops.mesh_raster(v, f, w2c, [0.0, 50.0, 15.5, 15.5], 32, 32)
    with pytest.raises(ValueError):
        ops.mesh_raster(v, f, w2c, [50.0, 50.0, float("nan"), 15.5], 32, 32)
    with pytest.raises(ValueError):
        ops.mesh_raster(v, f, w2c, K, 0, 32)
    with pytest.raises(ValueError):
        ops.mesh_raster(v, f, np.zeros((1, 7)), K, 32, 32)
    with pytest.raises(ValueError):
        ops.mesh_raster(v.cpu(), f, w2c, K, 32, 32)
    with pytest.raises(ValueError):
        ops.depth_l1(torch.zeros(1, 4, 4, device=DEV), torch.zeros(1, 4, 5, device=DEV))
    with pytest.raises(ValueError):
        ops.points_in_view(v, w2c, K, 32, 32, edge=-1.0)
    with pytest.raises(ValueError):
        ops.mesh_vertex_visible(v, torch.zeros(2, 32, 32, device=DEV), w2c, K)
    assert lib.cut3r_mesh_raster_workspace_bytes(0, 1, 32, 32) == -1 and lib.cut3r_mesh_raster_workspace_bytes(2, 17, 32, 32) == -1
    assert lib.cut3r_mesh_raster_workspace_bytes(2, 1, 0, 32) == -1 and lib.cut3r_mesh_raster_workspace_bytes(2, 1, 32, 65536) == -1
    nb = lib.cut3r_mesh_raster_workspace_bytes(2, 1, 32, 32)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    T12, K4 = _g(np.eye(4)[:3].reshape(1, 12)), _g(np.float32([K]))
    depth = torch.empty(1, 32, 32, device=DEV)
    cnt = torch.empty(1, dtype=torch.int32, device=DEV)
    flags = torch.zeros(4, dtype=torch.uint8, device=DEV)
    out = torch.empty(1, 2, dtype=torch.float64, device=DEV)
    s, p = ops._stream(), ops._p
    ok = (p(v), 4, p(f), 2, p(T12), p(K4), 1, 32, 32, 0.0, 20.0, p(depth), None, p(ws), nb, s)

    def call(**kw):
        a = list(ok)
        for k, val in kw.items():
            a[int(k[1:])] = val
        return lib.cut3r_mesh_raster(*a)

    assert call() == 0
    assert call(a0=None) == 1 and call(a2=None) == 1 and call(a4=None) == 1 and call(a5=None) == 1 and call(a11=None) == 1 and call(a13=None) == 1
    assert call(a1=0) == 1 and call(a3=0) == 1 and call(a6=0) == 1 and call(a6=17) == 1 and call(a7=0) == 1 and call(a8=70000) == 1
    assert call(a9=-0.5) == 1 and call(a9=float("nan")) == 1 and call(a10=0.0) == 1 and call(a9=3.0, a10=3.0) == 1 and call(a14=nb - 1) == 1
    assert lib.cut3r_depth_l1_workspace_bytes(0) == -1
    wb = lib.cut3r_depth_l1_workspace_bytes(1)
    assert lib.cut3r_depth_l1(p(depth), p(depth), 1, 32, 32, p(out), p(ws), wb, s) == 0
    assert lib.cut3r_depth_l1(p(depth), p(depth), 0, 32, 32, p(out), p(ws), wb, s) == 1
    assert lib.cut3r_depth_l1(p(depth), None, 1, 32, 32, p(out), p(ws), wb, s) == 1
    assert lib.cut3r_depth_l1(p(depth), p(depth), 1, 32, 32, p(out), p(ws), wb - 1, s) == 1
    assert lib.cut3r_points_in_view(p(v), 4, p(T12), p(K4), 1, 32, 32, 10.0, p(cnt), s) == 0
    assert lib.cut3r_points_in_view(p(v), 0, p(T12), p(K4), 1, 32, 32, 10.0, p(cnt), s) == 1
    assert lib.cut3r_points_in_view(p(v), 4, p(T12), p(K4), 17, 32, 32, 10.0, p(cnt), s) == 1
    assert lib.cut3r_points_in_view(p(v), 4, p(T12), p(K4), 1, 32, 32, -1.0, p(cnt), s) == 1
    assert lib.cut3r_points_in_view(p(v), 4, p(T12), p(K4), 1, 32, 32, 10.0, None, s) == 1
    assert lib.cut3r_mesh_vertex_visible(p(v), 4, p(depth), p(T12), p(K4), 1, 32, 32, 0.03, 20.0, p(flags), s) == 0
    assert lib.cut3r_mesh_vertex_visible(p(v), 4, p(depth), p(T12), p(K4), 1, 32, 32, -0.1, 20.0, p(flags), s) == 1
    assert lib.cut3r_mesh_vertex_visible(p(v), 4, p(depth), p(T12), p(K4), 1, 32, 32, 0.03, 0.0, p(flags), s) == 1
    assert lib.cut3r_mesh_vertex_visible(p(v), 4, None, p(T12), p(K4), 1, 32, 32, 0.03, 20.0, p(flags), s) == 1
    assert lib.cut3r_mesh_vertex_visible(p(v), 4, p(depth), p(T12), p(K4), 0, 32, 32, 0.03, 20.0, p(flags), s) == 1
    torch.cuda.synchronize()
