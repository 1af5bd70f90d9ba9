"""CPU: the pixel rule of csrc/raster.hip as tests/raster_oracle.py restates it, against geometry (closed rooms, analytic box and plane
depths, triangles across the camera plane, ties, degenerate faces), and the host side of the 2-D metric (check_proj against a plain fp64
pinhole projection, the view sampler).  Curved meshes are left to the GPU tests' bit equality: a faceted sphere is not its analytic
surface at grazing pixels."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import raster_oracle as R  # noqa: E402
from tests import recon_oracle as O  # noqa: E402

H = W = 96
K = [58.0, 58.0, W / 2.0 - 0.5, H / 2.0 - 0.5]
SIZE = (4.0, 3.0, 2.5)
# |depth - analytic| in units of 2^-24 x the room's diagonal (the size of the fp32 inputs whose rounding is all that is left once the edge
# values are fp64): achieved by the oracle on the six views below 1.053e-6 m = 3.16 units; the bound, here and on the GPU, is 4 x that
ACHIEVED_UNITS = 3.16
BOUND_UNITS = 4 * ACHIEVED_UNITS


def depth_bound(size):
    return BOUND_UNITS * 2.0 ** -24 * float(np.linalg.norm(size))


def _interior_views(n, seed=0):
    rng = np.random.default_rng(seed)
    views = []
    for _ in range(n):
        eye = rng.uniform(0.2, 0.8, 3) * SIZE
        views.append(R.look_at(eye, eye + rng.normal(size=3), up=rng.normal(size=3)))
    return np.stack(views)


def test_closed_room_has_no_empty_pixel_and_matches_the_analytic_depth():
    v, f = O.box_room(SIZE, 0.1)
    w2c = _interior_views(6)
    depth, fid = R.render(v, f, w2c, K, H, W)
    assert np.count_nonzero(depth == 0) == 0 and fid.min() >= 0
    worst = 0.0
    for b in range(len(w2c)):
        ref = R.box_depth(w2c[b], K, H, W, (0, 0, 0), SIZE)
        worst = max(worst, float(np.abs(depth[b] - ref).max()))
    print(f"worst |depth - analytic| {worst:.3e} m = {worst / (2.0 ** -24 * np.linalg.norm(SIZE)):.2f} units, bound {depth_bound(SIZE):.3e} m")
    # an all-fp32 prototype of the rule lost 2.2e-4 m at 3.9 m to the cancellation in its triple products (its bound: 1e-3 m for rooms
    # up to 5 m across).  With the edge values in fp64 only the fp32 rounding of the inputs and of z is left: see ACHIEVED_UNITS
    assert worst <= depth_bound(SIZE) <= 1e-3


def test_pixel_centres_on_shared_edges_leave_no_crack():
    # camera on a lattice point, axis-aligned, focal chosen so that pixel centres fall exactly on the 0.1 m lattice of the wall at 1.5 m
    v, f = O.box_room(SIZE, 0.1)
    eye = np.array([2.0, 1.5, 1.0])
    w2c = R.look_at(eye, eye + [0.0, 1.0, 0.0])[None]
    Kl = [60.0, 60.0, 47.0, 47.0]                  # (j - 47) / 60 * 1.5 = (j - 47) * 0.025: every fourth column is a lattice line
    depth, _ = R.render(v, f, w2c, Kl, H, W)
    assert np.count_nonzero(depth == 0) == 0
    wall = depth[0, 40:56, 30:66]                  # well inside the wall y = 3 (1.5 m ahead)
    assert np.abs(wall - 1.5).max() < 5e-5
    # the same on a dyadic lattice (step 1/8, focal 64, wall at 2 m: (j - 47) / 64 * 2 is a lattice line every fourth column): every
    # number is exact, so the edge values on shared edges and at shared vertices are exactly 0 and only the inclusive test fills them
    v, f = O.box_room(SIZE, 0.125)
    eye = np.array([2.0, 1.0, 1.25])
    depth, fid = R.render(v, f, R.look_at(eye, eye + [0.0, 1.0, 0.0])[None], [64.0, 64.0, 47.0, 47.0], H, W)
    assert np.count_nonzero(depth == 0) == 0
    assert np.all(depth[0, 27:68, 7:88] == np.float32(2.0))


def test_plane_from_both_sides_and_the_depth_range():
    pv, pf = O.grid_quad([-1, -1, 0], [2, 0, 0], [0, 2, 0], 7, 5)
    pv = pv.astype(np.float32)
    above = R.look_at([0.1, 0.05, 2.0], [0.1, 0.05, 0.0], up=(0, 1, 0))
    below = R.look_at([0.1, 0.05, -2.0], [0.1, 0.05, 0.0], up=(0, 1, 0))
    d, _ = R.render(pv, pf, np.stack([above, below]), K, H, W)
    # mirrored cameras: the image from below is the image from above with the columns reversed about cx
    assert np.count_nonzero(d[0]) > 1000
    assert np.abs(d[0][d[0] > 0] - 2.0).max() < 1e-5 and np.abs(d[1][d[1] > 0] - 2.0).max() < 1e-5
    assert np.array_equal(d[0] > 0, (d[1] > 0)[:, ::-1])
    # winding reversed: the same image
    d2, _ = R.render(pv, pf[:, ::-1], above[None], K, H, W)
    assert np.array_equal(d2[0], d[0])
    # z_far / z_near clip to 0; z == z_far is kept, z == z_near is not
    assert np.count_nonzero(R.render(pv, pf, above[None], K, H, W, z_far=1.9)[0]) == 0
    assert np.count_nonzero(R.render(pv, pf, above[None], K, H, W, z_near=2.1)[0]) == 0
    one = np.float32([[-1, -1, 2], [3, -1, 2], [-1, 3, 2]])
    eye44 = np.eye(4)[None]
    assert np.count_nonzero(R.render(one, np.int32([[0, 1, 2]]), eye44, K, H, W, z_far=2.0)[0]) > 0
    assert np.count_nonzero(R.render(one, np.int32([[0, 1, 2]]), eye44, K, H, W, z_near=2.0)[0]) == 0


def test_floor_under_and_behind_the_camera():
    # two triangles from 50 m behind the camera to 50 m ahead, 1.2 m below it: vertices at z < 0, no finite screen box
    v = np.float32([[-50, 1.2, -50], [50, 1.2, -50], [50, 1.2, 50], [-50, 1.2, 50]])
    f = np.int32([[0, 1, 2], [0, 2, 3]])
    depth, fid = R.render(v, f, np.eye(4)[None], K, H, W, z_far=100.0)
    _, ry = R.rays(K, H, W)
    with np.errstate(divide="ignore"):
        ref = np.where(ry > 0, 1.2 / ry.astype(np.float64), 0.0)          # z = h / ((i - cy) / fy) below the horizon
    ref = np.where(ref <= 50.0, ref, 0.0)[:, None] * np.ones(W)
    rx, _ = R.rays(K, H, W)
    ref = np.where(np.abs(rx[None].astype(np.float64) * ref) <= 50.0, ref, 0.0)
    assert np.array_equal(depth[0] > 0, ref > 0) and np.count_nonzero(ref) > 3000
    assert np.count_nonzero(depth[0, :H // 2]) == 0                        # nothing above the horizon
    rel = np.abs(depth[0] - ref)[ref > 0] / ref[ref > 0]
    print(f"floor: worst relative error {rel.max():.2e}")
    assert rel.max() < 1e-6


def test_ties_go_to_the_smaller_face_and_degenerate_faces_are_never_hit():
    v, f = O.box_room((2.0, 2.0, 2.0), 0.5)
    w2c = R.look_at([1.0, 0.9, 1.1], [2.0, 1.2, 0.7])[None]
    d0, f0 = R.render(v, f, w2c, K, 48, 48)
    # every face twice, the copies first: the copy (smaller index) wins everywhere, depth unchanged
    d1, f1 = R.render(v, np.concatenate([f, f]), w2c, K, 48, 48)
    assert np.array_equal(d0, d1) and np.array_equal(f0, f1) and f1.max() < len(f)
    # zero-area faces in front of everything: repeated vertices, collinear vertices
    vz = np.concatenate([v, np.float32([[1.2, 1.0, 1.0], [1.4, 1.06, 0.92], [1.6, 1.12, 0.84]])])
    n = len(v)
    bad = np.int32([[0, 0, 5], [7, 7, 7], [n, n + 1, n + 1], [n, n + 1, n + 2]])
    d2, f2 = R.render(vz, np.concatenate([bad, f]), w2c, K, 48, 48)
    assert np.array_equal(d2, d0) and np.array_equal(f2, f0 + len(bad))


def test_check_proj_against_a_plain_pinhole_projection():
    Wp = Hp = 500
    fx = fy = 300.0
    cx, cy = Wp / 2.0 - 0.5, Hp / 2.0 - 0.5
    c2w = np.linalg.inv(R.look_at([0.3, -0.2, 0.5], [2.0, 1.0, 0.7]))

    def point(u, v, z):                            # the world point that projects to (u, v) at depth z (fp64)
        return (c2w @ np.array([(u - cx) / fx * z, (v - cy) / fy * z, z, 1.0]))[:3]

    def plain(p):
        c = np.linalg.inv(c2w) @ np.append(p, 1.0)
        u, v = fx * c[0] / c[2] + cx, fy * c[1] / c[2] + cy
        return bool(c[2] > 0 and 10 < u < Wp - 10 and 10 < v < Hp - 10)

    cases = [(250, 250, 2.0), (100, 400, 0.5), (10.2, 250, 3.0), (9.8, 250, 3.0), (250, 10.2, 3.0), (250, 9.8, 3.0), (489.8, 250, 1.0),
             (490.2, 250, 1.0), (250, 489.8, 1.0), (250, 490.2, 1.0), (250, 250, -2.0), (100, 100, -0.5), (600, 250, 2.0)]
    for u, v, z in cases:
        p = point(u, v, z)[None].astype(np.float32)
        assert R.check_proj(p, Wp, Hp, fx, fy, cx, cy, c2w) == plain(p[0].astype(np.float64)), (u, v, z)
    assert [plain(point(*c)) for c in cases] == [True, True, True, False, True, False, True, False, True, False, False, False, False]
    # any one point inside is enough; none inside: False
    pts = np.stack([point(*c) for c in cases]).astype(np.float32)
    assert R.check_proj(pts, Wp, Hp, fx, fy, cx, cy, c2w)
    assert not R.check_proj(pts[[3, 5, 7, 9, 10, 11, 12]], Wp, Hp, fx, fy, cx, cy, c2w)


def test_sample_views_is_reproducible_prefix_stable_and_rejects():
    v, _ = O.box_room((6.0, 5.0, 3.0), 0.5)
    ext, T = R.get_cam_position(v)
    assert np.allclose(ext, [0.7 * 6, 0.7 * 5, 0.3 * 3]) and np.allclose(T[:3, 3], [3.0, 2.5, 1.9])
    a = R.sample_views(ext, T, 12, seed=5)
    assert np.array_equal(a, R.sample_views(ext, T, 12, seed=5)) and np.array_equal(a[:7], R.sample_views(ext, T, 7, seed=5))
    assert not np.array_equal(a, R.sample_views(ext, T, 12, seed=6))
    pos = (a[:, :3, 3] - T[:3, 3]) / ext
    assert np.abs(pos).max() <= 0.5
    rot = a[:, :3, :3]
    assert np.abs(rot @ rot.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12 and np.all(np.linalg.det(rot) > 0)
    # one unseen point: every accepted view fails check_proj for it; the share of redrawn candidates is the share of the sphere the
    # shrunk field of view covers (13.4 % for the whole image at focal 300 / 500 px; a numpy run of 20 000 candidates redrew 11.8 %)
    unseen = np.float32([[3.0, 2.5, 0.0]])
    stats = {}
    b = R.sample_views(ext, T, 400, unseen=unseen, seed=1, stats=stats)
    for c2w in b:
        assert not R.check_proj(unseen, 500, 500, 300.0, 300.0, 249.5, 249.5, c2w)
    share = stats.get("redrawn", 0) / stats["candidates"]
    print(f"redrawn {stats.get('redrawn', 0)} of {stats['candidates']} candidates ({100 * share:.1f} %)")
    assert 0.0 < share < 0.25
    assert np.array_equal(b[:50], R.sample_views(ext, T, 50, unseen=unseen, seed=1))
    # an unseen cloud all around the box: no view qualifies
    cloud, _ = O.icosphere(3, radius=20.0, center=(3.0, 2.5, 1.9))
    with pytest.raises(RuntimeError):
        R.sample_views(ext, T, 2, unseen=cloud, seed=0, max_tries=20)


def test_depth_l1_and_vertex_visibility_of_the_oracle():
    gt = np.float32([[[2.0, 2.0], [0.0, 3.0]]])
    ours = np.float32([[[2.5, 0.0], [1.0, 3.0]]])
    assert np.array_equal(R.depth_l1(gt, ours), [[3.0, 1.5]])
    # two parallel walls 1 m apart seen head-on from 2 m: the near one is seen, the far one hidden behind it
    nv, nf = O.grid_quad([-1, -1, 2], [2, 0, 0], [0, 2, 0], 8, 8)
    fv, ff = O.grid_quad([-0.5, -0.5, 3], [1, 0, 0], [0, 1, 0], 4, 4)
    v = np.concatenate([nv, fv]).astype(np.float32)
    f = np.concatenate([nf, ff + len(nv)]).astype(np.int32)
    depth, _ = R.render(v, f, np.eye(4)[None], K, H, W)
    seen = R.vertex_visible(v, depth, np.eye(4)[None], K)
    assert seen[:len(nv)].all() and not seen[len(nv):].any()


def test_cli_switches_of_the_2d_metric(tmp_path, monkeypatch):
    from cut3r_slam_amd import eval_recon as ER
    from cut3r_slam_amd import mesh_render as MR
    from cut3r_slam_amd import tsdf as T
    a = ER.parse_args(["rec.ply", "gt.ply"])
    assert (a.eval_2d, a.n_imgs, a.unseen) == (False, 10, None)
    a = ER.parse_args(["rec.ply", "gt.ply", "--eval_2d", "--n-imgs", "7", "--unseen", "u.npy"])
    assert (a.eval_2d, a.n_imgs, a.unseen) == (True, 7, "u.npy")
    with pytest.raises(SystemExit):
        ER.parse_args(["rec.ply", "gt.ply", "--n-imgs", "0"])
    v, f = O.icosphere(0)
    T.write_ply(tmp_path / "m.ply", T.Mesh(v, np.zeros_like(v, dtype=np.uint8), f))
    np.save(tmp_path / "u.npy", v[:2])
    seen = []
    monkeypatch.setattr(ER, "eval_recon", lambda rec, gt, **kw: seen.append(kw) or {"depth l1": 0.5})
    assert ER.main([str(tmp_path / "m.ply"), str(tmp_path / "m.ply")]) == 0
    assert "eval_2d" not in seen[0] and "n_imgs" not in seen[0]                  # without the switch: the call of before
    assert ER.main([str(tmp_path / "m.ply"), str(tmp_path / "m.ply"), "--eval_2d", "--n-imgs", "3", "--unseen", str(tmp_path / "u.npy")]) == 0
    assert seen[1]["eval_2d"] is True and seen[1]["n_imgs"] == 3 and np.array_equal(seen[1]["unseen"], v[:2])
    # a TUM row to a pose: the quaternion of a quarter turn about z
    M = MR.tum_to_c2w([[0.0, 1.0, 2.0, 3.0, 0.0, 0.0, np.sqrt(0.5), np.sqrt(0.5)]])[0]
    assert np.allclose(M, [[0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1]])
    # the axis-aligned camera box of eval_recon equals the oracle's
    rv, rf = O.box_room((6.0, 5.0, 3.0), 0.5)
    ext, tr = ER.get_cam_position(T.Mesh(rv, np.zeros_like(rv, dtype=np.uint8), rf))
    oext, otr = R.get_cam_position(rv)
    assert np.array_equal(ext, oext) and np.array_equal(tr, otr)
    assert np.array_equal(ER.viewmatrix([1.0, 2.0, 0.5], [0, 0, -1.0], [3.0, 2.0, 1.0]), R.viewmatrix([1.0, 2.0, 0.5], [0, 0, -1.0], [3.0, 2.0, 1.0]))
