"""CPU: the TSDF fusion / marching-tetrahedra contract on its numpy restatement (tests/tsdf_oracle.py, the oracle the GPU tests compare
the kernels against bit for bit), the tetrahedron table, and the PLY writer / reader of cut3r_slam_amd.tsdf."""
import numpy as np
import pytest

from cut3r_slam_amd import tsdf as T
from tests import tsdf_oracle as O

VOXEL, RADIUS = 0.02, 0.5
# Calibrated on the oracle (24 views at 256x192, f = 220, camera distance 1.6, radius 25 voxels): with a truncation of 4 voxels the
# vertex radius error is p99 0.30 / max 0.48 voxel, the mesh is closed (every edge in 2 faces, V - E + F = 2) and every face points
# outward.  At the 8-voxel default the projective distances of grazing views bend the zero crossing of so curved a surface: p99 0.86 /
# max 1.29 voxel and small handles (V - E + F = 4); the geometry bounds below are stated for the 4-voxel truncation.
TRUNC_VOXELS = 4.0


@pytest.fixture(scope="module")
def sphere():
    depth, rgb, w2c, K = O.sphere_scene(n_views=24, H=192, W=256, f=220.0, radius=RADIUS)
    origin, dims, trunc = O.sphere_grid(VOXEL, RADIUS, TRUNC_VOXELS)
    vol = O.integrate(O.new_volume(dims), origin, VOXEL, depth, w2c, K, trunc, 5.0, rgb=rgb)
    return vol, origin, dims


def _edges(faces):
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), 1)
    return np.unique(e, axis=0, return_counts=True)


def test_closed_sphere(sphere):
    vol, origin, dims = sphere
    v, c, f = O.extract(vol, origin, VOXEL, 1.0)
    assert v.dtype == np.float32 and c.dtype == np.uint8 and f.dtype == np.int32 and len(f) > 10000
    edges, count = _edges(f)
    assert np.all(count == 2), "every edge in exactly two faces"
    assert len(v) - len(edges) + len(f) == 2, "Euler characteristic of a sphere"
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]).astype(np.float64)
    assert np.all((n * v[f].mean(1)).sum(1) > 0), "every face normal points outward (negative -> positive tsdf)"
    err = np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - RADIUS) / VOXEL
    assert np.percentile(err, 99) <= 0.5 and err.max() <= 1.0, (np.percentile(err, 99), err.max())
    assert np.all(c[:, 0] > 0)            # the surface colour came through (the rendered colours are >= 7 on the sphere)


def test_no_unreferenced_vertices(sphere):
    vol, origin, _ = sphere
    for thr in (1.0, 3.0, 8.0):
        v, _, f = O.extract(vol, origin, VOXEL, thr)
        assert len(v) == 0 or np.array_equal(np.unique(f), np.arange(len(v)))


def test_cells_below_the_weight_threshold_give_no_faces(sphere):
    vol, origin, dims = sphere
    tsdf, weight, color = (a.copy() for a in vol)
    X, Y, Z = dims
    weight[:, :, : X // 2] = 0.5                          # the half x < 0 of the grid falls below the threshold
    v, _, f = O.extract((tsdf, weight, color), origin, VOXEL, 1.0)
    full = O.extract(vol, origin, VOXEL, 1.0)
    assert 0 < len(f) < len(full[2])
    # a face's cell has all 8 corners at weight >= 1: every vertex lies at x >= the first valid voxel column
    x_min = origin[0] + VOXEL * (X // 2)
    assert v[:, 0].min() >= np.float32(x_min) - 1e-6
    # a threshold above every weight leaves nothing
    v2, c2, f2 = O.extract(vol, origin, VOXEL, float(vol[1].max()) + 1)
    assert len(v2) == len(f2) == len(c2) == 0


def test_tetrahedron_table_orientation():
    """all 16 inside/outside cases on a positively oriented tetrahedron: triangles face from negative to positive tsdf, the two triangles
    of a quad share their diagonal in opposite directions, and every sign-changing edge is used"""
    Q = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 1]], np.float64)
    assert np.linalg.det(Q[1:] - Q[0]) > 0
    g = np.random.default_rng(0)
    for case in range(16):
        ins = [(case >> q) & 1 for q in range(4)]
        assert O.NTRI[case] == (0 if sum(ins) in (0, 4) else 2 if sum(ins) == 2 else 1)
        used = set()
        for _ in range(20):
            t = np.where(ins, -g.uniform(0.1, 1, 4), g.uniform(0.1, 1, 4))
            grad = np.linalg.solve(Q[1:] - Q[0], t[1:] - t[0])
            directed = []
            for r in range(O.NTRI[case]):
                tri = O.TRI[case][r]
                P = []
                for e in tri:
                    a, b = O.EDGE[e]
                    assert ins[a] != ins[b]
                    used.add(e)
                    P.append(Q[a] + t[a] / (t[a] - t[b]) * (Q[b] - Q[a]))
                assert np.cross(P[1] - P[0], P[2] - P[0]) @ grad > 0, (case, r)
                directed += [(tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])]
            if O.NTRI[case] == 2:
                shared = [d for d in directed if (d[1], d[0]) in directed]
                assert len(shared) == 2
        assert used == {e for e, (a, b) in enumerate(O.EDGE) if ins[a] != ins[b]}
    # the six tetrahedra tile the cell: chains along the 0 -> 7 diagonal with the parity of their permutation, total volume 1
    vol = 0.0
    for t in range(6):
        corners = np.array([[(c >> a) & 1 for a in range(3)] for c in O.chain(t)], np.float64)
        det = np.linalg.det(corners[1:] - corners[0])
        assert np.sign(det) == O.PARITY[t]
        vol += abs(det) / 6
    assert vol == pytest.approx(1.0)


def test_ply_round_trip(tmp_path):
    g = np.random.default_rng(1)
    mesh = T.Mesh(g.normal(size=(50, 3)).astype(np.float32), g.integers(0, 256, (50, 3), dtype=np.uint8),
                  g.integers(0, 50, (77, 3)).astype(np.int32))
    p = tmp_path / "m.ply"
    T.write_ply(p, mesh)
    back = T.read_ply(p)
    for a, b in zip(mesh, back):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    head = p.read_bytes()[:400].split(b"end_header\n")[0].decode()
    assert "format binary_little_endian 1.0" in head and "property list uchar int vertex_indices" in head
    assert p.stat().st_size == len(head) + len("end_header\n") + 50 * 15 + 77 * 13
    T.write_ply(tmp_path / "e.ply", T.Mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.int32)))
    e = T.read_ply(tmp_path / "e.ply")
    assert e.vertices.shape == (0, 3) and e.faces.shape == (0, 3)


def test_grid_bounds_and_size_limit():
    origin, dims = T.TSDFVolume.grid_for((0, 0, 0), (1.0, 0.5, 0.25), 0.05, pad=0.1)
    assert origin == pytest.approx((-0.1, -0.1, -0.1)) and dims == (25, 15, 10)
    with pytest.raises(ValueError, match="GB"):
        T.TSDFVolume.grid_for((0, 0, 0), (10.0, 10.0, 10.0), 0.006, pad=0.05)


def test_driver_fuses_the_tracked_keyframes_or_the_mapper(monkeypatch):
    """Cut3rSlam.fuse: 'auto' takes the mapper when one with keyframes is attached, else the tracker's keyframes 0..counter-2 (capped by
    tracker.t1 when only the tracked ones count) -- the keyframes of trajectory() and traj_kf.txt"""
    from types import SimpleNamespace
    from cut3r_slam_amd.slam import Cut3rSlam
    calls = []
    monkeypatch.setattr(T, "fuse_keyframes", lambda kf, n, voxel, **k: calls.append(("tracker", n, voxel, k["conf_min"])))
    monkeypatch.setattr(T, "fuse_mapper", lambda m, voxel, **k: calls.append(("mapper", voxel)))
    kf = SimpleNamespace(counter=SimpleNamespace(value=12))
    s = SimpleNamespace(keyframes=kf, tracked_only=False, tracker=SimpleNamespace(t1=7), mapper=None)
    Cut3rSlam.fuse(s, 0.05)
    s.tracked_only = True
    Cut3rSlam.fuse(s, 0.05, conf_min=0.5)
    s.mapper = SimpleNamespace(viewpoints={})
    Cut3rSlam.fuse(s, 0.05)                                  # a mapper without keyframes: the tracker
    s.mapper = SimpleNamespace(viewpoints={0: None})
    Cut3rSlam.fuse(s, 0.04)
    Cut3rSlam.fuse(s, 0.03, source="tracker")
    assert calls == [("tracker", 11, 0.05, None), ("tracker", 7, 0.05, 0.5), ("tracker", 7, 0.05, None), ("mapper", 0.04),
                     ("tracker", 7, 0.03, None)]
    s.mapper = None
    with pytest.raises(ValueError):
        Cut3rSlam.fuse(s, 0.05, source="mapper")
    with pytest.raises(ValueError):
        Cut3rSlam.fuse(s, 0.05, source="open3d")
