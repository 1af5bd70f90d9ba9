"""CPU: cut3r_slam_amd/views.py -- the pose and intrinsics layouts every consumer of posed depth maps accepts, the TUM formula, the three
inverses (each against its own numpy statement, never against one another) and the rule that picks the run's keyframes -- and what the
call sites in front of the kernels do with a lone [3,4] / [4,4] pose, which differs per site and is pinned here as it was before the
module existed."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cut3r_slam_amd import depth_consistency as DC  # noqa: E402
from cut3r_slam_amd import eval_dense as ED  # noqa: E402
from cut3r_slam_amd import mesh_render as MR  # noqa: E402
from cut3r_slam_amd import ops  # noqa: E402
from cut3r_slam_amd import tsdf as T  # noqa: E402
from cut3r_slam_amd import views as V  # noqa: E402
from cut3r_slam_amd.slam import Cut3rSlam  # noqa: E402

CPU = torch.device("cpu")
K4 = [50.0, 48.0, 15.5, 11.5]


def _poses(n, seed=0):
    """fp64 [n,4,4] with a last row that is NOT 0 0 0 1: it must be dropped unread"""
    return np.random.default_rng(seed).normal(size=(n, 4, 4))


def _as(x, kind):
    return torch.from_numpy(np.ascontiguousarray(x)) if kind == "tensor" else x


# ------------------------------------------------------------------------------------------------------------- layouts
@pytest.mark.parametrize("kind", ["array", "tensor"])
@pytest.mark.parametrize("n", [1, 3, 4])
def test_pose_rows_takes_the_four_layouts(n, kind):
    P = _poses(n)
    want = P[:, :3, :]                                                  # the slicing, written out
    layouts = {"[n,12]": P[:, :3].reshape(n, 12), "[n,16]": P.reshape(n, 16), "[n,3,4]": P[:, :3], "[n,4,4]": P}
    for name, x in layouts.items():
        got = V.pose_rows(_as(x, kind))
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (n, 3, 4) and np.array_equal(got, want), name
        got = V.pose_rows(_as(x, kind), torch.float32)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and torch.equal(got, torch.from_numpy(want).float()), name
        got = V.pose_rows(_as(x.astype(np.float32), kind), np.float32)
        assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32)), name
        mats = V.pose_matrices(_as(x, kind))
        assert mats.dtype == np.float64 and np.array_equal(mats[:, :3], want) and np.array_equal(mats[:, 3], [[0, 0, 0, 1]] * n), name


@pytest.mark.parametrize("kind", ["array", "tensor"])
def test_pose_rows_refuses_every_other_shape(kind):
    g = np.random.default_rng(1)
    for shape in [(12,), (16,), (3, 4), (4, 4), (3, 11), (3, 13), (4, 15), (3, 7), (3, 3, 3), (3, 4, 3), (3, 2, 4), (3, 5, 4), (2, 3, 3, 4),
                  (1, 1, 12), (3, 3, 12), ()]:
        with pytest.raises(ValueError, match=r"poses: \[n,12\], \[n,16\], \[n,3,4\] or \[n,4,4\]"):
            V.pose_rows(_as(g.normal(size=shape), kind))
        with pytest.raises(ValueError, match=r"poses: \[n,12\], \[n,16\], \[n,3,4\] or \[n,4,4\]"):
            V.pose_rows(_as(g.normal(size=shape), kind), torch.float32)
    # single=True: a lone [3,4] / [4,4] is one pose, and nothing else changes
    P = _poses(1)[0]
    for x in (P[:3], P):
        assert np.array_equal(V.pose_rows(_as(x, kind), single=True), P[None, :3])
    for shape in [(12,), (3, 3), (4, 3), (2, 4)]:
        with pytest.raises(ValueError, match="poses:"):
            V.pose_rows(_as(g.normal(size=shape), kind), single=True)
    P3 = _poses(3)
    assert np.array_equal(V.pose_rows(_as(P3, kind), single=True), P3[:, :3])


@pytest.mark.parametrize("kind", ["array", "tensor"])
@pytest.mark.parametrize("n", [1, 3, 4])
def test_intrinsics_broadcasts_one_row_and_refuses_a_count_mismatch(n, kind):
    g = np.random.default_rng(2)
    one = np.array(K4)
    rows = g.uniform(1, 100, (n, 4))
    for x, want in ((one, np.stack([one] * n)), (one[None], np.stack([one] * n)), (rows, rows)):
        got = V.intrinsics(_as(x, kind), n)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (n, 4) and np.array_equal(got, want)
        got[0, 0] = -1.0                                                # a copy: writable, and the input is untouched
        assert x.reshape(-1)[0] != -1.0
        got = V.intrinsics(_as(x, kind), n, torch.float32)
        assert got.dtype == torch.float32 and got.is_contiguous() and torch.equal(got, torch.from_numpy(want).float())
    assert np.array_equal(V.intrinsics(K4, n), np.stack([one] * n))   # a plain list
    bad = [(n + 1, 4), (2 * n + 1, 4), (5,), (3,), (n, 3), (n, 5), (2, 2), (4 * n + 4,), (1, 1, 4), (n, 1, 4), ()]
    for shape in bad:
        with pytest.raises(ValueError, match="intrinsics:"):
            V.intrinsics(_as(g.uniform(1, 2, shape), kind), n)
        with pytest.raises(ValueError, match="intrinsics:"):
            V.intrinsics(_as(g.uniform(1, 2, shape), kind), n, torch.float32)


# ----------------------------------------------------------------------------- a lone [3,4] / [4,4] pose at every call site
def _volume(monkeypatch, seen):
    def cast(tsdf, weight, color, origin, voxel, c2w, K, H, W, *a, **kw):
        seen.append(("cast", c2w.clone(), K.clone()))
        B = c2w.shape[0]
        return torch.zeros(B, H, W), torch.zeros(B, H, W, 3), torch.zeros(B, 3, H, W, dtype=torch.uint8), None
    fuse = lambda tsdf, weight, color, origin, voxel, d, w2c, K, *a, **kw: seen.append(("fuse", w2c.clone(), K.clone()))
    monkeypatch.setattr(ops, "tsdf_integrate", fuse)
    monkeypatch.setattr(ops, "tsdf_ray_cast", cast)
    return T.TSDFVolume((0, 0, 0), 0.1, (4, 4, 4), device="cpu")


@pytest.mark.parametrize("kind", ["array", "tensor"])
@pytest.mark.parametrize("rows", [3, 4])
def test_a_single_pose_is_taken_by_the_tsdf_sites_and_refused_by_the_others(rows, kind, monkeypatch, tmp_path):
    P = _poses(1, seed=3)[0]
    P[:3, :3] += 2 * np.eye(3)                                          # invertible
    x = _as(P[:rows], kind)
    row12 = torch.from_numpy(P[:3].reshape(1, 12)).float()
    Kn = torch.tensor([K4])
    # refused: the rasteriser's views, the cloud, the consistency rows, the evaluation's matrices, the culling
    with pytest.raises(ValueError):
        ops._views(x, K4, CPU)
    monkeypatch.setattr(ops, "_cuda", lambda *a: None)
    for B in (1, rows):
        with pytest.raises(ValueError):
            ops.depth_cloud(torch.ones(B, 6, 8), x, K4, 5.0)
    with pytest.raises(ValueError):
        DC.relative_rows(x, [0], [[-1]])
    with pytest.raises(ValueError):
        ED.pose_matrices(x)
    monkeypatch.setattr(MR, "_gpu_mesh", lambda m: (torch.zeros(5, 3), torch.zeros(2, 3, dtype=torch.int32)))
    monkeypatch.setattr(MR, "as_mesh", lambda m: m)
    raster = []
    monkeypatch.setattr(ops, "mesh_raster", lambda v, f, w, k, H, W, **kw: raster.append(ops._views(w, k, CPU)[0]) or torch.zeros(len(w), H, W))
    with pytest.raises(ValueError):
        MR.visible_vertices(None, P[:rows], K4, 6, 8)
    # taken as one pose: a rigid transform of the metrics, and every TSDF site
    assert torch.equal(ops._transform34(x, CPU), row12[0])
    seen = []
    vol = _volume(monkeypatch, seen)
    vol.integrate(torch.ones(1, 6, 8), x, K4)
    vol.ray_cast(x, K4, 6, 8)
    want_c2w = torch.from_numpy(T.c2w_rows(row12.numpy()))
    assert [s[0] for s in seen] == ["fuse", "cast"] and torch.equal(seen[0][1], row12) and torch.equal(seen[1][1], want_c2w)
    assert torch.equal(seen[0][2], Kn) and torch.equal(seen[1][2], Kn)
    with pytest.raises(ValueError):                                     # ... but one pose is not three
        vol.integrate(torch.ones(3, 6, 8), x, K4)
    normal = torch.nn.functional.normalize(torch.from_numpy(np.random.default_rng(4).normal(size=(1, 2, 2, 3))).float(), dim=-1)
    n_cam = torch.einsum("bij,bhwj->bhwi", row12.reshape(1, 3, 4)[:, :, :3], normal)
    assert torch.equal(T.shade(normal, x), torch.floor((n_cam * 0.5 + 0.5).clamp(0, 1) * 255 + 0.5).to(torch.uint8))
    with pytest.raises(ValueError):
        T.shade(normal.expand(3, -1, -1, -1), x)
    calls = []

    def ray_cast(w2c, K, H, W, **kw):
        calls.append((w2c.clone(), K.clone()))
        return T.RayCast(torch.zeros(1, H, W), torch.zeros(1, H, W, 3), torch.zeros(1, 3, H, W, dtype=torch.uint8))
    idx, _ = T.write_previews(SimpleNamespace(ray_cast=ray_cast), x, K4, 6, 8, tmp_path)
    assert idx == [0] and torch.equal(calls[0][0], row12) and torch.equal(calls[0][1], Kn)
    if rows == 4:                                                       # a camera-to-world 4x4 for the rasteriser is inverted as one matrix
        MR.render_depth(None, P, K4, 6, 8)
        assert torch.equal(raster[-1], torch.from_numpy(np.linalg.inv(P)[:3].reshape(1, 12)).float())


def test_the_tsdf_sites_take_every_layout_to_the_same_rows(monkeypatch, tmp_path):
    P = _poses(3, seed=5)
    P[:, :3, :3] += 2 * np.eye(3)
    P[:, 3] = [0, 0, 0, 1]
    want = torch.from_numpy(P[:, :3].reshape(3, 12)).float()
    Ks = np.random.default_rng(6).uniform(20, 60, (3, 4))
    seen = []
    vol = _volume(monkeypatch, seen)
    for x in (P[:, :3].reshape(3, 12), P.reshape(3, 16), P[:, :3], P, torch.from_numpy(P).float(), torch.from_numpy(P[:, :3].reshape(3, 12))):
        for k, want_k in ((K4, torch.tensor([K4] * 3)), ([K4], torch.tensor([K4] * 3)), (Ks, torch.from_numpy(Ks).float())):
            del seen[:]
            vol.integrate(torch.ones(3, 6, 8), x, k)
            vol.ray_cast(x, k, 6, 8)
            assert torch.equal(seen[0][1], want) and torch.equal(seen[1][1], torch.from_numpy(T.c2w_rows(want.numpy())))
            assert torch.equal(seen[0][2], want_k) and torch.equal(seen[1][2], want_k) and seen[0][2].is_contiguous()
            w, kk, B = ops._views(x, k, CPU)
            assert B == 3 and torch.equal(w, want) and torch.equal(kk, want_k)
    for bad_k in (Ks[:2], np.ones(5), np.ones((3, 3))):
        with pytest.raises(ValueError):
            vol.ray_cast(P, bad_k, 6, 8)
        with pytest.raises(ValueError):
            ops._views(P, bad_k, CPU)
    with pytest.raises(ValueError):
        vol.ray_cast(np.zeros((0, 12)), K4, 6, 8)
    with pytest.raises(ValueError):
        ops._views(np.zeros((0, 12)), K4, CPU)


# ------------------------------------------------------------------------------------------------------------- TUM rows
def _tum_written_out(t, q):
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    out = np.tile(np.eye(4), (len(t), 1, 1))
    out[:, :3, :3], out[:, :3, 3] = R, t
    return out


@pytest.mark.parametrize("unit", [True, False])
def test_tum_matrices_is_the_formula_bit_for_bit(unit):
    g = np.random.default_rng(7)
    t, q = g.normal(size=(5, 3)), g.normal(size=(5, 4))
    if unit:
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    else:
        q *= g.uniform(0.1, 9.0, (5, 1))
    want = _tum_written_out(t, q)
    rows7 = np.concatenate([t, q], 1)
    rows8 = np.concatenate([g.uniform(0, 100, (5, 1)), rows7], 1)
    for rows in (rows7, rows8, torch.from_numpy(rows7), torch.from_numpy(rows8)):
        for fn in (V.tum_matrices, V.pose_matrices, ED.pose_matrices):
            got = fn(rows)
            assert got.dtype == np.float64 and np.array_equal(got.view(np.int64), want.view(np.int64))
    assert np.array_equal(MR.tum_to_c2w(rows8).view(np.int64), want.view(np.int64))
    R = want[:, :3, :3]
    assert np.allclose(R @ R.transpose(0, 2, 1), np.eye(3), atol=1e-12) and np.allclose(np.linalg.det(R), 1.0)
    for shape in [(5, 6), (5, 9), (8,), (7,), (2, 5, 8)]:
        with pytest.raises(ValueError, match="TUM rows"):
            V.tum_matrices(np.ones(shape))


# ------------------------------------------------------------------------------------------------------------- inverses
def test_each_inverse_is_its_own_numpy_statement():
    g = np.random.default_rng(8)
    q = g.normal(size=(6, 4))
    M = _tum_written_out(g.normal(size=(6, 3)), q)                      # rigid up to rounding
    bits = lambda a: np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)
    # 4x4: np.linalg.inv of the stack, one [4,4] counting as a stack of one
    assert np.array_equal(bits(V.inverse44(M)), bits(np.linalg.inv(M)))
    assert np.array_equal(bits(V.inverse44(M[0])), bits(np.linalg.inv(M[:1])))
    # affine 3x4: the 3x3 inverse and -Ri t in fp64, rounded once to fp32 -- tsdf.c2w_rows
    rows = M[:, :3].reshape(6, 12).astype(np.float32)
    w = rows.astype(np.float64).reshape(-1, 3, 4)
    Ri = np.linalg.inv(w[:, :, :3])
    want = np.concatenate([Ri, -(Ri @ w[:, :, 3:])], 2).reshape(-1, 12).astype(np.float32)
    got = V.inverse_affine(rows)
    assert got.dtype == np.float32 and got.flags.c_contiguous and np.array_equal(bits(got), bits(want))
    assert T.c2w_rows is V.inverse_affine
    sheared = w + g.normal(size=w.shape) * 0.3                          # any invertible map, not only a rigid one
    back = V.inverse_affine(V.inverse_affine(sheared.reshape(6, 12))).reshape(6, 3, 4)
    assert np.allclose(back, sheared, atol=1e-5)
    # rigid: the transpose and -R^T t, nothing inverted
    W = np.ascontiguousarray(M[:, :3])
    Rt, tt = V.inverse_rigid(W)
    assert np.array_equal(bits(Rt), bits(W[:, :, :3].transpose(0, 2, 1)))
    assert np.array_equal(bits(tt), bits(-np.einsum("nij,nj->ni", W[:, :, :3].transpose(0, 2, 1), W[:, :, 3])))
    # relative_rows is built on it: view 0 into view 1 and back
    fwd, bwd = DC.relative_rows(W, [0], [[1]])
    want_R = np.einsum("ij,jk->ik", W[1, :, :3], Rt[0])
    want_t = np.einsum("ij,j->i", W[1, :, :3], tt[0]) + W[1, :, 3]
    assert np.array_equal(bits(fwd[0, 0]), bits(np.concatenate([want_R, want_t[:, None]], 1).reshape(12)))
    assert bwd.shape == (1, 1, 12)


# ------------------------------------------------------------------------------------------------------------- the run's views
def _run(counter, tracked_only=False, t1=7, mapper=None):
    kf = SimpleNamespace(counter=SimpleNamespace(value=counter), tstamp=torch.arange(32.0), pose=torch.zeros(32, 7))
    return SimpleNamespace(keyframes=kf, tracked_only=tracked_only, tracker=SimpleNamespace(t1=t1), mapper=mapper)


def _mapper(n):
    return SimpleNamespace(viewpoints={k: SimpleNamespace(tstamp=k) for k in range(n)})


RUNS = [  # (run, source, expected)
    (lambda: _run(12), "auto", ("tracker", 11)),                                       # no mapper
    (lambda: _run(12), "tracker", ("tracker", 11)),
    (lambda: _run(12), "mapper", ValueError),
    (lambda: _run(12, mapper=_mapper(0)), "auto", ("tracker", 11)),                   # a mapper without keyframes
    (lambda: _run(12, mapper=_mapper(0)), "mapper", ValueError),
    (lambda: _run(12, mapper=_mapper(3)), "auto", ("mapper", 3)),                     # a mapper with keyframes
    (lambda: _run(12, mapper=_mapper(3)), "mapper", ("mapper", 3)),
    (lambda: _run(12, mapper=_mapper(3)), "tracker", ("tracker", 11)),
    (lambda: _run(12, tracked_only=True, t1=7), "auto", ("tracker", 7)),              # t1 below the counter
    (lambda: _run(12, tracked_only=True, t1=20), "auto", ("tracker", 11)),            # t1 above it
    (lambda: _run(12, tracked_only=True, t1=7, mapper=_mapper(3)), "tracker", ("tracker", 7)),
    (lambda: _run(1), "auto", ("tracker", 0)),                                         # counter at 1: no tracked keyframe yet
    (lambda: _run(1, tracked_only=True, t1=0), "tracker", ("tracker", 0)),
    (lambda: _run(12), "open3d", ValueError),                                          # a bad source string
    (lambda: _run(12, mapper=_mapper(3)), "fused", ValueError),                        # "fused" is eval_dense's, not a keyframe source
]


@pytest.mark.parametrize("make, source, want", RUNS)
def test_run_views_and_its_three_users_agree(make, source, want, monkeypatch):
    seen = []
    monkeypatch.setattr(T, "fuse_keyframes", lambda kf, n, voxel, **k: seen.append(("tracker", n)))
    monkeypatch.setattr(T, "fuse_mapper", lambda m, voxel, **k: seen.append(("mapper", len(m.viewpoints))))
    monkeypatch.setattr(ED, "from_keyframes", lambda kf, n, stamps=None, consistency=None: seen.append(("tracker", n)))
    monkeypatch.setattr(ED, "from_mapper", lambda m, stamps=None, consistency=None: seen.append(("mapper", len(m.viewpoints))))
    s = make()
    if want is ValueError:
        texts = []
        for call in (lambda: V.run_views(s, source), lambda: Cut3rSlam.fuse(s, 0.05, source=source)) + \
                (() if source == "fused" else (lambda: ED.from_slam(s, source),)):
            with pytest.raises(ValueError) as e:
                call()
            texts.append(str(e.value))
        assert len(set(texts)) == 1 and not seen
        return
    assert V.run_views(s, source) == want
    Cut3rSlam.fuse(s, 0.05, source=source)
    ED.from_slam(s, source)
    assert seen == [want, want]
    ts, poses = Cut3rSlam.trajectory(s)                                 # the trajectory is the tracker's keyframes, whatever the source
    n = V.run_views(s, "tracker")[1]
    assert len(ts) == len(poses) == n and (want[0] == "mapper" or want[1] == n)
