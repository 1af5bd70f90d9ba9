"""CPU: the multi-view depth-consistency rule on its numpy restatement (tests/consistency_oracle.py) -- a closed form, the three single-pixel
cases, the box room with injected floaters -- and the host code of cut3r_slam_amd/depth_consistency.py (tables, rigid rows, chunking,
masking, the opt-in keywords), with ops.depth_consistency replaced by the oracle."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from cut3r_slam_amd import depth_consistency as DC
from cut3r_slam_amd import ops
from tests import consistency_oracle as O

DEPTH_MAX = 10.0


def _oracle_op(calls=None):
    def op(depth, K, ref, src, fwd, bwd, depth_max, pix=1.0, rel=0.01, z_min=1e-3, average=False):
        if calls is not None:
            calls.append((np.asarray(ref).tolist(), np.asarray(src).shape))
        s, v, a = O.consistency(depth.numpy(), K.numpy(), ref, src, fwd, bwd, depth_max, pix, rel, z_min)
        return torch.from_numpy(s), torch.from_numpy(v), torch.from_numpy(a) if average else None
    return op


@pytest.fixture
def oracle_op(monkeypatch):
    calls = []
    monkeypatch.setattr(ops, "depth_consistency", _oracle_op(calls))
    return calls


def _run(depth, w2c, K, window=1, **kw):
    src = DC.neighbour_table(len(depth), window)
    ref = np.arange(len(depth))
    fwd, bwd = DC.relative_rows(w2c, ref, src)
    return O.consistency(depth, K, ref, src, fwd, bwd, DEPTH_MAX, **kw)


# ------------------------------------------------------------------------------------------------------------------- the rule
def test_closed_form_plane_pair():
    """plane z = 2, K = (64, 64, 9.5, 2.5), baseline 0.25: every number is exact and the shift is 8 px, so view 0 is supported exactly on
    u >= 8 (the last row included: vs = H - 1 exactly) and view 1 exactly on u <= 11; nothing is a violation"""
    depth, w2c, K = O.plane_pair()
    s, v, a = _run(depth, w2c, K)
    u = np.broadcast_to(np.arange(20), (6, 20))
    assert np.array_equal(s[0], (u >= 8).astype(np.uint8)) and np.array_equal(s[1], (u <= 11).astype(np.uint8))
    assert not v.any()
    assert np.array_equal(a, depth)                                # (2 + 2) / 2 and 2 / 1


def test_a_pixel_pulled_forward_is_a_violation():
    depth, w2c, K = O.plane_pair()
    depth[0, 2, 17] = np.float32(0.6 * 2.0)                        # us = 17 - 40 / 3: inside the source, which sees the wall at 2 behind it
    s, v, _ = _run(depth, w2c, K)
    assert v[0, 2, 17] == 1 and s[0, 2, 17] == 0
    v[0, 2, 17] = 0
    assert not v.any()


def test_a_pixel_behind_the_sources_surface_is_neither():
    depth, w2c, K = O.plane_pair()
    depth[0, 2, 12] = 3.0                                          # us = 12 - 16 / 3: inside the source, whose wall at 2 hides the point
    s, v, _ = _run(depth, w2c, K)
    assert v[0, 2, 12] == 0 and s[0, 2, 12] == 0 and not v.any()
    assert s[0, 2, 11] == 1 and s[0, 2, 13] == 1


def test_taps_that_straddle_a_discontinuity_are_no_violation():
    """the pulled pixel (17 -> us = 17 - 40 / 3 = 3.67) is a violation against a flat source; with the source's columns <= 3 at depth 1
    (nearer than the point's 1.2) two of its four taps are in front of the point, and the verdict is withheld"""
    depth, w2c, K = O.plane_pair()
    depth[0, 2, 17] = np.float32(1.2)
    s, v, _ = _run(depth, w2c, K)
    assert v[0, 2, 17] == 1 and s[0, 2, 17] == 0
    depth[1, :, :4] = 1.0
    s, v, _ = _run(depth, w2c, K)
    assert v[0, 2, 17] == 0 and s[0, 2, 17] == 0
    assert not v[0].any()


@pytest.fixture(scope="module")
def room():
    depth, w2c, K = O.box_room()
    noisy, mask = O.inject_floaters(depth, 0.03, 0)
    return depth, noisy, mask, w2c, K


def test_box_room_floaters_are_rejected_and_the_clean_scene_kept(room):
    """7 views of the box room at 48 x 64, window 2, 3 % floaters at 0.4 .. 0.8 of the depth; rel 0.01, pix 1, min_support 2,
    max_violation 0.  Measured with this oracle: 0.786 of the clean pixels kept (0.914 on the three middle views), every floater
    rejected, 92.7 % of them by a violation.  The losses are border pixels, the end views' missing neighbours and pixels whose source taps
    include a floater."""
    depth, noisy, mask, w2c, K = room
    s0, v0, _ = _run(depth, w2c, K, window=2)
    assert not v0.any()                                            # the clean scene has no violation at all
    s, v, _ = _run(noisy, w2c, K, window=2)
    keep = (s >= 2) & (v <= 0)
    assert mask.sum() > 300
    assert not keep[mask].any()                                    # every injected pixel is rejected
    assert not v[~mask].any()                                      # no clean pixel has a violation
    kept = keep[~mask].mean()
    print(f"clean kept {kept:.3f}, middle views {keep[2:5][~mask[2:5]].mean():.3f}, floaters by violation {(v[mask] > 0).mean():.3f}")
    assert kept >= 0.75                                            # measured 0.786


# -------------------------------------------------------------------------------------------------------------- host functions
def test_neighbour_table_at_the_ends_and_for_few_views():
    assert DC.neighbour_table(5, 2).tolist() == [[1, 2, -1, -1], [0, 2, 3, -1], [0, 1, 3, 4], [1, 2, 4, -1], [2, 3, -1, -1]]
    assert DC.neighbour_table(2, 2).tolist() == [[1, -1, -1, -1], [0, -1, -1, -1]]
    assert DC.neighbour_table(1, 3).tolist() == [[-1] * 6]
    t = DC.neighbour_table(19, 8)
    assert t.dtype == np.int32 and t.shape == (19, 16) and t[9].tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 15, 16, 17]


def _compose(a, b):
    A, B = np.eye(4), np.eye(4)
    A[:3], B[:3] = a.reshape(3, 4), b.reshape(3, 4)
    return (A @ B)[:3].reshape(12)


def test_relative_rows_compose_to_the_identity_and_carry_points():
    _, w2c, _ = O.box_room()
    ref = np.array([1, 5, 3])
    src = np.array([[0, 2, -1], [6, 4, 3], [1, -1, -1]])
    fwd, bwd = DC.relative_rows(w2c, ref, src)
    assert fwd.dtype == np.float64 and fwd.shape == (3, 3, 12)
    eye = np.eye(4)[:3].reshape(12)
    p = np.array([0.3, -0.2, 1.1, 1.0])
    for r in range(3):
        for k in range(3):
            if src[r, k] < 0:
                assert not fwd[r, k].any() and not bwd[r, k].any()
                continue
            assert np.abs(_compose(fwd[r, k], bwd[r, k]) - eye).max() < 1e-15
            cam_r = w2c[ref[r]].reshape(3, 4) @ p
            cam_s = w2c[src[r, k]].reshape(3, 4) @ p
            assert np.abs(fwd[r, k].reshape(3, 4) @ np.append(cam_r, 1.0) - cam_s).max() < 1e-14
    assert np.array_equal(DC.relative_rows(torch.from_numpy(w2c).reshape(-1, 3, 4), ref, src)[0], fwd)


def test_refusals_of_the_host_code(oracle_op):
    depth, w2c, K = O.box_room()
    with pytest.raises(ValueError, match="own source"):
        DC.relative_rows(w2c, [2], [[1, 2]])
    for bad in ([[7]], [[-2]]):
        with pytest.raises(ValueError, match="outside"):
            DC.relative_rows(w2c, [0], bad)
    with pytest.raises(ValueError, match="outside"):
        DC.relative_rows(w2c, [7], [[0]])
    with pytest.raises(ValueError, match="sources"):
        DC.relative_rows(w2c, [0], [list(range(1, 7)) * 3][:1])           # S = 18
    with pytest.raises(ValueError, match="sources"):
        DC.consistency(torch.from_numpy(depth), w2c, K, window=9)
    with pytest.raises(ValueError):
        DC.consistency(torch.from_numpy(depth[0]), w2c, K)
    assert not oracle_op


def test_ops_wrapper_mirrors_the_c_refusals():
    """every one of these is refused on the host before the library is touched (the tensors are not even on a GPU)"""
    with pytest.raises(ValueError):
        ops.depth_consistency(torch.zeros(2, 4, 4), torch.ones(2, 4), [0], [[1]], np.zeros((1, 1, 12)), np.zeros((1, 1, 12)), 5.0)


def test_consistency_chunks_the_views(oracle_op, room):
    depth, noisy, mask, w2c, K = room
    whole = DC.consistency(torch.from_numpy(noisy), w2c, K, window=2, depth_max=DEPTH_MAX, average=True)
    assert [c[0] for c in oracle_op] == [list(range(7))] and oracle_op[0][1] == (7, 4)
    del oracle_op[:]
    parts = DC.consistency(torch.from_numpy(noisy), w2c, K[0], window=2, depth_max=DEPTH_MAX, average=True, chunk=3)
    assert [c[0] for c in oracle_op] == [[0, 1, 2], [3, 4, 5], [6]]
    assert len(whole) == len(parts) == 3 and all(torch.equal(a, b) for a, b in zip(whole, parts))
    assert len(DC.consistency(torch.from_numpy(noisy), w2c, K, depth_max=DEPTH_MAX)) == 2
    # an explicit source table replaces the window
    s, v = DC.consistency(torch.from_numpy(noisy), w2c, K, src=DC.neighbour_table(7, 1), depth_max=DEPTH_MAX)
    assert np.array_equal(s.numpy(), _run(noisy, w2c, K, window=1)[0])


def test_filter_depths_zeroes_exactly_the_rejected_pixels(oracle_op, room):
    depth, noisy, mask, w2c, K = room
    noisy = noisy.copy()
    noisy[3, 5, 5:9] = [np.nan, np.inf, -1.0, 11.0]                 # invalid pixels are never kept, whatever min_support says
    d = torch.from_numpy(noisy)
    out, keep = DC.filter_depths(d, w2c, K, depth_max=DEPTH_MAX)
    s, v, a = _run(noisy, w2c, K, window=2)
    want = (s >= 2) & (v == 0)
    assert np.array_equal(keep.numpy(), want) and keep.dtype == torch.bool
    assert np.array_equal(out.numpy()[want].view(np.int32), noisy[want].view(np.int32)) and not out.numpy()[~want].any()
    assert not keep.numpy()[mask].any()
    out0, keep0 = DC.filter_depths(d, w2c, K, min_support=0, max_violation=4, depth_max=DEPTH_MAX)
    assert np.array_equal(keep0.numpy(), O.valid(noisy, DEPTH_MAX)) and not keep0[3, 5, 5:9].any() and not out0[3, 5, 5:9].any()
    # average=True: depth_avg on keep, 0 elsewhere
    outa, keepa = DC.filter_depths(d, w2c, K, depth_max=DEPTH_MAX, average=True)
    assert np.array_equal(keepa.numpy(), want)
    assert np.array_equal(outa.numpy()[want].view(np.int32), a[want].view(np.int32)) and not outa.numpy()[~want].any()
    assert (outa.numpy()[want] != noisy[want]).any()
    # the options tuple is the same call
    outb, keepb = DC.apply(d, w2c, K, DC.ConsistencyOptions(average=True), DEPTH_MAX)
    assert torch.equal(outb, outa) and torch.equal(keepb, keepa)
    outc, _ = DC.apply(d, w2c, K, {"window": 1, "min_support": 1}, DEPTH_MAX)
    assert np.array_equal(outc.numpy() > 0, (_run(noisy, w2c, K, window=1)[0] >= 1) & (_run(noisy, w2c, K, window=1)[1] == 0))


def test_depth_max_is_compared_as_the_kernel_compares_it(oracle_op):
    """0.1 is no fp32: float32(0.1) > 0.1, so a depth of float32(0.1) is beyond depth_max = 0.1 in the kernel's fp64 comparison"""
    depth, w2c, K = O.plane_pair()
    depth[:] = np.float32(0.1)
    depth[0, 0, 0] = np.nextafter(np.float32(0.1), np.float32(0))
    _, keep = DC.filter_depths(torch.from_numpy(depth), w2c, K, min_support=0, depth_max=0.1)
    assert int(keep.sum()) == 1 and bool(keep[0, 0, 0])


# -------------------------------------------------------------------------------------------------------------- opt-in wiring
def test_fuse_filters_the_stack_before_bounds_and_integration(oracle_op, room, monkeypatch):
    from cut3r_slam_amd import tsdf as T
    depth, noisy, mask, w2c, K = room
    seen = []
    monkeypatch.setattr(ops, "tsdf_integrate", lambda tsdf, weight, color, origin, voxel, d, *a, **k: seen.append(d.clone()))
    n = 7
    kf = SimpleNamespace(device=torch.device("cpu"), depth=torch.from_numpy(noisy), image=torch.zeros(n, 3, 48, 64, dtype=torch.uint8),
                         w2c=torch.from_numpy(w2c).float(), intrinsic=torch.from_numpy(K), conf_ds=None, downsample_ratio=1)
    opts = DC.ConsistencyOptions()
    vol = T.fuse_keyframes(kf, n, 0.1, trunc_voxels=4.0, depth_max=DEPTH_MAX, consistency=opts)
    want, keep = DC.apply(kf.depth, kf.w2c, kf.intrinsic, opts, DEPTH_MAX)
    assert len(seen) == 1 and torch.equal(seen[0], want) and not seen[0][torch.from_numpy(mask)].any()
    assert int(vol.consistency[0]) == int(keep.sum()) and int(vol.consistency[1]) == 7 * 48 * 64
    plain = T.fuse_keyframes(kf, n, 0.1, trunc_voxels=4.0, depth_max=DEPTH_MAX)
    assert torch.equal(seen[1], kf.depth) and plain.consistency is None
    # the bounds are those of the filtered stack
    lo, hi = T.depth_bounds(want, kf.w2c, kf.intrinsic, DEPTH_MAX)
    assert vol.dims == T.TSDFVolume.grid_for(lo, hi, 0.1, 0.4)[1] and vol.dims != plain.dims


def test_the_driver_and_the_dense_sources_pass_consistency_through(oracle_op, room, monkeypatch):
    from cut3r_slam_amd import eval_dense as ED
    from cut3r_slam_amd import tsdf as T
    from cut3r_slam_amd.slam import Cut3rSlam
    depth, noisy, mask, w2c, K = room
    seen = []
    monkeypatch.setattr(T, "fuse_keyframes", lambda kf, n, voxel, **k: seen.append(k) or SimpleNamespace(extract_mesh=lambda w: "mesh"))
    s = SimpleNamespace(keyframes=SimpleNamespace(counter=SimpleNamespace(value=8)), tracked_only=False, tracker=None, mapper=None)
    s.fuse = lambda *a, **k: Cut3rSlam.fuse(s, *a, **k)
    opts = DC.ConsistencyOptions(window=1)
    Cut3rSlam.fuse(s, 0.05)
    Cut3rSlam.fuse(s, 0.05, consistency=opts)
    assert Cut3rSlam.reconstruct(s, 0.05, consistency=opts) == "mesh"
    assert "consistency" not in seen[0] and seen[1]["consistency"] is opts and seen[2]["consistency"] is opts
    # the dense evaluation's keyframe source: poses are camera->world (t, q xyzw)
    c, Rm = O.room_cameras()
    pose = np.zeros((7, 7))
    pose[:, :3] = c
    for i in range(7):
        w = 0.5 * np.sqrt(1 + np.trace(Rm[i]))
        pose[i, 3:] = [(Rm[i][2, 1] - Rm[i][1, 2]) / (4 * w), (Rm[i][0, 2] - Rm[i][2, 0]) / (4 * w), (Rm[i][1, 0] - Rm[i][0, 1]) / (4 * w), w]
    kf = SimpleNamespace(depth=torch.from_numpy(noisy), pose=torch.from_numpy(pose), intrinsic=torch.from_numpy(K),
                         tstamp=torch.arange(7.0), image=torch.zeros(7, 3, 48, 64, dtype=torch.uint8))
    monkeypatch.setattr(ED, "_device", lambda: torch.device("cpu"))
    plain = ED.from_keyframes(kf, 7)
    assert plain.depth is not None and torch.equal(plain.depth, kf.depth)
    got = ED.from_keyframes(kf, 7, consistency=DC.ConsistencyOptions())
    assert np.array_equal(got.c2w, plain.c2w) and np.array_equal(got.stamps, plain.stamps) and torch.equal(got.rgb, plain.rgb)
    s_, v_, _ = O.consistency(noisy, K, np.arange(7), DC.neighbour_table(7, 2), *DC.relative_rows(ED.pose_matrices(pose)[:, :3] * 0 + np.linalg.inv(
        ED.pose_matrices(pose))[:, :3], np.arange(7), DC.neighbour_table(7, 2)), float("inf"))
    want = np.where((s_ >= 2) & (v_ == 0), noisy, 0)
    assert np.array_equal(got.depth.numpy(), want) and not got.depth.numpy()[mask].any() and (got.depth.numpy() > 0).mean() > 0.7


@pytest.mark.parametrize("extra", [["--depth-consistency"], ["--mesh", "--depth-consistency", "--consistency-window", "9"],
                                   ["--mesh", "--depth-consistency", "--consistency-window", "0"],
                                   ["--mesh", "--depth-consistency", "--consistency-rel", "1.5"],
                                   ["--mesh", "--depth-consistency", "--consistency-pix", "0"],
                                   ["--mesh", "--depth-consistency", "--consistency-min-support", "-1"]])
def test_demo_refuses_bad_consistency_flags(extra, tmp_path):
    import demo
    with pytest.raises(SystemExit) as e:
        demo.main(["--imagedir", str(tmp_path), "--calib", "c.txt", "--output", str(tmp_path / "o")] + extra)
    assert e.value.code == 2
