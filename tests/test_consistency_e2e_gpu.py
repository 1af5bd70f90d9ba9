"""GPU, end to end: the opt-in `consistency=` of tsdf.fuse_keyframes and eval_dense.from_keyframes on the box room with injected floaters
(tests/consistency_oracle.py): the keyword is the manual filter followed by the plain call, None is the call without it, and the
filtered fusion has no surface inside the room where the unfiltered one has."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cut3r_slam_amd import depth_consistency as DC  # noqa: E402
from cut3r_slam_amd import eval_dense as ED  # noqa: E402
from cut3r_slam_amd import tsdf as T  # noqa: E402
from tests import consistency_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VOXEL, TRUNC_VOXELS, DEPTH_MAX = 0.1, 3.0, 6.0
OPTS = DC.ConsistencyOptions()


@pytest.fixture(scope="module")
def scene():
    depth, w2c, K = O.box_room()
    noisy, mask = O.inject_floaters(depth, 0.03, 0)
    return noisy, mask, w2c, K


def _store(depth, w2c, K):
    n, H, W = depth.shape
    g = torch.Generator().manual_seed(0)
    return SimpleNamespace(device=torch.device(DEV), depth=torch.as_tensor(depth).to(DEV), w2c=torch.from_numpy(w2c).float().to(DEV),
                           image=torch.randint(0, 256, (n, 3, H, W), generator=g, dtype=torch.uint8).to(DEV),
                           intrinsic=torch.from_numpy(K).to(DEV), conf_ds=None, downsample_ratio=1)


def _bits(vol):
    return [t.cpu().numpy().view(np.int32) for t in (vol.tsdf, vol.weight, vol.color)]


def _fuse(kf, sparse, **kw):
    return T.fuse_keyframes(kf, kf.depth.shape[0], VOXEL, trunc_voxels=TRUNC_VOXELS, depth_max=DEPTH_MAX, sparse=sparse, **kw)


@pytest.mark.parametrize("sparse", [False, True])
def test_the_keyword_is_the_manual_filter_then_the_plain_fusion(scene, sparse):
    noisy, mask, w2c, K = scene
    kf = _store(noisy, w2c, K)
    got = _fuse(kf, sparse, consistency=OPTS)
    filtered, keep = DC.apply(kf.depth, kf.w2c, kf.intrinsic, OPTS, DEPTH_MAX)
    assert not bool(filtered[torch.from_numpy(mask).to(DEV)].any()) and 0.7 < float(keep.float().mean()) < 0.85
    assert int(got.consistency[0]) == int(keep.sum()) and int(got.consistency[1]) == noisy.size
    want = _fuse(_store(filtered, w2c, K), sparse)
    assert got.dims == want.dims and got.origin == want.origin and want.consistency is None
    if sparse:
        assert torch.equal(got.bricks, want.bricks) and got.n_bricks > 0
    for a, b in zip(_bits(got), _bits(want)):
        assert a.shape == b.shape and np.array_equal(a, b)
    # None is the call without the keyword
    plain, none = _fuse(kf, sparse), _fuse(kf, sparse, consistency=None)
    assert plain.dims == none.dims and all(np.array_equal(a, b) for a, b in zip(_bits(plain), _bits(none)))
    assert plain.dims != got.dims or not np.array_equal(_bits(plain)[0], _bits(got)[0])


def test_from_keyframes_hands_on_the_filtered_stack(scene):
    noisy, mask, w2c, K = scene
    c, Rm = O.room_cameras()
    pose = np.zeros((7, 7))
    pose[:, :3] = c
    for i, R in enumerate(Rm):
        w = 0.5 * np.sqrt(1 + np.trace(R))
        pose[i, 3:] = [(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w]
    kf = SimpleNamespace(depth=torch.from_numpy(noisy).to(DEV), pose=torch.from_numpy(pose), intrinsic=torch.from_numpy(K),
                         tstamp=torch.arange(7.0), image=torch.zeros(7, 3, 48, 64, dtype=torch.uint8))
    plain = ED.from_keyframes(kf, 7)
    got = ED.from_keyframes(kf, 7, consistency=OPTS)
    assert torch.equal(plain.depth, kf.depth)
    want, keep = DC.apply(kf.depth, np.linalg.inv(ED.pose_matrices(pose))[:, :3], K, OPTS, float("inf"))
    assert torch.equal(got.depth, want) and not bool(got.depth[torch.from_numpy(mask).to(DEV)].any()) and float(keep.float().mean()) > 0.7
    assert np.array_equal(got.c2w, plain.c2w) and np.array_equal(got.stamps, plain.stamps) and np.array_equal(got.K, plain.K)
    # the quaternion poses are the scene's cameras up to rounding: the same pixels survive as with the exact rows
    exact, _ = DC.apply(kf.depth, w2c, K, OPTS, float("inf"))
    assert float(((exact > 0) != (want > 0)).float().mean()) < 1e-3


def _inside(vertices):
    """how far inside the room's walls each vertex lies (negative: outside)"""
    return (np.asarray(O.ROOM)[None] - np.abs(vertices)).min(1)


def test_the_filtered_mesh_has_no_surface_inside_the_room(scene):
    """a floater seen once leaves a weight-1 shell in the middle of the room; after the filter every vertex lies within one truncation
    distance of a wall"""
    noisy, mask, w2c, K = scene
    kf = _store(noisy, w2c, K)
    trunc = TRUNC_VOXELS * VOXEL
    raw = _fuse(kf, False).extract_mesh(1.0)
    clean = _fuse(kf, False, consistency=OPTS).extract_mesh(1.0)
    assert len(raw.faces) > 1000 and len(clean.faces) > 1000
    assert (_inside(raw.vertices) > trunc).sum() > 0               # the numpy fusion of this scene leaves 60 such vertices
    assert _inside(clean.vertices).max() <= trunc


def test_demo_depth_consistency_reaches_the_fusion(tmp_path, monkeypatch, capsys):
    """one tiny demo.py --mesh --depth-consistency run with random weights: the flags arrive at Cut3rSlam.fuse as ConsistencyOptions, the
    share of kept pixels is printed and the mesh is written.  (The random network's depth scale sets the voxel, so the spy on fuse
    replaces the command line's voxel size and depth range by the store's; min_support 0 keeps what no neighbour sees through.)"""
    import re
    import demo
    from cut3r_slam_amd.slam import Cut3rSlam
    from tests.test_stream_gpu import _write_sequence
    d = tmp_path / "colors"
    d.mkdir()
    _write_sequence(str(d), 36)
    (tmp_path / "calib.txt").write_text("600.0 600.0 320.0 240.0")
    seen, real = [], Cut3rSlam.fuse

    def fuse(self, voxel_size, depth_max=5.0, **k):
        kf = self.keyframes
        n = kf.counter.value - 1
        dep = kf.depth[:n]
        top = float(dep[(dep > 0) & torch.isfinite(dep)].max())
        lo, hi = T.depth_bounds(dep, kf.w2c[:n], kf.intrinsic[:n].to(DEV), top)
        seen.append(k)
        return real(self, float(np.max(hi - lo)) / 64, depth_max=top, **k)
    monkeypatch.setattr(Cut3rSlam, "fuse", fuse)
    out = tmp_path / "out"
    rc = demo.main(["--imagedir", str(d), "--calib", str(tmp_path / "calib.txt"), "--kf_every", "2", "--synthetic-weights", "--small", "--seed", "1",
                    "--output", str(out), "--mesh", "--depth-consistency", "--consistency-window", "1", "--consistency-min-support", "0",
                    "--consistency-rel", "0.02", "--consistency-pix", "1.5"])
    assert rc == 0
    assert seen[0]["consistency"] == DC.ConsistencyOptions(window=1, min_support=0, max_violation=0, pix=1.5, rel=0.02, average=False)
    m = re.search(r"depth consistency \(window 1, support >= 0\): (\d+) of (\d+) valid pixels kept", capsys.readouterr().out)
    assert m and 0 < int(m.group(1)) <= int(m.group(2))
    mesh = T.read_ply(out / "tsdf_mesh_w1.0.ply")
    assert np.isfinite(mesh.vertices).all() and (len(mesh.faces) == 0 or mesh.faces.max() < len(mesh.vertices))
