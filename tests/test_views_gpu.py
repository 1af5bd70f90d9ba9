"""GPU: the consumers of posed depth maps give the same bits whichever layout the poses ([B,12], [B,3,4], [B,4,4]) and the intrinsics ([4],
[B,4]) arrive in -- TSDFVolume.integrate + ray_cast, ops.mesh_raster, ops.depth_cloud, depth_consistency.consistency -- on 3 views of
24 x 32 and a grid of 29^3 voxels."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cut3r_slam_amd import depth_consistency as DC  # noqa: E402
from cut3r_slam_amd import ops  # noqa: E402
from cut3r_slam_amd import tsdf as T  # noqa: E402
from tests import tsdf_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H, W = 3, 24, 32
VOXEL, TRUNC_VOXELS = 0.05, 4.0


def _layouts(rows12, K4):
    """every (poses, K) pair for the same B poses; the first is [B,12] with K [B,4]"""
    m = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    m[:, :3] = rows12.reshape(B, 3, 4)
    return [(p, k) for p in (rows12, rows12.reshape(B, 3, 4), m, torch.from_numpy(m).to(DEV)) for k in (np.stack([K4] * B), K4)]


@pytest.fixture(scope="module")
def scene():
    depth, rgb, w2c, K = O.sphere_scene(n_views=B, H=H, W=W, f=30.0)
    return torch.from_numpy(depth).to(DEV), torch.from_numpy(rgb).to(DEV), w2c, K


def _same(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and torch.equal(a, b)


def test_fusion_and_ray_cast_do_not_depend_on_the_layout(scene):
    depth, rgb, w2c, K = scene
    origin, dims, _ = O.sphere_grid(VOXEL, trunc_voxels=TRUNC_VOXELS)
    assert max(dims) <= 32
    want = None
    for poses, k in _layouts(w2c, K):
        vol = T.TSDFVolume(origin, VOXEL, dims, trunc_voxels=TRUNC_VOXELS, depth_max=3.0, device=DEV).integrate(depth, poses, k, rgb=rgb)
        rc = vol.ray_cast(poses, k, H, W)
        got = (vol.tsdf, vol.weight, vol.color, rc.depth, rc.normal, rc.color)
        if want is None:
            want = got
            assert bool((vol.weight > 0).any()) and bool((rc.depth > 0).any())
        _same(got, want)


def test_the_rasteriser_the_cloud_and_the_consistency_filter_do_not_depend_on_the_layout(scene):
    depth, rgb, w2c, K = scene
    verts = torch.tensor([[0.3, 0, 0], [-0.3, 0, 0], [0, 0.3, 0], [0, -0.3, 0], [0, 0, 0.3], [0, 0, -0.3]], dtype=torch.float32, device=DEV)
    faces = torch.tensor([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], dtype=torch.int32, device=DEV)
    c2w = T.c2w_rows(w2c)
    want = None
    for (poses, k), (inv, _) in zip(_layouts(w2c, K), _layouts(c2w, K)):
        raster = ops.mesh_raster(verts, faces, poses, k, H, W, face_id=True)
        points, colors, counts = ops.depth_cloud(depth, inv, k, 3.0, rgb=rgb)
        got = (*raster, points, colors, counts, *DC.consistency(depth, poses, k, depth_max=3.0, average=True))
        if want is None:
            want = got
            assert bool((raster[0] > 0).any()) and points.shape[0] > 0
        _same(got, want)
