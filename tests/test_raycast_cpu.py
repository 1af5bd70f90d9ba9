"""CPU: the numpy restatement of the TSDF ray cast (tests/raycast_oracle.py) against things that are not the code under test: the analytic
sphere the volume was fused from, and the marching-tetrahedra mesh of the same volume rendered by the rasteriser's oracle -- two
independent readings of one volume.  The kernels are then pinned to this oracle bit for bit (tests/test_raycast_gpu.py)."""
import numpy as np
import pytest

from tests import raster_oracle as RO
from tests import raycast_oracle as R
from tests import tsdf_oracle as O

f32 = np.float32
H, W = R.CAST_HW
STEP = float(f32(0.5 * f32(R.VOXEL)))
T_MAX = 5.0


@pytest.fixture(scope="module")
def scene():
    vol, origin, dims, trunc, _ = R.fused_sphere()
    assert dims == (67, 67, 67)
    w2c = R.pose_rows(list(R.POSES.values()))
    depth, normal, rgb = R.ray_cast(vol, origin, R.VOXEL, w2c, R.cast_K(), H, W, 0.0, T_MAX, STEP)
    return {"vol": vol, "origin": origin, "w2c": w2c, "depth": depth, "normal": normal, "rgb": rgb}


def _analytic(eye):
    """(depth [H,W] fp64, unit normals [H,W,3], interior mask: the 3 x 3 neighbourhood lies in the image and is all hits)"""
    T = O.look_at(eye)
    K = R.cast_K().astype(np.float64)
    d, _ = O.render_sphere(T, K, H, W, R.RADIUS)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dw = np.stack([(u - K[2]) / K[0], (v - K[3]) / K[1], np.ones_like(u)], -1) @ T[:3, :3]
    p = np.asarray(eye, np.float64) + d[..., None] * dw
    hit = d > 0
    inner = np.zeros_like(hit)
    inner[1:-1, 1:-1] = True
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            inner[1:-1, 1:-1] &= hit[1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx]
    return d, p / R.RADIUS, inner


# measured with this oracle (maximum over the interior pixels): depth error in voxels and normal angle in degrees, per pose; the bounds
# are those maxima plus a quarter
MEASURED = {"oblique": (1.477, 86.66), "far": (1.291, 58.05), "near": (1.159, 75.02)}


@pytest.mark.parametrize("b,name", list(enumerate(R.POSES)))
def test_interior_pixels_hit_the_analytic_sphere(scene, b, name):
    d, n, inner = _analytic(R.POSES[name])
    assert inner.sum() >= 300
    got = scene["depth"][b]
    assert np.all(got[inner] > 0), f"{np.count_nonzero(got[inner] == 0)} interior pixels missed"
    err = np.abs(got[inner].astype(np.float64) - d[inner]) / R.VOXEL
    cosang = np.clip((scene["normal"][b][inner].astype(np.float64) * n[inner]).sum(-1), -1, 1)
    ang = np.degrees(np.arccos(cosang))
    print(f"{name}: {inner.sum()} interior pixels, depth error max {err.max():.3f} median {np.median(err):.3f} voxels, "
          f"normal angle max {ang.max():.2f} median {np.median(ang):.2f} degrees")
    e_max, a_max = MEASURED[name]
    assert err.max() <= 1.25 * e_max
    assert ang.max() <= 1.25 * a_max
    lens = np.linalg.norm(scene["normal"][b][got > 0].astype(np.float64), axis=-1)
    assert np.all(np.abs(lens - 1) < 1e-6)
    assert not scene["normal"][b][got == 0].any() and not scene["rgb"][b][:, got == 0].any()


def test_exact_distance_field_gives_the_analytic_depth_and_normal():
    """The large normal angles above are the fused volume's (nearest-pixel lookup leaves steps in its tsdf), not the cast's: on the
    exact distance field of the same sphere every hit lies within a tenth of a voxel and every normal within a few degrees.  Measured
    with this oracle: 0.0874 voxel and 2.48 degrees at most; the bounds are those plus a quarter."""
    origin, dims, trunc = O.sphere_grid(R.VOXEL, R.RADIUS)
    px, py, pz = (a.astype(np.float64) for a in O.centres(origin, f32(R.VOXEL), dims))
    sd = (np.sqrt(px * px + py * py + pz * pz) - R.RADIUS) / trunc
    vol = (np.clip(sd, -1, 1).astype(f32), np.ones(sd.shape, f32), np.zeros((3,) + sd.shape, f32))
    depth, normal, _ = R.ray_cast(vol, origin, R.VOXEL, R.pose_rows(list(R.POSES.values())), R.cast_K(), H, W, 0.0, T_MAX, STEP)
    for b, name in enumerate(R.POSES):
        d, n, inner = _analytic(R.POSES[name])
        assert np.array_equal(depth[b][inner] > 0, d[inner] > 0)
        err = np.abs(depth[b][inner].astype(np.float64) - d[inner]) / R.VOXEL
        ang = np.degrees(np.arccos(np.clip((normal[b][inner].astype(np.float64) * n[inner]).sum(-1), -1, 1)))
        print(f"{name}: exact field, depth error max {err.max():.4f} voxels, normal angle max {ang.max():.2f} degrees")
        assert err.max() <= 1.25 * 0.0874 and ang.max() <= 1.25 * 2.48


# measured with this oracle: (pixels whose hit masks differ, mesh hit pixels, share of the pixels both hit that differ by more than half
# a voxel); the cap on the share is the measured one plus a quarter
MESH_MEASURED = {"oblique": (6, 1093, 0.0110), "near": (0, 3072, 0.0016)}


def test_ray_cast_agrees_with_the_marching_tetrahedra_mesh(scene):
    verts, _, faces = O.extract(scene["vol"], scene["origin"], R.VOXEL, 1.0)
    sel = [0, 2]
    mesh_depth, _ = RO.render(verts, faces, scene["w2c"][sel], R.cast_K(), H, W)
    for q, name in zip(range(2), ("oblique", "near")):
        md, rd = mesh_depth[q], scene["depth"][sel[q]]
        mh, rh = md > 0, rd > 0
        both = mh & rh
        diff = np.abs(md[both].astype(np.float64) - rd[both]) / R.VOXEL
        share = float((diff > 0.5).mean())
        print(f"{name}: masks differ on {np.count_nonzero(mh != rh)} of {mh.sum()} mesh pixels; of {both.sum()} common pixels {share:.4f} "
              f"differ by > 0.5 voxel, max {diff.max():.2f} median {np.median(diff):.3f} voxels")
        assert np.count_nonzero(mh != rh) <= 0.01 * mh.sum()
        assert share <= 1.25 * MESH_MEASURED[name][2]


def test_special_cameras_miss_everywhere(scene):
    vol, origin = scene["vol"], scene["origin"]
    K = R.cast_K()
    inside = R.pose_rows([(0.0, 0.0, 0.0)], target=(1.0, 0.2, 0.1))
    away = R.pose_rows([R.POSES["oblique"]], target=(3.0, 3.0, 3.0))
    for w2c, t_max in ((inside, T_MAX), (away, T_MAX), (scene["w2c"][1:2], 1.5)):
        depth, normal, rgb = R.ray_cast(vol, origin, R.VOXEL, w2c, K, H, W, 0.0, t_max, STEP)
        assert not depth.any() and not normal.any() and not rgb.any()
    # and the far camera does see the sphere when depth_max allows it
    assert (scene["depth"][1] > 0).sum() > 300
