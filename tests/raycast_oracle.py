"""numpy restatement of csrc/tsdf_raycast.hip: the PLAIN march of the TSDF ray cast, every sample from k = 0 up to t_max, vectorised over
the pixels of a view, in fp32 and in the kernel's order of operations (the kernel is compiled with -ffp-contract=off), so depth, normal
and colour are compared bit for bit.  None of the kernel's accelerations is restated: they must not be visible.  The scenes are those of
tests/tsdf_oracle.py."""
from __future__ import annotations

import numpy as np

from tests import tsdf_oracle as O

f32 = np.float32


def c2w_rows(w2c):
    """camera->world rows fp32 [B,12] of world->camera rows (cut3r_slam_amd.tsdf.c2w_rows: the inverse in float64)"""
    w = np.asarray(w2c, np.float64).reshape(-1, 3, 4)
    Ri = np.linalg.inv(w[:, :, :3])
    ti = -(Ri @ w[:, :, 3:])
    return np.ascontiguousarray(np.concatenate([Ri, ti], 2).reshape(-1, 12), dtype=f32)


def _lerp(a, b, f):
    return a + f * (b - a)


def _trilinear(v, fx, fy, fz):
    """x, then y, then z over the corner values v[e] (bit 0 of e = +x, bit 1 = +y, bit 2 = +z)"""
    c0 = _lerp(_lerp(v[0], v[1], fx), _lerp(v[2], v[3], fx), fy)
    c1 = _lerp(_lerp(v[4], v[5], fx), _lerp(v[6], v[7], fx), fy)
    return _lerp(c0, c1, fz)


def _bilinear(q0, q1, q2, q3, fa, fb):
    return _lerp(_lerp(q0, q1, fa), _lerp(q2, q3, fa), fb)


def _cast_view(vol, origin, voxel, c2w, K, H, W, t_min, t_max, step, wth):
    tsdf, weight, color = vol
    Z, Y, X = tsdf.shape
    dims = (X, Y, Z)
    r = np.asarray(c2w, f32).reshape(12)
    fx, fy, cx, cy = (f32(a) for a in np.asarray(K, f32).reshape(4))
    o = [f32(a) for a in origin]
    voxel, t_min, t_max, step, wth = f32(voxel), f32(t_min), f32(t_max), f32(step), f32(wth)
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    xc = ((u.astype(f32) - cx) / fx).reshape(-1)
    yc = ((v.astype(f32) - cy) / fy).reshape(-1)
    c = [r[a * 4 + 3] for a in range(3)]
    d = [(r[a * 4] * xc + r[a * 4 + 1] * yc) + r[a * 4 + 2] for a in range(3)]
    n = H * W
    depth = np.zeros(n, f32)
    normal = np.zeros((n, 3), f32)
    rgb = np.zeros((3, n), np.uint8)
    alive = np.arange(n)                                   # the rays that have not ended
    have = np.zeros(n, bool)                               # per ray: the predecessor is there
    sp, tp = np.zeros(n, f32), np.zeros(n, f32)
    k = 0
    with np.errstate(all="ignore"):
        while alive.size:
            tk = t_min + f32(k) * step
            if not tk <= t_max:
                break
            k += 1
            fl, fr = [], []
            inb = np.ones(alive.size, bool)
            for a in range(3):
                g = ((c[a] + tk * d[a][alive]) - o[a]) / voxel
                fa = np.floor(g)
                fl.append(fa)
                fr.append(g - fa)
                inb &= (fa >= 0) & (fa < f32(dims[a] - 1))
            have[alive[~inb]] = False
            if not inb.any():
                continue
            sel = alive[inb]
            ci, cj, ck = (fl[a][inb].astype(np.int64) for a in range(3))
            f = [fr[a][inb] for a in range(3)]
            corner = lambda p: [p[ck + ((e >> 2) & 1), cj + ((e >> 1) & 1), ci + (e & 1)] for e in range(8)]
            valid = np.ones(sel.size, bool)
            for w in corner(weight):
                valid &= w >= wth
            val = corner(tsdf)
            s = _trilinear(val, f[0], f[1], f[2])
            neg = valid & (s < 0)
            hit = neg & have[sel]
            if hit.any():
                hs = sel[hit]
                depth[hs] = tp[hs] + (tk - tp[hs]) * (sp[hs] / (sp[hs] - s[hit]))
                hv = [q[hit] for q in val]
                h = [q[hit] for q in f]
                gx = _bilinear(hv[1] - hv[0], hv[3] - hv[2], hv[5] - hv[4], hv[7] - hv[6], h[1], h[2])
                gy = _bilinear(hv[2] - hv[0], hv[3] - hv[1], hv[6] - hv[4], hv[7] - hv[5], h[0], h[2])
                gz = _bilinear(hv[4] - hv[0], hv[5] - hv[1], hv[6] - hv[2], hv[7] - hv[3], h[0], h[1])
                ln = np.sqrt((gx * gx + gy * gy) + gz * gz)
                pos = ln > 0
                for a, ga in enumerate((gx, gy, gz)):
                    normal[hs, a] = np.where(pos, ga / np.where(pos, ln, f32(1)), f32(0))
                for a in range(3):
                    cv = [q[hit] for q in corner(color[a])]
                    cc = np.floor(_trilinear(cv, h[0], h[1], h[2]) + f32(0.5))
                    rgb[a, hs] = np.minimum(f32(255), np.maximum(f32(0), cc)).astype(np.uint8)
            keep = valid & ~neg                            # becomes the predecessor
            have[sel] = keep
            sp[sel[keep]] = s[keep]
            tp[sel[keep]] = tk
            ended = np.zeros(alive.size, bool)
            ended[np.flatnonzero(inb)[neg]] = True
            alive = alive[~ended]
    return depth.reshape(H, W), normal.reshape(H, W, 3), rgb.reshape(3, H, W)


def ray_cast(vol, origin, voxel, w2c, K, H, W, t_min, t_max, step, weight_threshold=1.0):
    """vol = (tsdf [Z,Y,X], weight, color [3,Z,Y,X]); w2c [B,12] world->camera rows, K [4] or [B,4] -> depth fp32 [B,H,W] (0 on a miss),
    normal fp32 [B,H,W,3], rgb u8 [B,3,H,W]"""
    c2w = c2w_rows(w2c)
    B = c2w.shape[0]
    K = np.broadcast_to(np.asarray(K, f32).reshape(-1, 4), (B, 4))
    out = [_cast_view(vol, origin, voxel, c2w[b], K[b], H, W, t_min, t_max, step, weight_threshold) for b in range(B)]
    return tuple(np.stack(q) for q in zip(*out))


# ------------------------------------------------------------------------------------------------------------------------ scenes
VOXEL, RADIUS, CAST_HW, CAST_F = 0.02, 0.5, (48, 64), 55.0
POSES = {"oblique": (1.1, 0.9, 0.7), "far": (0.0, -2.5, 0.3), "near": (0.75, 0.1, -0.2)}


def cast_K(H=CAST_HW[0], W=CAST_HW[1], f=CAST_F):
    return np.asarray((f, f, (W - 1) / 2, (H - 1) / 2), f32)


def pose_rows(eyes, target=(0.0, 0.0, 0.0)):
    """world->camera rows fp32 [B,12] of cameras at `eyes` looking at the target"""
    return np.ascontiguousarray(np.stack([O.look_at(e, target)[:3].reshape(12) for e in eyes]), dtype=f32)


def fused_sphere():
    """the sphere of tsdf_oracle fused from 24 views of 96 x 128 into the 67^3 grid at voxel 0.02 -> (vol, origin, dims, trunc, views)"""
    views = O.sphere_scene(n_views=24, H=96, W=128, f=110.0, radius=RADIUS)
    depth, rgb, w2c, K = views
    origin, dims, trunc = O.sphere_grid(VOXEL, RADIUS)
    origin = tuple(float(f32(a)) for a in origin)
    vol = O.integrate(O.new_volume(dims), origin, float(f32(VOXEL)), depth, w2c, K, trunc, 5.0, rgb=rgb)
    return vol, origin, dims, trunc, views
