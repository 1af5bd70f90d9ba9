"""numpy restatement of csrc/tsdf.hip: TSDF integration and marching-tetrahedra extraction in fp32, every operation in the kernels'
order (the kernels are compiled with -ffp-contract=off), so the GPU volume and mesh are compared bit for bit.  Also the analytic scenes
of the TSDF tests (a sphere seen from all around)."""
from __future__ import annotations

import numpy as np

f32 = np.float32

# the six tetrahedra of a cell (axis permutations, lexicographic) and their parities; tetrahedron edges and the 16-case triangle table
PERM = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
PARITY = [1, -1, -1, 1, 1, -1]
EDGE = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
TRI = [[[-1, -1, -1], [-1, -1, -1]], [[0, 1, 2], [-1, -1, -1]], [[0, 4, 3], [-1, -1, -1]], [[1, 2, 4], [1, 4, 3]],
       [[1, 3, 5], [-1, -1, -1]], [[0, 5, 2], [0, 3, 5]], [[0, 4, 5], [0, 5, 1]], [[2, 4, 5], [-1, -1, -1]],
       [[2, 5, 4], [-1, -1, -1]], [[0, 1, 5], [0, 5, 4]], [[0, 5, 3], [0, 2, 5]], [[1, 5, 3], [-1, -1, -1]],
       [[1, 3, 4], [1, 4, 2]], [[0, 3, 4], [-1, -1, -1]], [[0, 2, 1], [-1, -1, -1]], [[-1, -1, -1], [-1, -1, -1]]]
NTRI = [0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0]


def chain(t):
    """cell corners (bit 0 = +x, 1 = +y, 2 = +z) of tetrahedron t: 0 -> 1<<p0 -> (1<<p0)|(1<<p1) -> 7"""
    p = PERM[t]
    a = 1 << p[0]
    return [0, a, a | (1 << p[1]), 7]


def new_volume(dims):
    X, Y, Z = dims
    return np.ones((Z, Y, X), f32), np.zeros((Z, Y, X), f32), np.zeros((3, Z, Y, X), f32)


def centres(origin, voxel, dims):
    X, Y, Z = dims
    k, j, i = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    v = f32(voxel)
    return (f32(origin[0]) + v * i.astype(f32), f32(origin[1]) + v * j.astype(f32), f32(origin[2]) + v * k.astype(f32))


def integrate(vol, origin, voxel, depth, w2c, K, trunc, depth_max, rgb=None, conf=None, conf_ds=1, conf_min=None):
    """in place on vol = (tsdf, weight, color): the views of depth [B,H,W] applied in order (the kernel's per-voxel loop over a batch
    gives the same values as one view after the other over the whole grid)"""
    tsdf, weight, color = vol
    Z, Y, X = tsdf.shape
    px, py, pz = centres(origin, voxel, (X, Y, Z))
    depth = np.asarray(depth, f32)
    B, H, W = depth.shape
    w2c = np.asarray(w2c, f32).reshape(B, 12)
    K = np.asarray(K, f32).reshape(-1, 4)
    K = np.broadcast_to(K, (B, 4))
    trunc, depth_max = f32(trunc), f32(depth_max)
    gate = conf is not None and conf_min is not None
    for b in range(B):
        r, (fx, fy, cx, cy) = w2c[b], K[b]
        with np.errstate(all="ignore"):
            zc = ((r[8] * px + r[9] * py) + r[10] * pz) + r[11]
            xc = ((r[0] * px + r[1] * py) + r[2] * pz) + r[3]
            yc = ((r[4] * px + r[5] * py) + r[6] * pz) + r[7]
            ok = zc > 0
            u = (fx * xc) / zc + cx
            v = (fy * yc) / zc + cy
            uf, vf = np.floor(u + f32(0.5)), np.floor(v + f32(0.5))
            ok &= (uf >= 0) & (uf < f32(W)) & (vf >= 0) & (vf < f32(H))
        ui = np.where(ok, uf, 0).astype(np.int64)
        vi = np.where(ok, vf, 0).astype(np.int64)
        d = depth[b][vi, ui]
        with np.errstate(invalid="ignore"):
            ok &= (d > 0) & (d <= depth_max)
        if gate:
            c = np.asarray(conf[b], f32)
            ch, cw = c.shape
            ok &= ~(c[np.minimum(vi // conf_ds, ch - 1), np.minimum(ui // conf_ds, cw - 1)] < f32(conf_min))
        with np.errstate(all="ignore"):
            sdf = d - zc
            ok &= ~(sdf < -trunc)
            t = np.minimum(f32(1), sdf / trunc)
        w = weight[ok]
        w1 = w + f32(1)
        tsdf[ok] = (tsdf[ok] * w + t[ok]) / w1
        if rgb is not None:
            im = np.asarray(rgb[b])
            for c_ in range(3):
                col = im[c_][vi[ok], ui[ok]].astype(f32)
                color[c_][ok] = (color[c_][ok] * w + col) / w1
        weight[ok] = w1
    return vol


def extract(vol, origin, voxel, weight_threshold=1.0):
    """marching tetrahedra -> (vertices f32 [V,3], colors u8 [V,3], faces i32 [F,3]) in the kernels' order"""
    tsdf, weight, color = vol
    Z, Y, X = tsdf.shape
    N = X * Y * Z
    if min(X, Y, Z) < 2:
        return np.zeros((0, 3), f32), np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.int32)
    cz, cy, cx = np.meshgrid(np.arange(Z - 1), np.arange(Y - 1), np.arange(X - 1), indexing="ij")
    cell_n = ((cz * Y + cy) * X + cx).reshape(-1)

    def corner(a, e):
        return a[(e >> 2) & 1:Z - 1 + ((e >> 2) & 1), (e >> 1) & 1:Y - 1 + ((e >> 1) & 1), e & 1:X - 1 + (e & 1)].reshape(-1)

    inside = [corner(tsdf, e) < 0 for e in range(8)]
    valid = np.ones(cell_n.shape, bool)
    for e in range(8):
        valid &= corner(weight, e) >= f32(weight_threshold)
    off = [(e & 1) + ((e >> 1) & 1) * X + ((e >> 2) & 1) * X * Y for e in range(8)]
    keys = np.full((cell_n.size, 6, 2, 3), -1, np.int64)       # vertex key = owning voxel * 8 + direction mask
    for t in range(6):
        cc = chain(t)
        cs = sum(inside[cc[q]].astype(np.int64) << q for q in range(4))
        for r in range(2):
            for case in range(16):
                if NTRI[case] <= r:
                    continue
                sel = valid & (cs == case)
                tri = TRI[case][r]
                order = [0, 2, 1] if PARITY[t] < 0 else [0, 1, 2]
                for q, qq in enumerate(order):
                    a, b = EDGE[tri[qq]]
                    lo, m = cc[a], cc[a] ^ cc[b]
                    keys[sel, t, r, q] = (cell_n[sel] + off[lo]) * 8 + m
    keys = keys.reshape(-1, 3)
    keys = keys[keys[:, 0] >= 0]
    uniq = np.unique(keys)
    faces = np.searchsorted(uniq, keys).astype(np.int32)
    n, m = uniq // 8, uniq % 8
    i, j, k = n % X, (n // X) % Y, n // (X * Y)
    u = n + (m & 1) + ((m >> 1) & 1) * X + ((m >> 2) & 1) * X * Y
    ts = tsdf.reshape(-1)
    t0, t1 = ts[n], ts[u]
    s = t0 / (t0 - t1)
    v = f32(voxel)
    verts = np.empty((uniq.size, 3), f32)
    for a, (idx, bit) in enumerate(((i, 1), (j, 2), (k, 4))):
        p0 = f32(origin[a]) + v * idx.astype(f32)
        p1 = f32(origin[a]) + v * (idx + ((m & bit) > 0)).astype(f32)
        verts[:, a] = p0 + s * (p1 - p0)
    cols = np.empty((uniq.size, 3), np.uint8)
    cf = color.reshape(3, N)
    for a in range(3):
        ca, cb = cf[a][n], cf[a][u]
        c = np.floor((ca + s * (cb - ca)) + f32(0.5))
        cols[:, a] = np.minimum(f32(255), np.maximum(f32(0), c)).astype(np.uint8)
    return verts, cols, faces


# ------------------------------------------------------------------------------------------------------------------ scenes
def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """world->camera 4x4 (float64) of a camera at eye looking at target (x right, y down, z forward)"""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    if np.linalg.norm(x) < 1e-9:
        x = np.cross(z, (1.0, 0.0, 0.0))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, -R @ eye
    return T


def sphere_poses(n, dist, seed=0):
    """n cameras on a sphere of radius dist (Fibonacci spiral with a seeded jitter), all looking at the origin"""
    g = np.random.default_rng(seed)
    out = []
    for a in range(n):
        zc = 1 - 2 * (a + 0.5) / n
        ph = a * np.pi * (3 - np.sqrt(5)) + g.uniform(-0.1, 0.1)
        rr = np.sqrt(1 - zc * zc)
        eye = dist * np.array([rr * np.cos(ph), rr * np.sin(ph), zc])
        out.append(look_at(eye, target=g.uniform(-0.02, 0.02, 3)))
    return np.stack(out)


def render_sphere(w2c44, K, H, W, radius, center=(0.0, 0.0, 0.0)):
    """float64 ray cast of a sphere: z-depth [H,W] (0 where the ray misses) and a colour u8 [3,H,W] that varies over the surface"""
    fx, fy, cx, cy = K
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dc = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    R, t = w2c44[:3, :3], w2c44[:3, 3]
    eye = -R.T @ t
    dw = dc @ R                                              # R^T d
    oc = eye - np.asarray(center, np.float64)
    a = (dw * dw).sum(-1)
    b = 2 * (dw @ oc)
    c = oc @ oc - radius * radius
    disc = b * b - 4 * a * c
    hit = disc > 0
    s = np.where(hit, (-b - np.sqrt(np.where(hit, disc, 0))) / (2 * a), 0)
    depth = np.where(hit & (s > 0), s, 0.0)                  # z of the hit (the ray direction has z = 1 in the camera frame)
    p = eye + s[..., None] * dw
    col = np.stack([127.5 + 120 * np.sin(4 * p[..., 0]), 127.5 + 120 * np.cos(3 * p[..., 1]), 127.5 + 120 * np.sin(5 * p[..., 2])])
    col = np.where(depth > 0, col, 0).round().astype(np.uint8)
    return depth, col


def sphere_scene(n_views=24, H=96, W=128, f=110.0, radius=0.5, dist=1.6, seed=0):
    """(depth f32 [B,H,W], rgb u8 [B,3,H,W], w2c f32 [B,12], K f32 [4]) of the sphere from n_views poses around it"""
    K = (f, f, (W - 1) / 2, (H - 1) / 2)
    poses = sphere_poses(n_views, dist, seed)
    ds, cs = zip(*(render_sphere(T, K, H, W, radius) for T in poses))
    return (np.stack(ds).astype(f32), np.stack(cs), np.ascontiguousarray(poses[:, :3, :].reshape(-1, 12), dtype=f32),
            np.asarray(K, f32))


def sphere_grid(voxel=0.02, radius=0.5, trunc_voxels=8.0):
    """(origin, dims, trunc) of the grid around the sphere padded by the truncation distance"""
    pad = radius + trunc_voxels * voxel
    n = int(np.floor(2 * pad / voxel)) + 1
    o = float(f32(-pad))
    return (o, o, o), (n, n, n), float(f32(trunc_voxels * f32(voxel)))
