"""numpy restatement of csrc/tsdf_sparse.hip: the brick mark rule in the kernel's fp32 order (the GPU flags are compared exactly), the
dense oracle (tests/tsdf_oracle.py) evaluated on a WINDOW of a larger lattice -- positions origin + voxel * float(i0 + i), which a
sub-grid with a shifted origin does not reproduce bit for bit -- and a canonical form of a mesh as a set of triangles, for meshes that
agree up to the order of their vertices and faces."""
from __future__ import annotations

import contextlib

import numpy as np

from tests import tsdf_oracle as O

f32 = np.float32
BRICK = 8
SEGMENTS = 2


def brick_dims(dims):
    return tuple((int(d) + BRICK - 1) // BRICK for d in dims)


def c2w_rows(w2c):
    """camera->world rows fp32 [B,12]: the float64 inverse of each world->camera 3x4 map"""
    w = np.asarray(w2c, np.float64).reshape(-1, 3, 4)
    Ri = np.linalg.inv(w[:, :, :3])
    ti = -(Ri @ w[:, :, 3:])
    return np.ascontiguousarray(np.concatenate([Ri, ti], 2).reshape(-1, 12), dtype=f32)


def _mark_range(lo, hi, o, voxel, dim):
    """per pixel: (hit, first brick, last brick) of one axis -- the interval in voxel indices, dilated by 1.5, clamped to the grid"""
    with np.errstate(all="ignore"):
        flo = np.floor((lo - f32(o)) / voxel - f32(1.5))
        fhi = np.ceil((hi - f32(o)) / voxel + f32(1.5))
        hit = (fhi >= 0) & (flo <= f32(dim - 1))
        b0 = np.where(hit, np.maximum(flo, f32(0)), 0).astype(np.int64) >> 3
        b1 = np.where(hit, np.minimum(fhi, f32(dim - 1)), 0).astype(np.int64) >> 3
    return hit, b0, b1


def mark(flags, origin, voxel, dims, depth, w2c, K, trunc, depth_max):
    """in place on flags (bool or u8 [BZ,BY,BX]): every brick overlapped by the dilated world AABB of a z-segment of the slab
    u +- 0.5, v +- 0.5, z in [d, d + trunc] of a pixel with 0 < d <= depth_max"""
    depth = np.asarray(depth, f32)
    B, H, W = depth.shape
    c2w = c2w_rows(w2c)
    K = np.broadcast_to(np.asarray(K, f32).reshape(-1, 4), (B, 4))
    voxel, trunc, depth_max = f32(voxel), f32(trunc), f32(depth_max)
    for b in range(B):
        c, (fx, fy, cx, cy) = c2w[b], K[b]
        d = depth[b]
        with np.errstate(invalid="ignore"):
            vi, ui = np.nonzero((d > 0) & (d <= depth_max))
        d = d[vi, ui]
        uf, vf = ui.astype(f32), vi.astype(f32)
        ax = [((uf - f32(0.5)) - cx) / fx, ((uf + f32(0.5)) - cx) / fx]
        ay = [((vf - f32(0.5)) - cy) / fy, ((vf + f32(0.5)) - cy) / fy]
        for s in range(SEGMENTS):
            zz = [d + trunc * (f32(s) / f32(SEGMENTS)), d + trunc * (f32(s + 1) / f32(SEGMENTS))]
            lo = [np.full(d.shape, np.inf, f32) for _ in range(3)]
            hi = [np.full(d.shape, -np.inf, f32) for _ in range(3)]
            for q in range(8):
                z = zz[q >> 2]
                xc, yc = ax[q & 1] * z, ay[(q >> 1) & 1] * z
                for a in range(3):
                    w = ((c[a * 4] * xc + c[a * 4 + 1] * yc) + c[a * 4 + 2] * z) + c[a * 4 + 3]
                    lo[a], hi[a] = np.fmin(lo[a], w), np.fmax(hi[a], w)
            rng = [_mark_range(lo[a], hi[a], origin[a], voxel, dims[a]) for a in range(3)]
            hit = rng[0][0] & rng[1][0] & rng[2][0]
            (x0, x1), (y0, y1), (z0, z1) = ((r[1][hit], r[2][hit]) for r in rng)
            if not hit.any():
                continue
            for dz in range(int((z1 - z0).max()) + 1):
                for dy in range(int((y1 - y0).max()) + 1):
                    for dx in range(int((x1 - x0).max()) + 1):
                        m = (x0 + dx <= x1) & (y0 + dy <= y1) & (z0 + dz <= z1)
                        flags[z0[m] + dz, y0[m] + dy, x0[m] + dx] = 1
    return flags


def voxel_mask(flags, dims):
    """bool [Z,Y,X]: the voxels of the allocated bricks"""
    X, Y, Z = dims
    m = np.asarray(flags).astype(bool)
    return np.repeat(np.repeat(np.repeat(m, BRICK, 0), BRICK, 1), BRICK, 2)[:Z, :Y, :X]


def dilate26(m):
    """bool [Z,Y,X]: m or any of its 26 in-grid neighbours"""
    Z, Y, X = m.shape
    p = np.pad(m, 1)
    out = np.zeros_like(m)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                out |= p[dz:dz + Z, dy:dy + Y, dx:dx + X]
    return out


def masked(vol, vm):
    """the volume as the sparse one holds it: the initial state (1, 0, 0) outside the allocated voxels"""
    return np.where(vm, vol[0], f32(1)), np.where(vm, vol[1], f32(0)), np.where(vm[None], vol[2], f32(0))


# --------------------------------------------------------------------------------------------------------------------- windows
@contextlib.contextmanager
def _window_centres(offset):
    """O.integrate with voxel positions origin + voxel * float(offset + index): the one place where the dense oracle forms them"""
    i0, j0, k0 = offset
    real = O.centres

    def centres(origin, voxel, dims):
        X, Y, Z = dims
        k, j, i = np.meshgrid(np.arange(k0, k0 + Z), np.arange(j0, j0 + Y), np.arange(i0, i0 + X), indexing="ij")
        v = f32(voxel)
        return (f32(origin[0]) + v * i.astype(f32), f32(origin[1]) + v * j.astype(f32), f32(origin[2]) + v * k.astype(f32))

    O.centres = centres
    try:
        yield
    finally:
        O.centres = real


def integrate_window(vol, origin, voxel, offset, *args, **kwargs):
    """O.integrate on the window of the lattice (origin, voxel) that starts at the integer voxel offset (i0, j0, k0); vol has the
    window's shape"""
    with _window_centres(offset):
        return O.integrate(vol, origin, voxel, *args, **kwargs)


def extract_window(vol, origin, voxel, offset=(0, 0, 0), weight_threshold=1.0):
    """O.extract on such a window (outside the window = outside the grid): the same cells, tables, interpolation and colour rounding,
    the vertex positions from origin + voxel * float(offset + index).  With offset (0, 0, 0) it is O.extract."""
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
    keys = []                                                    # per face: vertex key = owning voxel * 8 + direction mask
    for t in range(6):
        cc = O.chain(t)
        cs = sum(inside[cc[q]].astype(np.int64) << q for q in range(4))
        order = [0, 2, 1] if O.PARITY[t] < 0 else [0, 1, 2]
        for case in range(1, 15):
            sel = np.nonzero(valid & (cs == case))[0]
            for r in range(O.NTRI[case]):
                tri = O.TRI[case][r]
                k3 = np.empty((sel.size, 3), np.int64)
                for q, qq in enumerate(order):
                    a, b = O.EDGE[tri[qq]]
                    k3[:, q] = (cell_n[sel] + off[cc[a]]) * 8 + (cc[a] ^ cc[b])
                keys.append(np.concatenate([cell_n[sel, None], np.full((sel.size, 1), t * 2 + r), k3], 1))
    keys = np.concatenate(keys)
    keys = keys[np.lexsort((keys[:, 1], keys[:, 0]))][:, 2:]       # faces by (cell, tetrahedron, triangle)
    uniq = np.unique(keys)
    faces = np.searchsorted(uniq, keys).astype(np.int32)
    n, m = uniq // 8, uniq % 8
    idx = (n % X + offset[0], (n // X) % Y + offset[1], n // (X * Y) + offset[2])
    u = n + (m & 1) + ((m >> 1) & 1) * X + ((m >> 2) & 1) * X * Y
    ts = tsdf.reshape(-1)
    t0, t1 = ts[n], ts[u]
    s = t0 / (t0 - t1)
    v = f32(voxel)
    verts = np.empty((uniq.size, 3), f32)
    for a, bit in enumerate((1, 2, 4)):
        p0 = f32(origin[a]) + v * idx[a].astype(f32)
        p1 = f32(origin[a]) + v * (idx[a] + ((m & bit) > 0)).astype(f32)
        verts[:, a] = p0 + s * (p1 - p0)
    cols = np.empty((uniq.size, 3), np.uint8)
    cf = color.reshape(3, N)
    for a in range(3):
        ca, cb = cf[a][n], cf[a][u]
        c = np.floor((ca + s * (cb - ca)) + f32(0.5))
        cols[:, a] = np.minimum(f32(255), np.maximum(f32(0), c)).astype(np.uint8)
    return verts, cols, faces


# ------------------------------------------------------------------------------------------------------------------------ soups
def soup(vertices, colors, faces):
    """int64 [F,18]: per face its three (x y z bits, r g b) tuples, rotated to the lexicographically smallest of the three rotations
    (the winding is kept); the faces sorted.  Two meshes are the same set of triangles iff their soups are equal arrays."""
    v = np.ascontiguousarray(vertices, f32).view(np.uint32).astype(np.int64)
    t = np.concatenate([v, np.asarray(colors).astype(np.int64)], 1)[np.asarray(faces, np.int64)]         # [F,3,6]
    F = t.shape[0]
    best = t.reshape(F, 18)
    rows = np.arange(F)
    for r in (1, 2):
        cand = np.roll(t, -r, axis=1).reshape(F, 18)
        diff = cand != best
        first = diff.argmax(1)
        less = diff.any(1) & (cand[rows, first] < best[rows, first])
        best = np.where(less[:, None], cand, best)
    return best[np.lexsort(best.T[::-1])] if F else best
