"""numpy restatement of csrc/raster.hip (the mesh depth rasteriser, the depth-L1 sums, check_proj / points_in_view, vertex visibility) and of
the host side of the 2-D metric (view sampling), plus the analytic depths the tests compare with.  fp32 where the kernels are fp32, fp64 where they are fp64: the
depth and face-id images match bit for bit.  The oracle visits every (pixel, triangle) pair and applies the rule's candidate clause as a mask: no culling of its own."""
import numpy as np

from tests.recon_oracle import rand_u64, xform32

F32 = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def w2c12(w2c):
    """[B,12] fp32 from [B,12] / [B,3,4] / [B,4,4]"""
    w = np.asarray(w2c)
    return np.ascontiguousarray(w.reshape(len(w), -1)[:, :12].astype(F32))


def rays(K, H, W):
    """rx [W], ry [H] fp32: (float(j) - cx) / fx, (float(i) - cy) / fy"""
    fx, fy, cx, cy = (F32(v) for v in K)
    return (np.arange(W, dtype=F32) - cx) / fx, (np.arange(H, dtype=F32) - cy) / fy


def _cross(p, q):
    return np.stack([p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2], p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]], 1)


def _candidates(p, faces, K):
    """fp32 bounds (lo_u, hi_u, lo_v, hi_v) [F] of the pixels a triangle may hit: nothing when its three z are <= 0, the padded box of its
    projected vertices when they are > 0, everything otherwise"""
    fx, fy, cx, cy = K
    z = p[:, 2][faces]
    front, back = (z > 0).all(1), (z <= 0).all(1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u = (fx * (p[:, 0] / p[:, 2]) + cx)[faces]
        w = (fy * (p[:, 1] / p[:, 2]) + cy)[faces]
        lo_u, hi_u = np.floor(u.min(1)) - F32(1), np.ceil(u.max(1)) + F32(1)
        lo_v, hi_v = np.floor(w.min(1)) - F32(1), np.ceil(w.max(1)) + F32(1)
    inf = F32(np.inf)
    lo = lambda x: np.where(back, inf, np.where(front, x, -inf)).astype(F32)
    hi = lambda x: np.where(back, -inf, np.where(front, x, inf)).astype(F32)
    return lo(lo_u), hi(hi_u), lo(lo_v), hi(hi_v)


def render(verts, faces, w2c, K, H, W, z_near=0.0, z_far=20.0, budget=1 << 22):
    """(depth [B,H,W] fp32, face_id [B,H,W] int32) by the pixel rule of csrc/raster.hip: camera space and rays in fp32, the cross products,
    edge values and det / den in fp64, z rounded to fp32"""
    verts, faces, w2c = np.asarray(verts, F32), np.asarray(faces), w2c12(w2c)
    K = np.broadcast_to(np.asarray(K, F32), (len(w2c), 4))
    zn, zf = F32(z_near), F32(z_far)
    depth = np.zeros((len(w2c), H, W), F32)
    fid = np.full((len(w2c), H, W), -1, np.int32)
    for v in range(len(w2c)):
        p32 = xform32(w2c[v], verts)
        lo_u, hi_u, lo_v, hi_v = _candidates(p32, faces, K[v])
        p = p32.astype(np.float64)                                   # fp32 camera space, fp64 from here on
        a, b, c = p[faces[:, 0]], p[faces[:, 1]], p[faces[:, 2]]
        n0, n1, n2 = _cross(b, c), _cross(c, a), _cross(a, b)
        det = (a[:, 0] * n0[:, 0] + a[:, 1] * n0[:, 1]) + a[:, 2] * n0[:, 2]
        rx, ry = rays(K[v], H, W)
        RX, RY = np.tile(rx, H)[None].astype(np.float64), np.repeat(ry, W)[None].astype(np.float64)
        JF, IF = np.tile(np.arange(W, dtype=F32), H)[None], np.repeat(np.arange(H, dtype=F32), W)[None]
        best = np.full(H * W, EMPTY, np.uint64)
        step = max(1, budget // (H * W))
        for s in range(0, len(faces), step):
            e = [(RX * n[s:s + step, 0, None] + RY * n[s:s + step, 1, None]) + n[s:s + step, 2, None] for n in (n0, n1, n2)]
            hit = ((e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0)) | ((e[0] <= 0) & (e[1] <= 0) & (e[2] <= 0))
            den = (e[0] + e[1]) + e[2]
            hit &= den != 0
            q = slice(s, s + step)
            hit &= (JF >= lo_u[q, None]) & (JF <= hi_u[q, None]) & (IF >= lo_v[q, None]) & (IF <= hi_v[q, None])
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                z = (det[s:s + step, None] / den).astype(F32)
            hit &= (z > zn) & (z <= zf)
            face = np.arange(s, s + len(z), dtype=np.uint64)[:, None]
            key = np.where(hit, (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | face, EMPTY)
            best = np.minimum(best, key.min(0))
        got = best != EMPTY
        depth[v] = np.where(got, (best >> np.uint64(32)).astype(np.uint32).view(F32), F32(0)).reshape(H, W)
        fid[v] = np.where(got, (best & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32).reshape(H, W)
    return depth, fid


def depth_l1(gt, ours):
    """fp64 [B,2]: per view the number of pixels with ours > 0 and the sum of |gt - ours| over them"""
    m = ours > 0
    d = np.abs(gt.astype(np.float64) - ours.astype(np.float64)) * m
    return np.stack([m.reshape(len(m), -1).sum(1).astype(np.float64), d.reshape(len(d), -1).sum(1)], 1)


def points_in_view(points, w2c, K, H, W, edge=10.0):
    """int [B]: the points with 0 <= z', edge < u < W - edge, edge < v < H - edge; z' = z - 1e-5, u = (fx x + cx z) / z', all fp32"""
    w2c = w2c12(w2c)
    K = np.broadcast_to(np.asarray(K, F32), (len(w2c), 4))
    edge, Wf, Hf = F32(edge), F32(W), F32(H)
    out = np.zeros(len(w2c), np.int64)
    for v in range(len(w2c)):
        c = xform32(w2c[v], points)
        fx, fy, cx, cy = K[v]
        zz = c[:, 2] - F32(1e-5)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            u, w = (fx * c[:, 0] + cx * c[:, 2]) / zz, (fy * c[:, 1] + cy * c[:, 2]) / zz
        out[v] = np.count_nonzero((F32(0) <= zz) & (u < Wf - edge) & (u > edge) & (w < Hf - edge) & (w > edge))
    return out


def check_proj(points, W, H, fx, fy, cx, cy, c2w):
    """does the camera c2w (OpenCV axes) see one of the points inside the image shrunk by 10 pixels"""
    return bool(points_in_view(points, np.linalg.inv(np.asarray(c2w, np.float64))[None, :3], [fx, fy, cx, cy], H, W, 10.0)[0] > 0)


def vertex_visible(verts, depth, w2c, K, eps=0.03, z_far=20.0):
    w2c = w2c12(w2c)
    K = np.broadcast_to(np.asarray(K, F32), (len(w2c), 4))
    _, H, W = depth.shape
    seen = np.zeros(len(verts), bool)
    for v in range(len(w2c)):
        c = xform32(w2c[v], verts)
        fx, fy, cx, cy = K[v]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            u, w = np.floor((fx * (c[:, 0] / c[:, 2]) + cx) + F32(0.5)), np.floor((fy * (c[:, 1] / c[:, 2]) + cy) + F32(0.5))
        ok = (c[:, 2] > 0) & (c[:, 2] <= F32(z_far)) & (u >= 0) & (u <= W - 1) & (w >= 0) & (w <= H - 1)
        d = depth[v][np.where(ok, w, 0).astype(np.int64), np.where(ok, u, 0).astype(np.int64)]
        seen |= ok & ((d == 0) | (c[:, 2] <= d + F32(eps)))
    return seen


# ------------------------------------------------------------------------------------------------------------------ view sampling
def get_cam_position(verts):
    """(extents [3], transform [4,4]) of the box the cameras are drawn from: the axis-aligned box of the vertices shrunk to 0.3 on its
    shortest axis and 0.7 on the other two, its centre raised by 0.4 along world z"""
    v = np.asarray(verts, np.float64)
    lo, hi = v.min(0), v.max(0)
    ext = hi - lo
    fac = np.full(3, 0.7)
    fac[np.argmin(ext)] = 0.3
    T = np.eye(4)
    T[:3, 3] = 0.5 * (lo + hi)
    T[2, 3] += 0.4
    return ext * fac, T


def uniform(seed, view, attempt, component):
    """the 53-bit uniform in [0, 1) keyed by (seed, view, try, component)"""
    return float(rand_u64(seed, view, [8 * attempt + component])[0] >> np.uint64(11)) * 2.0 ** -53


def viewmatrix(z, up, pos):
    n = lambda x: x / np.linalg.norm(x)
    v2 = n(np.asarray(z, np.float64))
    v0 = n(np.cross(up, v2))
    v1 = n(np.cross(v2, v0))
    m = np.eye(4)
    m[:3] = np.stack([v0, v1, v2, np.asarray(pos, np.float64)], 1)
    return m


def candidate(extents, transform, seed, view, attempt):
    u = np.array([uniform(seed, view, attempt, k) for k in range(6)])
    pos = np.asarray(transform, np.float64)[:3, :3] @ ((u[:3] - 0.5) * np.asarray(extents, np.float64)) + np.asarray(transform)[:3, 3]
    target = np.array([round(-10000.0 + 20000.0 * x, 2) for x in u[3:]])
    return viewmatrix(target - pos, np.array([0.0, 0.0, -1.0]), pos)


def sample_views(extents, transform, n, unseen=None, seed=0, max_tries=1000, W=500, H=500, focal=300.0, stats=None):
    out = np.zeros((n, 4, 4))
    for v in range(n):
        for attempt in range(max_tries + 1):
            if attempt == max_tries:
                raise RuntimeError(f"view {v}: {max_tries} candidates in a row see the unseen region")
            c2w = candidate(extents, transform, seed, v, attempt)
            if stats is not None:
                stats["candidates"] = stats.get("candidates", 0) + 1
            if unseen is None or not check_proj(unseen, W, H, focal, focal, W / 2.0 - 0.5, H / 2.0 - 0.5, c2w):
                break
            if stats is not None:
                stats["redrawn"] = stats.get("redrawn", 0) + 1
        out[v] = c2w
    return out


# ------------------------------------------------------------------------------------------------------------------ analytic scenes
def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """w2c [4,4] fp64 of an OpenCV camera at `eye` looking at `target`"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = -R @ eye
    return M


def box_depth(w2c, K, H, W, lo, hi):
    """fp64 [H,W] depth (camera z) of the inside of the axis-aligned box [lo, hi] seen from a camera inside it; w2c the fp32 matrix the
    renderer gets, read exactly"""
    T = np.asarray(w2c12(np.asarray(w2c)[None])[0], np.float64).reshape(3, 4)
    R, t = T[:, :3], T[:, 3]
    eye = -R.T @ t
    fx, fy, cx, cy = (float(F32(v)) for v in K)
    j, i = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d = np.stack([(j - cx) / fx, (i - cy) / fy, np.ones_like(j)], -1) @ R          # world direction per unit camera z (R orthonormal)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(d > 0, (np.asarray(hi) - eye) / d, np.where(d < 0, (np.asarray(lo) - eye) / d, np.inf))
    return s.min(-1)
