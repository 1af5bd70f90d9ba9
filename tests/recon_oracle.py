"""numpy restatement of csrc/recon.hip (surface sampling, exact 1-NN with its tie rule, point-to-point ICP) and the test meshes of the
reconstruction-metric tests.  fp32 where the kernels are fp32, fp64 where they are fp64: the samples and the NN results match bit for bit."""
import math

import numpy as np

M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def splitmix64(z):
    z = np.asarray(z, np.uint64) + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def rand_u64(seed, stream, counters):
    """h(seed, stream, c) = sm(sm(sm(seed) ^ stream) ^ c) for an array of counters"""
    with np.errstate(over="ignore"):
        key = splitmix64(splitmix64(np.array([seed % 2 ** 64], np.uint64)) ^ np.uint64(stream % 2 ** 64))
        return splitmix64(key ^ np.asarray(counters, np.uint64))


def face_areas(v, f):
    v = np.asarray(v, np.float32)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    e1, e2 = b - a, c - a
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return np.float32(0.5) * np.sqrt((cx * cx + cy * cy) + cz * cz)


def sample(v, f, cdf, n, seed=0, stream=0):
    """the kernel's samples [n,3] fp32, given its fp64 CDF"""
    v = np.asarray(v, np.float32)
    i = np.arange(n, dtype=np.uint64)
    h0 = rand_u64(seed, stream, np.uint64(3) * i)
    h1 = rand_u64(seed, stream, np.uint64(3) * i + np.uint64(1))
    h2 = rand_u64(seed, stream, np.uint64(3) * i + np.uint64(2))
    u0 = (h0 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    target = u0 * cdf[-1]
    face = np.minimum(np.searchsorted(cdf, target, side="right"), len(cdf) - 1)
    u1 = (h1 >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    u2 = (h2 >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    flip = (u1 + u2) > np.float32(1)
    u1 = np.where(flip, np.float32(1) - u1, u1)
    u2 = np.where(flip, np.float32(1) - u2, u2)
    a, b, c = v[f[face, 0]], v[f[face, 1]], v[f[face, 2]]
    return (a + u1[:, None] * (b - a)) + u2[:, None] * (c - a)


def xform32(T, q):
    """fp32 (((T0 x + T1 y) + T2 z) + T3) per row, as the kernel loads a query"""
    q = np.asarray(q, np.float32)
    if T is None:
        return q.copy()
    T = np.asarray(T, np.float64).reshape(-1)[:12].astype(np.float32).reshape(3, 4)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1)


def nn(ref, query, max_dist=None, T=None, chunk=1024):
    """fp32 brute force: (dist2 [Q] fp32, idx [Q] int32), ties to the smallest reference index, idx -1 / +inf beyond max_dist"""
    r = np.asarray(ref, np.float32)
    q = xform32(T, query)
    lim = np.float32(np.inf) if max_dist is None else np.float32(max_dist) * np.float32(max_dist)
    d2 = np.empty(len(q), np.float32)
    idx = np.empty(len(q), np.int32)
    for a in range(0, len(q), chunk):
        qq = q[a:a + chunk]
        dx = r[None, :, 0] - qq[:, None, 0]
        dy = r[None, :, 1] - qq[:, None, 1]
        dz = r[None, :, 2] - qq[:, None, 2]
        d = dx * dx + dy * dy + dz * dz
        d = np.where(d <= lim, d, np.float32(np.inf))
        j = np.argmin(d, 1)
        best = d[np.arange(len(qq)), j]
        ok = np.isfinite(best)
        d2[a:a + chunk] = np.where(ok, best, np.float32(np.inf))
        idx[a:a + chunk] = np.where(ok, j, -1)
    return d2, idx


def rigid_fit(s, d):
    """eval_ate.umeyama (with_scale=False) on fp64 point pairs -> 4x4"""
    mu_s, mu_d = s.mean(0), d.mean(0)
    cov = (d - mu_d).T @ (s - mu_s) / len(s)
    U, _, Vt = np.linalg.svd(cov)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1
    R = U @ S @ Vt
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = mu_d - R @ mu_s
    return T


def icp(src, dst, threshold, init=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6, nn_fn=None):
    """Open3D's point-to-point loop in fp64 (the correspondences by `nn_fn`, default the fp32 brute force with fp32(T) applied on load)
    -> (T, fitness, rmse, iterations)"""
    nn_fn = nn_fn or (lambda T: nn(dst, src, threshold, T))
    dst64 = np.asarray(dst, np.float64)
    T = np.eye(4) if init is None else np.asarray(init, np.float64).copy()

    def evaluate(T):
        d2, idx = nn_fn(T)
        ok = idx >= 0
        n = int(ok.sum())
        s = xform32(T, src)[ok].astype(np.float64)
        return (s, dst64[idx[ok]]), n / len(src), (math.sqrt(d2[ok].astype(np.float64).sum() / n) if n else 0.0)

    pairs, fit, rmse = evaluate(T)
    it = 0
    for i in range(max_iteration):
        T = (rigid_fit(*pairs) if len(pairs[0]) else np.eye(4)) @ T
        pf, pr = fit, rmse
        pairs, fit, rmse = evaluate(T)
        it = i + 1
        if abs(pf - fit) < relative_fitness and abs(pr - rmse) < relative_rmse:
            break
    return T, fit, rmse, it


def rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K


# ------------------------------------------------------------------------------------------------------------------- test meshes
def icosphere(subdiv=3, radius=1.0, center=(0.0, 0.0, 0.0)):
    """(verts fp32 [V,3], faces int32 [F,3]) of a subdivided icosahedron, outward winding"""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
         (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdiv):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    verts = np.asarray(v) * radius + np.asarray(center, np.float64)
    return verts.astype(np.float32), np.asarray(f, np.int32)


def grid_quad(origin, e1, e2, n1, n2):
    """the parallelogram origin + [0,1] e1 + [0,1] e2 tessellated into n1 x n2 cells of two triangles"""
    o, e1, e2 = (np.asarray(x, np.float64) for x in (origin, e1, e2))
    i, j = np.meshgrid(np.arange(n1 + 1), np.arange(n2 + 1), indexing="ij")
    v = o + (i[..., None] / n1) * e1 + (j[..., None] / n2) * e2
    idx = (i * (n2 + 1) + j)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    f = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])
    return v.reshape(-1, 3), f


def box_room(size=(4.0, 3.0, 2.5), step=0.02, origin=(0.0, 0.0, 0.0)):
    """(verts fp32, faces int32) of the six walls of an axis-aligned box, each tessellated at about `step`"""
    sx, sy, sz = size
    o = np.asarray(origin, np.float64)
    X, Y, Z = np.array([sx, 0, 0]), np.array([0, sy, 0]), np.array([0, 0, sz])
    walls = [(o, Y, X), (o + Z, X, Y), (o, X, Z), (o + Y, Z, X), (o, Z, Y), (o + X, Y, Z)]
    vs, fs, n = [], [], 0
    for org, a, b in walls:
        v, f = grid_quad(org, a, b, max(1, round(np.linalg.norm(a) / step)), max(1, round(np.linalg.norm(b) / step)))
        vs.append(v)
        fs.append(f + n)
        n += len(v)
    return np.concatenate(vs).astype(np.float32), np.concatenate(fs).astype(np.int32)
