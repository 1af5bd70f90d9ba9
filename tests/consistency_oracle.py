"""numpy restatement of csrc/consistency.hip (multi-view depth consistency) and the synthetic scenes its tests share.  fp64 throughout,
every operation in the kernel's order (numpy never contracts a product and a sum into an FMA), so the counts and the fp32 averaged depth
are compared bit for bit."""
import numpy as np


def valid(d, depth_max):
    """the kernel's cons_valid on fp32 depths"""
    d = np.asarray(d, np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d.astype(np.float64) > 0.0) & (d.astype(np.float64) <= float(depth_max))


def consistency(depth, K, ref, src, fwd, bwd, depth_max, pix=1.0, rel=0.01, z_min=1e-3):
    """depth fp32 [N,H,W], K fp32 [N,4], ref int [R], src int [R,S] (-1: none), fwd, bwd fp64 [R,S,12] ->
    (support u8 [R,H,W], violation u8 [R,H,W], depth_avg fp32 [R,H,W])"""
    depth = np.asarray(depth, np.float32)
    K = np.asarray(K, np.float32).astype(np.float64)
    ref, src = np.asarray(ref), np.asarray(src)
    fwd, bwd = np.asarray(fwd, np.float64), np.asarray(bwd, np.float64)
    N, H, W = depth.shape
    R, S = src.shape
    depth_max, pix, rel, z_min = float(depth_max), float(pix), float(rel), float(z_min)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    support = np.zeros((R, H, W), np.uint8)
    violation = np.zeros((R, H, W), np.uint8)
    avg = np.zeros((R, H, W), np.float32)
    keep = 1.0 - rel
    with np.errstate(all="ignore"):
        for r in range(R):
            vr = int(ref[r])
            ok_r = valid(depth[vr], depth_max)
            d = np.where(ok_r, depth[vr], np.float32(1)).astype(np.float64)
            fx, fy, cx, cy = K[vr]
            x = (u - cx) * d / fx
            y = (v - cy) * d / fy
            n_sup = np.zeros((H, W), np.int64)
            n_vio = np.zeros((H, W), np.int64)
            acc = d.copy()
            for k in range(S):
                vs_ = int(src[r, k])
                if vs_ < 0 or vs_ >= N:
                    continue
                F, B = fwd[r, k], bwd[r, k]
                X = ((F[0] * x + F[1] * y) + F[2] * d) + F[3]
                Y = ((F[4] * x + F[5] * y) + F[6] * d) + F[7]
                Z = ((F[8] * x + F[9] * y) + F[10] * d) + F[11]
                m = ok_r & (Z > z_min)
                fxs, fys, cxs, cys = K[vs_]
                us = fxs * X / Z + cxs
                vs = fys * Y / Z + cys
                m &= (us >= 0.0) & (us <= float(W - 1)) & (vs >= 0.0) & (vs <= float(H - 1))
                us, vs = np.where(m, us, 0.0), np.where(m, vs, 0.0)
                fx0, fy0 = np.floor(us), np.floor(vs)
                x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
                x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
                ds_ = depth[vs_]
                f00, f01, f10, f11 = ds_[y0, x0], ds_[y0, x1], ds_[y1, x0], ds_[y1, x1]
                m &= valid(f00, depth_max) & valid(f01, depth_max) & valid(f10, depth_max) & valid(f11, depth_max)
                t00, t01, t10, t11 = (np.where(m, f, np.float32(1)).astype(np.float64) for f in (f00, f01, f10, f11))
                vio = m & (Z < t00 * keep) & (Z < t01 * keep) & (Z < t10 * keep) & (Z < t11 * keep)
                n_vio += vio
                m &= ~vio
                ax, ay = us - fx0, vs - fy0
                ds = (t00 * (1.0 - ax) + t01 * ax) * (1.0 - ay) + (t10 * (1.0 - ax) + t11 * ax) * ay
                xs = (us - cxs) * ds / fxs
                ys = (vs - cys) * ds / fys
                X2 = ((B[0] * xs + B[1] * ys) + B[2] * ds) + B[3]
                Y2 = ((B[4] * xs + B[5] * ys) + B[6] * ds) + B[7]
                Z2 = ((B[8] * xs + B[9] * ys) + B[10] * ds) + B[11]
                m &= Z2 > z_min
                du = (fx * X2 / Z2 + cx) - u
                dv = (fy * Y2 / Z2 + cy) - v
                sup = m & (du * du + dv * dv < pix * pix) & (np.abs(Z2 - d) < rel * d)
                n_sup += sup
                acc = np.where(sup, acc + Z2, acc)
            support[r] = np.where(ok_r, n_sup, 0).astype(np.uint8)
            violation[r] = np.where(ok_r, n_vio, 0).astype(np.uint8)
            avg[r] = np.where(ok_r, (acc / (1 + n_sup).astype(np.float64)).astype(np.float32), np.float32(0))
    return support, violation, avg


# ----------------------------------------------------------------------------------------------------------------------- scenes
ROOM = (2.0, 1.5, 2.5)             # half-extents of the box room, centred at the origin


def rot_yaw_pitch(yaw, pitch):
    """camera->world rotation: the camera looks along +z, yaw about y then pitch about x"""
    cy_, sy = np.cos(yaw), np.sin(yaw)
    cp, sp = np.cos(pitch), np.sin(pitch)
    Ry = np.array([[cy_, 0, sy], [0, 1, 0], [-sy, 0, cy_]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    return Ry @ Rx


def room_cameras(n=7):
    """(centres [n,3], camera->world rotations [n,3,3]) of the box-room walk: c_i = (0.12 (i - 3), 0.04 cos i, -0.5 + 0.05 i), yaw
    0.08 (i - 3), pitch 0.03 sin i"""
    i = np.arange(n, dtype=np.float64)
    c = np.stack([0.12 * (i - 3), 0.04 * np.cos(i), -0.5 + 0.05 * i], 1)
    Rm = np.stack([rot_yaw_pitch(0.08 * (k - 3), 0.03 * np.sin(k)) for k in i])
    return c, Rm


def w2c_rows(c, Rm):
    """world->camera rows fp64 [n,12] of centres and camera->world rotations: [R^T | -R^T c]"""
    Rt = Rm.transpose(0, 2, 1)
    t = -np.einsum("nij,nj->ni", Rt, c)
    return np.concatenate([Rt, t[..., None]], 2).reshape(-1, 12)


def room_depth(c, Rm, K, H, W, half=ROOM):
    """analytic z-depth fp32 [n,H,W] of the box's inside seen from centres c with rotations Rm; K [n,4] or [4]"""
    n = len(c)
    K = np.broadcast_to(np.asarray(K, np.float64).reshape(-1, 4), (n, 4))
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.zeros((n, H, W), np.float32)
    half = np.asarray(half, np.float64)
    for b in range(n):
        ray = np.stack([(u - K[b, 2]) / K[b, 0], (v - K[b, 3]) / K[b, 1], np.ones_like(u)], -1) @ Rm[b].T     # world direction per unit z
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(ray > 0, (half - c[b]) / ray, np.where(ray < 0, (-half - c[b]) / ray, np.inf))
        out[b] = t.min(-1).astype(np.float32)
    return out


def box_room(n=7, H=48, W=64, K=(50.0, 50.0, 31.5, 23.5)):
    """(depth fp32 [n,H,W], w2c fp64 [n,12], K fp32 [n,4]) of the box-room walk"""
    c, Rm = room_cameras(n)
    K = np.broadcast_to(np.asarray(K, np.float64).reshape(-1, 4), (n, 4)).astype(np.float32)
    return room_depth(c, Rm, K, H, W), w2c_rows(c, Rm), np.ascontiguousarray(K)


def inject_floaters(depth, share=0.03, seed=0):
    """(depth with `share` of the pixels multiplied by U(0.4, 0.8), the mask of those pixels)"""
    g = np.random.default_rng(seed)
    mask = g.random(depth.shape) < share
    out = depth.copy()
    out[mask] = (depth[mask].astype(np.float64) * g.uniform(0.4, 0.8, int(mask.sum()))).astype(np.float32)
    return out, mask


def plane_pair(H=6, W=20):
    """two views of the plane z = 2, K = (64, 64, 9.5, 2.5), the second camera 0.25 to the right: the disparity is exactly 8 px"""
    depth = np.full((2, H, W), 2.0, np.float32)
    w2c = np.tile(np.eye(4)[:3].reshape(1, 12), (2, 1))
    w2c[1, 3] = -0.25
    K = np.tile(np.array([64.0, 64.0, 9.5, 2.5], np.float32), (2, 1))
    return depth, w2c, K
