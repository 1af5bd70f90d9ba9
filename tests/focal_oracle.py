"""numpy restatement of csrc/calib.hip (focal length from self-view pointmaps): the per-pixel arithmetic in fp32, every operation rounded on
its own; the Weiszfeld sums in fp64 in the kernel's order (16 contiguous pixel ranges per view, 256 strided running sums per range, a halving
tree, the 16 range sums in ascending order); the median from a plain sort of the non-NaN votes.  No final clip (self_calib applies it)."""
import numpy as np

G, T = 16, 256
F = np.float32


def _uv(H, W, pp):
    """u, v fp32 [B,HW]: pixel (row, col) minus the view's principal point"""
    pp = np.asarray(pp, F).reshape(-1, 2)
    col = np.tile(np.arange(W, dtype=F), H)[None]
    row = np.repeat(np.arange(H, dtype=F), W)[None]
    return col - pp[:, 0:1], row - pp[:, 1:2]


def _keep(B, HW, conf, conf_min):
    if conf is None:
        return np.ones((B, HW), bool)
    return ~(np.asarray(conf, F).reshape(B, HW) < F(conf_min))


def ordered_sum(vals):
    """vals fp64 [B,HW] (0 where a pixel takes no part) -> fp64 [B] in the kernel's order"""
    B, HW = vals.shape
    chunk = (HW + G - 1) // G
    K = (chunk + T - 1) // T
    pad = np.zeros((B, G * K * T), np.float64).reshape(B, G, K * T)
    for g in range(G):
        lo, hi = g * chunk, min(HW, (g + 1) * chunk)
        if hi > lo:
            pad[:, g, :hi - lo] = vals[:, lo:hi]
    pad = pad.reshape(B, G, K, T)
    acc = np.zeros((B, G, T), np.float64)
    for k in range(K):                                 # thread t: its pixels in increasing order
        acc = acc + pad[:, :, k]
    o = T // 2
    while o > 0:                                       # s[t] += s[t + o]
        acc = acc[..., :o] + acc[..., o:2 * o]
        o //= 2
    part = acc[..., 0]
    tot = np.zeros(B, np.float64)
    for g in range(G):
        tot = tot + part[:, g]
    return tot


def _ratio(A, Bs):
    with np.errstate(all="ignore"):
        return np.where(Bs == 0.0, np.nan, A / np.where(Bs == 0.0, 1.0, Bs)).astype(F)


def weiszfeld(pts, pp, iters=10, conf=None, conf_min=None):
    pts = np.asarray(pts, F)
    B, H, W, _ = pts.shape
    HW = H * W
    u, v = _uv(H, W, pp)
    keep = _keep(B, HW, conf, conf_min)
    x, y, z = (pts.reshape(B, HW, 3)[..., k] for k in range(3))
    with np.errstate(all="ignore"):
        xz, yz = x / z, y / z
        xz = np.where(np.isfinite(xz), xz, F(0))
        yz = np.where(np.isfinite(yz), yz, F(0))
        a = (xz * u).astype(F) + (yz * v).astype(F)
        b = (xz * xz).astype(F) + (yz * yz).astype(F)
        f = _ratio(ordered_sum(np.where(keep, a.astype(np.float64), 0.0)), ordered_sum(np.where(keep, b.astype(np.float64), 0.0)))
        for _ in range(iters):
            fk = f.reshape(B, 1)
            du = u - (fk * xz).astype(F)
            dv = v - (fk * yz).astype(F)
            dis = np.sqrt((du * du).astype(F) + (dv * dv).astype(F))
            w = F(1) / np.fmax(dis, F(1e-8))
            wa, wb = (w * a).astype(F), (w * b).astype(F)
            f = _ratio(ordered_sum(np.where(keep, wa.astype(np.float64), 0.0)), ordered_sum(np.where(keep, wb.astype(np.float64), 0.0)))
    assert f.dtype == F
    return f


def votes(pts, pp, conf=None, conf_min=None):
    """the non-NaN votes of every view, ascending: list of fp32 arrays"""
    pts = np.asarray(pts, F)
    B, H, W, _ = pts.shape
    HW = H * W
    u, v = _uv(H, W, pp)
    keep = _keep(B, HW, conf, conf_min)
    x, y, z = (pts.reshape(B, HW, 3)[..., k] for k in range(3))
    with np.errstate(all="ignore"):
        fx = (u * z).astype(F) / x
        fy = (v * z).astype(F) / y
    out = []
    for i in range(B):
        al = np.concatenate([fx[i][keep[i]], fy[i][keep[i]]])
        out.append(np.sort(al[~np.isnan(al)]))
    return out


def median(pts, pp, conf=None, conf_min=None):
    res = [s[(len(s) - 1) // 2] if len(s) else F(np.nan) for s in votes(pts, pp, conf, conf_min)]
    return np.asarray(res, F)
