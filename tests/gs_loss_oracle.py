"""fp64 references with PER-ELEMENT first-order fp32 error bounds of the loss kernels of csrc/gs.hip (cut3r_ssim_forward / _backward,
cut3r_pixel_loss_forward / _backward, cut3r_refine_loss_forward / _backward) and of the 3-NN (cut3r_knn3_mean_dist2,
cut3r_knn3_grid_mean_dist2, the grid build of csrc/knn_grid.h).  CPU only (numpy, scipy's cKDTree where it is installed); shared by
tests/test_gs_loss_cpu.py and tests/test_gs_loss_gpu.py.  Not collected by pytest.

Every function is written once over the numbers of tests/gs_render_oracle.py (EV: fp64 with a bound, or with f32=True fp32 in the
kernel's order of operations: the restatement) and takes `mutants`, wrong variants of the restatement that the comparison must reject.

Error model beyond EV's.
  * SSIM: the eleven window taps are exact inputs (SS_G restates the fp32 table of the kernel); each tap of the two passes is one fused
    multiply-add, one rounding.  A pass over zeros is exact, so two black images give S = 1 and d_mu1 = 0 exactly.
  * logf: nobody has measured it on the device.  It is MODELLED as one unit in the last place (2 u |log x|), as _pow1 and _sqrt1 of
    tests/gs_train_oracle.py model powf and sqrtf; what the MI355X says about that is in the docstring of tests/test_gs_loss_gpu.py.
  * a sum over pixels goes through a wave tree and one atomic per workgroup: u (6 + workgroups) sum |term| on top of the terms' own bounds.
    The counts (sums[3] of the pixel loss, sums[1] and sums[4] of the refine loss) are sums of ones below 2^24: exact, bound 0.
  * decisions.  d > 0.001f, gt_d > 0.001f, alpha > th and sign(img - gt) are decisions on fp32 inputs (the rounded difference of two
    fp32 numbers has the sign of the exact one): exact, which makes g_img exact.  Two are not: |c| against 1e-12 in the pixel loss's
    backward pass (the forward pass clamps, which is continuous: there the error of |c| is carried through the clamp and nothing is
    ambiguous) and the sign of 1/d - 1/gt_d.  A pixel whose own sign, or one of whose four neighbours' |c|, lies within MARGIN x its error
    of the switch is `ambiguous`.  d bit-equal to gt_d is not: both reciprocals round alike, the difference is exactly 0.
  * 3-NN.  With exact fp32 inputs, dx = fl(x_j - x_i) has a relative error of u, dx^2 of 2 u plus u for the rounding of the square: 3 u
    per term; the terms are non-negative, so the two additions (fused with the squares or not) add u each: every fp32 squared distance
    is within 5 u of the exact one.  The k-th smallest of values each perturbed by a relative eps is within eps of the k-th smallest of
    the exact values, so the three order statistics carry 5 u and no ambiguity rule is needed.  (b0 + b1) + b2 adds 2 u, the division by
    3 one more: the mean is within 8 u of the exact mean.  A duplicate is a neighbour at distance 0; only the point's own INDEX is left out.

The constants K = max(1, 2 RATIO), RATIO = the worst |fp32 restatement - reference| / bound over the cases of tests/test_gs_loss_cpu.py
plus 0.05, rounded up to a decimal (the rule of tests/gs_render_oracle.py):

  group      measured (worst case of)                          RATIO  K     what it covers
  ssim_map   0.185  (3x37x50 exposure)                         0.3   1.0    ssim_map of cut3r_ssim_forward
  d_mu1      0.149  (3x37x50 exposure)                         0.2   1.0    d_mu1
  d_x11      0.185  (3x37x50 exposure)                         0.3   1.0    d_x11
  d_x12      0.382  (1x1x1 black)                              0.5   1.0    d_x12
  ssim_grad  0.242  (3x16x16 exposure)                         0.3   1.0    grad_a of cut3r_ssim_backward
  pix_sums   0.198  (3x40 mixed)                               0.3   1.0    sums[0..3] of cut3r_pixel_loss_forward
  pix_g_d    0.677  (37x50 tiny_c)                             0.8   1.6    grad_depth of cut3r_pixel_loss_backward
  ref_sums   0.137  (16x16 mixed)                              0.2   1.0    sums[0..4] of cut3r_refine_loss_forward
  ref_g_d    0.387  (41x53 mixed)                              0.5   1.0    grad_depth of cut3r_refine_loss_backward
  knn        0.381  (exhaustive P = 32769)                     0.5   1.0    both 3-NN entry points
  The kernels on an MI355X against K x bound: see the docstring of tests/test_gs_loss_gpu.py.
"""
import numpy as np

from tests.gs_render_oracle import EV, F32, F64, MARGIN, U, ratio
from tests.gs_train_oracle import _cross, _normal_parts, _roll, _unary

RATIO = {"ssim_map": 0.3, "d_mu1": 0.2, "d_x11": 0.3, "d_x12": 0.5, "ssim_grad": 0.3, "pix_sums": 0.3, "pix_g_d": 0.8, "ref_sums": 0.2,
         "ref_g_d": 0.5, "knn": 0.5}
K = {name: max(1.0, 2.0 * r) for name, r in RATIO.items()}
MAX_AMBIGUOUS = 0.01

SS_G = np.array([0.00102838, 0.00759876, 0.03600077, 0.10936069, 0.21300553, 0.26601172, 0.21300553, 0.10936069, 0.03600077, 0.00759876,
                 0.00102838], dtype=F32)
SS_T, SS_R = 16, 5
TH_D = F32(0.001)
FLOOR = float(F32(1e-12))
FLT_MAX = F32(3.402823466e38)


def _lift(a, f32):
    """exact inputs: fp32 arrays (fp64 ones keep their values in the reference: the CPU cross-checks feed fp64 maps)"""
    if f32:
        return EV(np.ascontiguousarray(a, dtype=F32))
    v = np.asarray(a).astype(F64)
    return EV(v, np.zeros(v.shape))


def _sl(x, idx):
    return EV(x.v[idx], None if x.e is None else x.e[idx])


def _fma(g, x, acc):
    """fmaf(g, x, acc), g an exact tap: one rounding (fp32 mode: the product of two fp32 numbers is exact in fp64)"""
    if x.e is None:
        return EV((np.float64(g) * x.v.astype(F64) + acc.v.astype(F64)).astype(F32))
    return EV.mk(g * x.v + acc.v, abs(g) * x.e + acc.e)


def _zeros(shape, f32):
    return EV(np.zeros(shape, dtype=F32 if f32 else F64), None if f32 else np.zeros(shape))


# ------------------------------------------------------------------------------------------------------------------ SSIM
def _filter(x, taps, f32, mutants):
    """ss_filter on a whole plane stack [C,H,W]: zero padding, the horizontal pass, then the vertical pass, both as fma chains from 0"""
    C, H, W = x.v.shape
    mode = "edge" if "replicate_pad" in mutants else "constant"
    pad = lambda a: np.pad(a, ((0, 0), (SS_R, SS_R), (SS_R, SS_R + 1)), mode=mode)       # (one spare column for the shifted window)
    p = EV(pad(x.v), None if f32 else pad(np.broadcast_to(x.e, x.v.shape)))
    off = 1 if "window_shift" in mutants else 0
    seam = (np.arange(W) % SS_T != SS_T - 1)[None, None, :]                               # the tile's last halo column feeds its last output column
    acc = _zeros((C, H + 2 * SS_R, W), f32)
    for k in range(11):
        t = _sl(p, (slice(None), slice(None), slice(k + off, k + off + W)))
        if "drop_halo" in mutants and k == 10:
            t = t.where(seam, t.v.dtype.type(0))
        acc = _fma(taps[k], t, acc)
    out = _zeros((C, H, W), f32)
    for k in range(11):
        out = _fma(taps[k], _sl(acc, (slice(None), slice(k, k + H), slice(None))), out)
    return out


def _taps(window, f32):
    return [F32(w) if f32 else F64(w) for w in np.asarray(window)]


def ssim_forward(a, b, C, H, W, window=SS_G, f32=False, mutants=()):
    """cut3r_ssim_forward -> (smap, d_mu1, d_x11, d_x12), EV [C,H,W]"""
    dt = F32 if f32 else F64
    A, B = _lift(np.asarray(a).reshape(C, H, W), f32), _lift(np.asarray(b).reshape(C, H, W), f32)
    taps = _taps(window, f32)
    with np.errstate(all="ignore"):
        mu1, mu2, x11, x22, x12 = (_filter(m, taps, f32, mutants) for m in (A, B, A * A, B * B, A * B))
        s11, s22, s12 = x11 - mu1 * mu1, x22 - mu2 * mu2, x12 - mu1 * mu2
        C1 = dt(F32(0.0001))
        C2 = C1 if "c2_is_c1" in mutants else dt(F32(0.0009))
        A1, A2 = 2.0 * mu1 * mu2 + C1, 2.0 * s12 + C2
        B1, B2 = mu1 * mu1 + mu2 * mu2 + C1, s11 + s22 + C2
        iB = 1.0 / (B1 * B2)
        S = A1 * A2 * iB
        d_mu1 = 2.0 * mu2 * (A2 - A1) * iB - S * (2.0 * mu1 / B1 - 2.0 * mu1 / B2)
        d_x11 = (-S) / B2
        d_x12 = 2.0 * A1 * iB
    return S, d_mu1, d_x11, d_x12


def ssim_backward(a, b, d_mu1, d_x11, d_x12, gscale, C, H, W, window=SS_G, f32=False, mutants=()):
    """cut3r_ssim_backward on GIVEN partial maps -> grad_a EV [C,H,W]"""
    sh = lambda m: _lift(np.asarray(m).reshape(C, H, W), f32)
    A, B = sh(a), sh(b)
    taps = _taps(window, f32)
    gs = _lift(np.asarray(gscale).reshape(1, 1, 1), f32)
    with np.errstate(all="ignore"):
        f = [_filter(sh(m), taps, f32, mutants) for m in (d_mu1, d_x11, d_x12)]
        inner = f[0] + (f[1] if "no_2a" in mutants else 2.0 * A * f[1]) + B * f[2]
        return gs * inner


# ------------------------------------------------------------------------------------------------------------------ sums
def _groups(n):
    return (n + 255) // 256


def _sum(term, f32, exact=False):
    """one of the kernels' sums over pixels: (value, bound)"""
    dt = F32 if f32 else F64
    tot = term.v.sum(dtype=dt)
    if f32 or exact:
        return tot, 0.0
    return tot, np.broadcast_to(term.e, term.v.shape).sum() + U * (6.0 + _groups(term.v.size)) * np.abs(term.v).sum()


def _sums(terms, exact, f32):
    vs, es = zip(*[_sum(t, f32, k in exact) for k, t in enumerate(terms)])
    return EV(np.array(vs, dtype=F32 if f32 else F64), None if f32 else np.array(es, dtype=F64))


def _l1(img, gt, f32):
    """v = 0; v += |gt_c - img_c| for the three channels"""
    I, G = _lift(img, f32), _lift(gt, f32)
    d = [(_sl(G, c) - _sl(I, c)).abs() for c in range(3)]
    return (d[0] + d[1]) + d[2]


def _sign_grad(img, gt, c):
    """c sign(img - gt) as the fp32 numbers the kernels store"""
    e = np.asarray(img, dtype=F32) - np.asarray(gt, dtype=F32)
    return np.where(e > 0, F32(c), np.where(e < 0, -F32(c), F32(0))).astype(F32)


def _valid(depth, gt_depth, mutants=()):
    d, g = np.asarray(depth, dtype=F32), np.asarray(gt_depth, dtype=F32)
    return (g >= TH_D) & (d >= TH_D) if "ge_threshold" in mutants else (g > TH_D) & (d > TH_D)


def _safe(x, mask, f32):
    return _lift(np.where(mask, np.asarray(x, dtype=F32), F32(1.0)), f32)


# ------------------------------------------------------------------------------------------------------------------ pixel loss
def pixel_loss_forward(img, gt, depth, gt_depth, gt_normal, H, W, cam, f32=False, mutants=()):
    """cut3r_pixel_loss_forward -> sums EV [4]"""
    dt = F32 if f32 else F64
    sh = lambda a, c=None: np.asarray(a, dtype=F32).reshape((H, W) if c is None else (c, H, W))
    depth, gt_depth, gn = sh(depth), sh(gt_depth), sh(gt_normal, 3)
    mask = _valid(depth, gt_depth, mutants)
    zero = _zeros((H, W), f32)
    with np.errstate(all="ignore"):
        v0 = _l1(sh(img, 3), sh(gt, 3), f32)
        v1 = (1.0 / _safe(depth, mask, f32) - 1.0 / _safe(gt_depth, mask, f32)).abs().where(mask, zero)
        p = _normal_parts(depth, H, W, cam, f32, "border_normal" in mutants)
        ln = p["len"]                                                          # fmaxf is continuous: |c|'s error goes through unless clearly below
        ln = EV(np.maximum(ln.v, dt(FLOOR)), None if f32 else np.where(ln.v < FLOOR - MARGIN * ln.e, 0.0, ln.e))
        il = 1.0 / ln
        dot = (p["c"][0] * _lift(gn[0], f32) + p["c"][1] * _lift(gn[1], f32) + p["c"][2] * _lift(gn[2], f32)) * il
        v2 = (1.0 - dot.where(p["inner"], zero)).where(mask, zero)
    v3 = _lift(mask.astype(F32), f32)
    return _sums([v0, v1, v2, v3], (3,), f32)


def pixel_loss_backward(img, gt, depth, gt_depth, gt_normal, H, W, cam, coef, f32=False, mutants=()):
    """cut3r_pixel_loss_backward -> (g_img exact fp32 [3,H,W], g_d EV [H,W], ambiguous [H,W])"""
    dt = F32 if f32 else F64
    sh = lambda a, c=None: np.asarray(a, dtype=F32).reshape((H, W) if c is None else (c, H, W))
    depth, gt_depth, gn = sh(depth), sh(gt_depth), sh(gt_normal, 3)
    c_rgb, c_dep, c_nrm = (F32(c) for c in coef)
    g_img = _sign_grad(sh(img, 3), sh(gt, 3), c_rgb)
    mask = _valid(depth, gt_depth, mutants)
    zero = _zeros((H, W), f32)
    with np.errstate(all="ignore"):
        dp, gp = _safe(depth, mask, f32), _safe(gt_depth, mask, f32)
        e = 1.0 / dp - 1.0 / gp
        sg = np.where(e.v > 0, 1.0, np.where(e.v < 0, -1.0, 0.0))
        g = (_lift((sg * dt(c_dep)).astype(dt), f32) * ((-1.0) / (dp * dp))).where(mask, zero)
        amb = np.zeros((H, W), bool) if f32 else mask & (depth != gt_depth) & (np.abs(e.v) < MARGIN * e.e)
        p = _normal_parts(depth, H, W, cam, f32, "border_normal" in mutants)
        gate = p["inner"] & (mask if "q_gate_dropped" not in mutants else True)
        ok = gate & (p["len"].v > FLOOR)
        if not f32:
            near = gate & (np.abs(p["len"].v - FLOOR) < MARGIN * p["len"].e)
        il2 = 1.0 / EV(np.where(ok, p["len"].v, dt(1.0)), p["len"].e)
        nq = [p["c"][i] * il2 for i in range(3)]
        gq = [_lift(gn[i], f32) for i in range(3)]
        ng = nq[0] * gq[0] + nq[1] * gq[1] + nq[2] * gq[2]
        h = [(-(gq[i] - nq[i] * ng)) * il2 for i in range(3)]
        for k, (sx, sy) in enumerate(((-1, 0), (1, 0), (0, -1), (0, 1))):    # q = p + (sx, sy): bring q's quantities to p
            at = lambda a: _roll(a, -sy, -sx)
            okq = np.roll(ok, (-sy, -sx), (0, 1))
            dc = _cross(p["ray"], [at(a) for a in p["dy"]]) if k < 2 else _cross([at(a) for a in p["dx"]], p["ray"])
            hq = [at(a) for a in h]
            sgn = 1.0 if k in (0, 2) or (k == 1 and "ex_sign_flipped" in mutants) else -1.0
            term = ((hq[0] * dc[0] + hq[1] * dc[1] + hq[2] * dc[2]) * dt(c_nrm * F32(sgn))).where(okq, zero)
            g = EV.where(g + term, okq, g)
            if not f32:
                amb |= np.roll(near, (-sy, -sx), (0, 1))
    return g_img, g, amb


# ------------------------------------------------------------------------------------------------------------------ refine loss
def _log1(x):
    """logf MODELLED as one unit in the last place (fp32 mode: the correctly rounded value)"""
    return _unary(x, np.log, lambda t: 1.0 / np.abs(t), 1.0)


def refine_loss_forward(img, gt, depth, gt_depth, alpha, alpha_th, H, W, f32=False, mutants=()):
    """cut3r_refine_loss_forward -> sums EV [5]"""
    sh = lambda a, c=None: np.asarray(a, dtype=F32).reshape((H, W) if c is None else (c, H, W))
    depth, gt_depth = sh(depth), sh(gt_depth)
    a = sh(alpha) > F32(alpha_th)
    m = a & _valid(depth, gt_depth)
    zero = _zeros((H, W), f32)
    with np.errstate(all="ignore"):
        v0 = _l1(sh(img, 3), sh(gt, 3), f32).where(a, zero)
        diff = _log1(_safe(depth, m, f32)) - _log1(_safe(gt_depth, m, f32))
        v2, v3 = diff.where(m, zero), (diff * diff).where(m, zero)
    return _sums([v0, _lift(a.astype(F32), f32), v2, v3, _lift(m.astype(F32), f32)], (1, 4), f32)


def refine_loss_backward(img, gt, depth, gt_depth, alpha, alpha_th, H, W, coef, f32=False, mutants=()):
    """cut3r_refine_loss_backward -> (g_img exact fp32 [3,H,W], g_d EV [H,W])"""
    dt = F32 if f32 else F64
    sh = lambda a, c=None: np.asarray(a, dtype=F32).reshape((H, W) if c is None else (c, H, W))
    depth, gt_depth = sh(depth), sh(gt_depth)
    c_rgb, c_var, mean = (F32(c) for c in coef)
    a = sh(alpha) > F32(alpha_th)
    g_img = np.where(a[None], _sign_grad(sh(img, 3), sh(gt, 3), c_rgb), F32(0)).astype(F32)
    m = _valid(depth, gt_depth) & (a if "alpha_ignored" not in mutants else True)
    with np.errstate(all="ignore"):
        dp = _safe(depth, m, f32)
        diff = _log1(dp) - _log1(_safe(gt_depth, m, f32))
        if "mean_not_subtracted" not in mutants:
            diff = diff - dt(mean)
        g_d = ((dt(c_var) * dt(2.0)) * diff / dp).where(m, _zeros((H, W), f32))
    return g_img, g_d


# ------------------------------------------------------------------------------------------------------------------ 3-NN
def knn3_chunks(P):
    """cut3r_knn3_chunks restated"""
    if P < 4:
        return 0
    blocks = (P + 255) // 256
    return max(1, min((2048 + blocks - 1) // blocks, (P + 2047) // 2048))


def knn3_chunk_size(P):
    c = knn3_chunks(P)
    return ((P + c - 1) // c + 255) // 256 * 256


def knn3_grid_G(P):
    return min(160, max(8, int(np.ceil(np.sqrt(float(P)) / 2.0))))


def _knn4(p):
    """indices of the four nearest points of each point, itself included, in fp64"""
    try:
        from scipy.spatial import cKDTree
        return cKDTree(p).query(p, k=4)[1]
    except ImportError:
        idx = np.empty((len(p), 4), dtype=np.int64)
        for i0 in range(0, len(p), 512):
            d = ((p[None, :, :] - p[i0:i0 + 512, None, :]) ** 2).sum(-1)
            idx[i0:i0 + 512] = np.argpartition(d, 3, axis=1)[:, :4]
        return idx


def knn3_mean_dist2(points):
    """mean of the three smallest squared distances to OTHER INDICES, EV [P] with the 8 u bound of the docstring.  The four nearest of a
    point, itself included, hold one distance 0 for the point itself (or four zeros of duplicates): dropping the smallest of the four
    leaves out the point's own index and nothing else."""
    p = np.asarray(points, dtype=F32).astype(F64).reshape(-1, 3)
    idx = _knn4(p)
    d2 = np.sort(((p[idx] - p[:, None, :]) ** 2).sum(-1), axis=1)
    mean = (d2[:, 1] + d2[:, 2] + d2[:, 3]) / 3.0
    return EV(mean, 8.0 * U * mean)


def knn3_dense64(points):
    """the same quantity by exhaustive search in fp64 (the cross-check of knn3_mean_dist2)"""
    p = np.asarray(points, dtype=F32).astype(F64).reshape(-1, 3)
    out = np.empty(len(p))
    for i0 in range(0, len(p), 512):
        d = ((p[None, :, :] - p[i0:i0 + 512, None, :]) ** 2).sum(-1)
        r = np.arange(d.shape[0])
        d[r, i0 + r] = np.inf
        out[i0:i0 + 512] = np.sort(np.partition(d, 2, axis=1)[:, :3], axis=1).sum(1) / 3.0
    return out


def _d32(p, q):
    """fp32 squared distances of the candidates p [.., 3] to the queries q [.., 3]: dx dx + dy dy + dz dz"""
    dx, dy, dz = p[..., 0] - q[..., 0], p[..., 1] - q[..., 1], p[..., 2] - q[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def _best3(d):
    """(b0 + b1 + b2) / 3.f of the three smallest of each row"""
    if d.shape[1] < 3:
        d = np.concatenate([d, np.full((d.shape[0], 3 - d.shape[1]), FLT_MAX, dtype=F32)], 1)
    b = np.sort(np.partition(d, 2, axis=1)[:, :3], axis=1)
    with np.errstate(over="ignore"):
        return ((b[:, 0] + b[:, 1]) + b[:, 2]) / F32(3.0), b[:, 2]


def knn3_exhaustive_f32(points, mutants=()):
    """knn3_kernel + knn3_merge_kernel in fp32: the best three of every chunk, merged, are the best three of all candidates below
    chunks x chunk.  Above 5000 points the candidates are the sixteen nearest in fp64 instead of all (the same values: a point outside them
    is further than thirteen that are inside)."""
    p = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
    P = len(p)
    chunks = knn3_chunks(P) - ("last_chunk_dropped" in mutants)
    limit = min(P, chunks * knn3_chunk_size(P))
    out = np.empty(P, dtype=F32)
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    if P > 5000 and cKDTree is not None and not mutants:
        p64 = p.astype(F64)
        idx = cKDTree(p64).query(p64, k=16)[1]
        d = _d32(p[idx], p[:, None, :])
        d[idx == np.arange(P)[:, None]] = FLT_MAX
        return _best3(d)[0]
    for i0 in range(0, P, 512):
        d = _d32(p[None, :limit, :], p[i0:i0 + 512, None, :])
        r = np.arange(d.shape[0])
        own = i0 + r < limit
        if "dup_by_distance" in mutants:
            d[d == 0] = FLT_MAX
        elif "self_included" not in mutants:
            d[r[own], (i0 + r)[own]] = FLT_MAX
        out[i0:i0 + 512] = _best3(d)[0]
    return out


def knn_grid_header(points):
    """the header of knn_header_kernel (fp32; the moments summed in numpy's order: they only steer the speed) -> lo [3], cs, g [3]"""
    p = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
    P, G = len(p), knn3_grid_G(len(p))
    bb_lo, bb_hi = p.min(0), p.max(0)
    d = p - p[0]

    def box(sel):
        n = F32(max(int(sel.sum()), 1))
        mean_d = d[sel].sum(0, dtype=F32) / n
        var = np.maximum((d[sel] * d[sel]).sum(0, dtype=F32) / n - mean_d * mean_d, F32(0))
        mu, sg = p[0] + mean_d, np.sqrt(var)
        lo, hi = np.maximum(bb_lo, mu - F32(3) * sg), np.minimum(bb_hi, mu + F32(3) * sg)
        bad = ~(hi >= lo)
        return np.where(bad, bb_lo, lo).astype(F32), np.where(bad, bb_hi, hi).astype(F32)
    lo, hi = box(np.ones(P, bool))
    lo, hi = box(((p >= lo) & (p <= hi)).all(1))
    ext = hi - lo
    cs = F32(ext.max() / F32(G))
    if not cs > 0:
        cs = F32(1.0)
    inv = F32(1.0) / cs
    g = np.minimum(G + 1, (ext * inv).astype(np.int64) + 1)
    return lo, cs, inv, g


def knn3_grid_f32(points, mutants=()):
    """knn_query_kernel in fp32 on the grid of knn_grid_header: shells of growing Chebyshev radius R until the third best is within
    (R cs)^2; a query outside the box scans the list.  -> (means [P], queries outside the box)"""
    p = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
    P = len(p)
    lo, cs, inv, g = knn_grid_header(p)
    cell = np.clip(((p - lo) * inv).astype(np.int64), 0, g - 1)
    outside = ((p < lo) | (p > lo + g.astype(F32) * cs)).any(1)
    out = np.empty(P, dtype=F32)
    early = 1 if "shell_early" in mutants else 0
    for t in range(P):
        d = _d32(p, p[t])
        d[t] = FLT_MAX
        if outside[t]:
            out[t] = _best3(d[None])[0][0]
            continue
        cheb = np.abs(cell - cell[t]).max(1)
        for R in range(int(g.max()) + 1):
            m, b2 = _best3(d[cheb <= R][None])
            reach = F32(R + early) * cs
            if b2[0] <= reach * reach:
                break
        out[t] = m[0]
    return out, outside


def within(got, ref, name, keep=None):
    """(largest |got - ref| / (K bound), elements beyond)"""
    return ratio(got, ref.v, K[name] * ref.e, keep)


# ------------------------------------------------------------------------------------------------------------------ cases
SSIM_SHAPES = ((1, 1, 1), (1, 1, 40), (1, 5, 5), (2, 11, 11), (3, 16, 16), (1, 17, 33), (3, 37, 50))
SSIM_CONTENTS = ("random", "same", "black", "one_zero", "flat_bright", "exposure")
SSIM_IMPULSES = ((0, 0), (15, 15), (16, 16), (16, 32))                       # on the 17 x 33 image: corners of the first tile, the one-pixel tiles


def ssim_case(content, C, H, W):
    r = np.random.default_rng(C * H * W + len(content))
    a = r.random((C, H, W))
    if content == "random":
        b = np.clip(a + 0.2 * r.normal(size=a.shape), 0, 1)
    elif content == "same":
        b = a
    elif content == "black":
        a, b = np.zeros_like(a), np.zeros_like(a)
    elif content == "one_zero":
        a, b = np.ones_like(a), np.zeros_like(a)
    elif content == "flat_bright":                                           # E[a^2] - mu1^2 cancels against C2 = 9e-4
        a, b = 0.9 + 1e-3 * r.normal(size=a.shape), 0.9 + 1e-3 * r.normal(size=a.shape)
    elif content == "exposure":                                              # exposure-compensated renders leave [0, 1]
        a, b = 4.0 * a, 4.0 * r.random((C, H, W))
    else:
        raise KeyError(content)
    return a.astype(F32), b.astype(F32)


def ssim_impulse_case(y, x):
    """(1, 17, 33): one bright pixel on a dim image: a shifted tap or a bad tile seam shows as a displaced copy of the window"""
    a = np.full((1, 17, 33), 0.125, dtype=F32)
    a[0, y, x] = 1.0
    return a, (F32(0.5) * a + F32(0.1)).astype(F32)


def ssim_cases():
    """(name, C, H, W, a, b)"""
    for C, H, W in SSIM_SHAPES:
        for content in SSIM_CONTENTS:
            yield (f"{C}x{H}x{W} {content}", C, H, W) + ssim_case(content, C, H, W)
    for y, x in SSIM_IMPULSES:
        yield (f"1x17x33 impulse ({y},{x})", 1, 17, 33) + ssim_impulse_case(y, x)


def ssim_cotangent(C, H, W):
    return np.array([0.37 / (C * H * W)], dtype=F32)


PIXEL_SHAPES = ((3, 3), (3, 40), (17, 16), (37, 50))
PIXEL_COEF = (3.1e-4, 0.021, 0.0043)
# per shape: gt-invalid patch, render-invalid patch, the valid pixel enclosed by invalid ones, threshold pixels (depth = 0.001f, then its
# successor), the d == gt_d patch, the d = nextafter(gt_d) patch (at most 1 % of the image: its sign is ambiguous)
_PIXEL_MARKS = {
    (3, 3): dict(gt0=((0, 1), (0, 1)), d0=((2, 3), (2, 3)), th=((0, 2), (2, 0)), same=((1, 2), (1, 2))),
    (3, 40): dict(gt0=((1, 2), (5, 6)), d0=((0, 2), (9, 10)), hole=(1, 20), th=((1, 30), (1, 31)), same=((0, 3), (12, 15)), near=((1, 2), (25, 26))),
    (17, 16): dict(gt0=((3, 5), (4, 6)), d0=((8, 10), (9, 11)), hole=(13, 3), th=((12, 7), (12, 8)), same=((13, 16), (8, 11)), near=((6, 7), (1, 3))),
    (37, 50): dict(gt0=((3, 6), (4, 9)), d0=((10, 12), (20, 25)), hole=(21, 31), th=((25, 5), (25, 6), (25, 7), (25, 8)), same=((30, 33), (10, 14)),
                   near=((30, 33), (20, 24))),
}


def pixel_case(H, W, kind="mixed"):
    """-> dict(img, gt, depth, gt_depth, gn, cam).  `mixed`: an off-centre principal point, the marks of _PIXEL_MARKS; every pixel of
    rows / columns 1 and W - 2 outside the marks is valid.  `tiny_c` (37 x 50): fx = fy = 2500 and depths of 0.0011 (|c| = 7.7e-13, clearly
    below 1e-12) on the left half, 0.0014 (1.25e-12, clearly above) on the right"""
    r = np.random.default_rng(H * W + len(kind))
    ys, xs = np.meshgrid(np.arange(H, dtype=F64), np.arange(W, dtype=F64), indexing="ij")
    img, gt = r.random((3, H, W)).astype(F32), r.random((3, H, W)).astype(F32)
    img[:, 0, 0] = gt[:, 0, 0]                                               # sign(0)
    gn = r.normal(size=(3, H, W))
    gn = (gn / np.linalg.norm(gn, axis=0)).astype(F32)
    succ = np.nextafter(TH_D, F32(1))
    if kind == "tiny_c":
        cam = (2500.0, 2500.0, 0.37 * W, 0.61 * H)
        depth = (np.where(xs < W // 2, 0.0011, 0.0014) * (1 + 1e-3 * np.sin(xs / 5 + ys / 7))).astype(F32)
        gt_depth = (depth * F32(1.01)).astype(F32)
        gt_depth[5:8, 5:9] = TH_D
        return dict(img=img, gt=gt, depth=depth, gt_depth=gt_depth, gn=gn, cam=cam)
    cam = (60.0, 62.0, 0.37 * W, 0.61 * H)
    gt_depth = (2.0 + 0.3 * np.sin(xs / 7) + 0.2 * np.cos(ys / 5)).astype(F32)
    depth = np.maximum(gt_depth + 0.05 * r.normal(size=(H, W)), 0.01).astype(F32)
    mk = _PIXEL_MARKS[(H, W)]
    box = lambda k: (slice(*mk[k][0]), slice(*mk[k][1]))
    if "hole" in mk:
        y, x = mk["hole"]
        keep = gt_depth[y, x]
        gt_depth[max(y - 1, 0):y + 2, x - 1:x + 2] = 0
        gt_depth[y, x] = keep
    gt_depth[box("gt0")] = 0
    depth[box("d0")] = 0
    for k, (y, x) in enumerate(mk["th"]):
        (depth if k < max(2, len(mk["th"]) // 2) else gt_depth)[y, x] = TH_D if k % 2 == 0 else succ
    depth[box("same")] = gt_depth[box("same")]
    if "near" in mk:
        depth[box("near")] = np.nextafter(gt_depth[box("near")], F32(10))
    return dict(img=img, gt=gt, depth=depth, gt_depth=gt_depth, gn=gn, cam=cam)


def pixel_cases():
    for H, W in PIXEL_SHAPES:
        yield f"{H}x{W} mixed", H, W, pixel_case(H, W)
    yield "37x50 tiny_c", 37, 50, pixel_case(37, 50, "tiny_c")


REFINE_SHAPES = ((1, 1), (16, 16), (17, 16), (41, 53))
REFINE_CONTENTS = ("below", "no_depth", "mixed")
REFINE_TH = 0.4
REFINE_COEF = (2.7e-4, 0.013, -0.021)


def refine_case(H, W, content):
    """`below`: no covered pixel; `no_depth`: covered pixels, none with both depths valid; `mixed`: both kinds and invalid patches"""
    r = np.random.default_rng(H * W + len(content))
    img, gt = r.random((3, H, W)).astype(F32), r.random((3, H, W)).astype(F32)
    gt_depth = (1.5 + r.random((H, W))).astype(F32)
    depth = np.maximum(gt_depth * (1 + 0.1 * r.normal(size=(H, W))), 0.01).astype(F32)
    alpha = r.random((H, W)).astype(F32)
    if content == "below":
        alpha = (alpha * F32(REFINE_TH)).astype(F32)
        alpha.flat[0] = F32(REFINE_TH)                                       # equal is not above
    elif content == "no_depth":
        alpha = (F32(0.5) + F32(0.5) * alpha).astype(F32)
        depth[::2], gt_depth[1::2] = 0, TH_D
    else:
        alpha.flat[0] = 0.9
        if H > 4:
            img[:, 1, 1] = gt[:, 1, 1]
            gt_depth[2:5, 3:9], depth[8:11, 10:14] = 0, 0
            depth[5, 5], gt_depth[5, 5], alpha[5, 5] = TH_D, 2.0, 0.9
            depth[5, 6], gt_depth[5, 6], alpha[5, 6] = np.nextafter(TH_D, F32(1)), 2.0, 0.9
            depth[6, 5], gt_depth[6, 5], alpha[6, 5] = 1.0, 1.0, 0.9          # log 1 - log 1
    return dict(img=img, gt=gt, depth=depth, gt_depth=gt_depth, alpha=alpha)


def refine_cases():
    for H, W in REFINE_SHAPES:
        for content in REFINE_CONTENTS:
            yield f"{H}x{W} {content}", H, W, refine_case(H, W, content)


KNN_SIZES = (4, 5, 255, 256, 257, 2049, 16385, 32769)
KNN_GRID = ("random4", "identical4", "random9", "identical", "collinear", "two_sites", "clusters", "plane", "offset", "cauchy", "outliers")
KNN_SHARED = ("random9", "two_sites", "clusters", "outliers")                # grid cases that the exhaustive kernel runs too


def knn_surface(P, seed=11):
    """a noisy surface with one exact duplicate pair"""
    r = np.random.default_rng(seed + P)
    xy = r.random((P, 2))
    z = 0.2 * np.sin(3 * xy[:, 0]) * np.cos(2 * xy[:, 1]) + 0.002 * r.normal(size=P)
    p = np.concatenate([xy, z[:, None]], 1).astype(F32)
    p[P - 1] = p[0]
    return p


def knn_grid_case(name):
    r = np.random.default_rng(len(name) + 23)
    if name == "random4":
        p = r.normal(size=(4, 3))
    elif name == "identical4":                                               # cs = 1
        p = np.tile(r.normal(size=(1, 3)), (4, 1))
    elif name == "random9":
        p = r.normal(size=(9, 3))
    elif name == "identical":
        p = np.tile(r.normal(size=(1, 3)), (257, 1))
    elif name == "collinear":
        p = np.array([0.3, -0.2, 1.0]) + r.random(300)[:, None] * np.array([1.0, 0.0, 0.0])     # two empty axes
    elif name == "two_sites":
        p = np.repeat(np.array([[0.1, 0.2, 0.3], [1.1, -0.7, 0.9]]), 150, axis=0)
    elif name == "clusters":
        c = r.random((20, 3))
        p = np.repeat(c, 250, axis=0) + 1e-3 * r.normal(size=(5000, 3))
        p[1::250] = p[0::250]
    elif name == "plane":
        p = np.concatenate([r.random((5000, 2)), np.full((5000, 1), 0.75)], 1)
    elif name == "offset":
        return (knn_surface(5000, 31).astype(F64) + np.array([1e4, -1e4, 1e4])).astype(F32)
    elif name == "cauchy":
        p = r.standard_cauchy(size=(3000, 3))
    elif name == "outliers":
        p = knn_surface(2005, 37).astype(F64)
        p[1000:1005] = 100.0 * r.normal(size=(5, 3))
    else:
        raise KeyError(name)
    return np.ascontiguousarray(p, dtype=F32)
