"""fp64 evaluations and PER-ELEMENT error bounds of the small kernels every window runs through: LayerNorm / adaLN, patch im2col, column
mean, bilinear x2 upsample, the DPT output stage (dpt_final, postprocess_pts, postprocess_pose), the fp16-weight GEMV and the ConvTranspose
pixel shuffle.  CPU only (numpy fp64, torch for erf); shared by tests/test_elementwise_cpu.py and tests/test_elementwise_gpu.py.  Not
collected by pytest.

Every reference works on the kernel's STORED inputs: fp32 inputs as they are, fp16 inputs as their exact values, constants of the kernel
(1e-8f, 1e-6f, 1e-12f) as the fp32 numbers they are.  Every bound is a first-order rounding model with u = 2^-24 (fp32 unit round-off),
h = 2^-11 (fp16) and s = 2^-25 (half the spacing of fp16 subnormals); an fp16 store costs h |y| + s.

  LayerNorm     y = (x - mu) rstd g + b [then y (1 + sc) + sh].  The mean is a sum of C terms, so it carries u A with A = mean |x| (the
                error of a sum scales with sum |x_j|, not with |sum x_j|: on zero-mean rows |mu| would understate it several times over);
                x - mu then carries that plus u |x - mu| <= u (|x| + A), scaled by rstd |g|; the variance's relative error and the final
                multiply-adds cost u (|y| + |b|):
                   B = k u [ |g| rstd (|x| + A) + |y| + |b| ],   adaLN: B |1 + sc| + k u (|y0| (1 + |sc|) + |y| + |sh|).
  column mean   a sum of M fp32 terms:   B = k u sum_m |x_mc| / M.
  upsample      y = sum_j w_j v_j over four fp16 taps with fp32 weights from the fp32 source coordinate sy = fl(fl((H-1)/(2H-1)) oy):
                B = h |y| + s + k u sum_j w_j |v_j| + u oy |dy/dsy| + u ox |dy/dsx|   (|d sy| <= 2 u sy ~ u oy; at a knot the steeper of the
                two adjacent segments).
  dpt_final     a_o = sum_k x_k w_ok + b_o with delta_o = k u (sum_k |x_k w_ok| + |b_o|), pushed through the fp64 Jacobian J of the
                activation; the activation's own arithmetic costs k u (|out| + R) where R is what the rounding of an intermediate is
                amplified to: for points the norm d (relative error ~u) reaches the output through g(d) = expm1(d) / max(d, 1e-8):
                R = |a_i| d |g'(d)|; for rgb the intermediates are of size 1 while the output may be near 0: R = 1.
                B = |J| delta + k u (|out| + R).  The Jacobian is that of the side of the max(d, 1e-8) kink the fp64 value falls on.
                The PER-LANE kernel (Cin / 8 does not divide 64) sums in one chain that starts from the bias: see dpt_final64(chain=True).
  postprocess   the same with delta = 0.
  GEMV          Y = act(sum_k a_k w_k + bias) + res, a_k = fp16(x_k) or fp16(silu(x_k)).  The kernel's silu uses the fast __expf: its fp32
                value is within tau = (|x| + 4) u of silu(x) (the argument reduction of __expf costs u |x|), so an activation within tau of an
                fp16 rounding tie may round either way.  gemv_interval returns [lo, hi]: the dot product with every such activation rounded
                to the side that lowers / raises it, widened by B = k u (sum_k |a_k w_k| + |bias| + |pre-activation| + |res| + |Y|) (products
                of two fp16 numbers are exact in fp32: accumulation error only); GELU maps the interval by its derivative at the midpoint
                plus the second-order remainder (|gelu''| < 1), and its own arithmetic 0.5 x (1 + erf(x / sqrt 2)) -- the exact GELU as torch
                states it in fp32 -- rounds 1 + erf, a number of size 1, so it costs k u (|gelu| + |x| / 2): for x < -3 the result is
                far smaller than |x| / 2 and the error is absolute, not relative (measured on the GPU: gelu(-5.2) = -1.6e-7 for -1.1e-7).
  ConvTranspose B = h |y| + s + k u (sum |a w| + |bias|)  (the GEMM bound of tests/gemm_forms_child.py, per element).

The constants k are MEASURED, not chosen: the fp32 numpy restatement of each operation (`*_f32`, the kernel's operation order as far as
numpy can state it) is compared with the fp64 reference over every input kind and width of the GPU test, RATIO below is its largest
(error - the part of the bound without k) / (the part with k, at k = 1), rounded up to one decimal, and k = 2 RATIO: the kernels sum in a
wave tree where numpy sums pairwise or in sequence.  tests/test_elementwise_cpu.py repeats the measurement, asserts it stays <= RATIO and
that each named mutant falls outside the bound at the full k.  (Where the measurement gave less than 1 the RATIO is 1: a bound below one
rounding of the result would not be a bound.)

  operation             restatement, largest ratio at k = 1 (257 rows per kind and width for LayerNorm)                  RATIO     k
  LayerNorm (two-pass)  typical 2.10, massive 3.13, near-constant 1.30, constant 0.00, tiny 1.69, large 1.86              3.2    6.4
                        one-pass mutant E[x^2] - mu^2, in the same units: massive 8.1 .. 30 (outside the k = 6.4 bound at
                        every width), near-constant NaN; typical 1.0 .. 2.5, tiny 0.5 .. 1.7, large 1.0 .. 3.9 (inside: on
                        rows whose mean does not dwarf their spread the one-pass form is not worse than a rounding model allows)
  column mean           2.03 (M = 769, columns of |x| ~ 1e3 that cancel)                                                 2.1    4.2
  upsample (u terms)    0.00: every error is inside the fp16 rounding of the result                                      1.0    2.0
  points                dpt_final 1.96, postprocess_pts 3.39, postprocess_pose 1.59                                      3.4    6.8
  confidence            dpt_final 2.05, postprocess_pts 1.74                                                             2.1    4.2
  rgb                   2.58                                                                                             2.6    5.2
  GEMV (widening)       0.50                                                                                             1.0    2.0
  ConvTranspose (u)     0.48 (Cin = 192)                                                                                 1.0    2.0
  dpt_final per-lane    chain restatement: 0.23 (Cin = 24), 0.20 (40), 0.05 (1024) of the constant-free chain bound; the
                        same outputs are 0.52, 0.60 and 2.86 of the tree bound above, which is why that bound is not used there

Measured on an MI355X against these bounds (largest error / bound of tests/test_elementwise_gpu.py): LayerNorm fp32 0.41 (fast kernels
0.40), column mean 0.48 (batched 0.56), dpt_final coalesced points 0.26 / confidence 0.37 / rgb 0.47, per-lane 0.38 / 0.37 / 0.47,
postprocess_pts 0.30 / 0.27, postprocess_pose 0.23.  The fp16 outputs (LayerNorm fp16 0.997, upsample 0.999, ConvTranspose 0.994) and the
GEMV interval (0.999) reach their bound by construction: round-to-nearest errs by up to half a spacing, and an activation on a tie sits at
one end of its interval.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
H16 = 2.0 ** -11
S16 = 2.0 ** -25
F32 = np.float32

RATIO = {"layernorm": 3.2, "colmean": 2.1, "upsample": 1.0, "pts": 3.4, "conf": 2.1, "rgb": 2.6, "gemv": 1.0, "convt": 1.0}
K = {name: 2.0 * r for name, r in RATIO.items()}


def f64(a):
    return np.asarray(a, dtype=np.float64)


def ratio(got, ref, bound):
    """largest |got - ref| / bound, its index, and the number of elements beyond the bound; a NaN in `got` gives inf"""
    err = np.abs(f64(got) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    r = np.where(np.isfinite(r), r, np.inf)
    idx = np.unravel_index(int(np.argmax(r)), r.shape) if r.size else ()
    return (float(r[idx]) if r.size else 0.0), idx, int((r > 1.0).sum())


def describe(name, got, ref, bound):
    """the worst ratio of `got` against ref +- bound and a message for a failing assertion: worst index, both values, violations"""
    r, idx, nbad = ratio(got, ref, bound)
    msg = (f"{name}: worst error/bound {r:.3g} at {tuple(int(i) for i in idx)}: got {float(f64(got)[idx]):.9g} ref {float(ref[idx]):.9g} "
           f"bound {float(np.broadcast_to(bound, ref.shape)[idx]):.3g}; {nbad}/{ref.size} elements beyond the bound")
    return r, msg


def fp16_ulp(y):
    """spacing of fp16 numbers at |y| (2^-24 in the subnormal range)"""
    a = np.maximum(np.abs(f64(y)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(a)) - 10)


# ------------------------------------------------------------------------------------------------ LayerNorm
LN_KINDS = ("typical", "massive", "near_constant", "constant", "tiny", "large")
LN_GENERIC_C = (4, 48, 252, 256, 260, 516, 1280, 2048)
LN_FAST_C = (768, 1024, 1536)


def ln_rows(kind, M, C, seed):
    """fp32 rows [M, C] of one kind (see LN_KINDS)"""
    g = np.random.default_rng(seed)
    n = g.standard_normal((M, C))
    if kind == "typical":
        x = 3.0 * n + 0.5
    elif kind == "massive":                 # the residual stream late in the decoder: a per-row mean of ~3 sigma, one channel at |x| ~ 300
        x = n + 3.0 * g.standard_normal((M, 1))
        x[::3, min(7, C - 1)] += 300.0
    elif kind == "near_constant":
        x = 100.0 + 1e-3 * n
    elif kind == "constant":                # 100 C <= 2^24: every partial sum is exact, so the mean is exact and the output is beta
        x = np.full((M, C), 100.0)
    elif kind == "tiny":                    # eps dominates the variance
        x = 1e-4 * n
    elif kind == "large":
        x = 1e4 * n
    else:
        raise ValueError(kind)
    return x.astype(F32)


def ln_params(C, seed, adaln):
    g = np.random.default_rng(1000 + seed)
    gamma, beta = (1.0 + 0.3 * g.standard_normal(C)).astype(F32), (0.2 * g.standard_normal(C)).astype(F32)
    sc, sh = ((0.3 * g.standard_normal(C)).astype(F32), g.standard_normal(C).astype(F32)) if adaln else (None, None)
    return gamma, beta, sc, sh


def layernorm64(x, gamma, beta, eps, sc=None, sh=None, k=K["layernorm"], fp16=False):
    """-> (y fp64, per-element bound)"""
    x, g, b = f64(x), f64(gamma), f64(beta)
    eps = float(F32(eps))
    mu = x.mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(((x - mu) ** 2).mean(1, keepdims=True) + eps)
    y = (x - mu) * rstd * g + b
    bound = k * U * (np.abs(g) * rstd * (np.abs(x) + np.abs(x).mean(1, keepdims=True)) + np.abs(y) + np.abs(b))
    if sc is not None:
        sc, sh = f64(sc), f64(sh)
        y0, y = y, y * (1.0 + sc) + sh
        bound = bound * np.abs(1.0 + sc) + k * U * (np.abs(y0) * (1.0 + np.abs(sc)) + np.abs(y) + np.abs(sh))
    if fp16:
        bound = bound + H16 * np.abs(y) + S16
    return y, bound


def layernorm_f32(x, gamma, beta, eps, sc=None, sh=None, one_pass=False):
    """the kernel's order in fp32 numpy: mean, then the variance of x - mean (one_pass: the mutant E[x^2] - mean^2)"""
    x = np.asarray(x, F32)
    C = F32(x.shape[1])
    mean = x.sum(1, keepdims=True, dtype=F32) / C
    d = x - mean
    with np.errstate(invalid="ignore"):
        var = ((x * x).sum(1, keepdims=True, dtype=F32) / C - mean * mean) if one_pass else (d * d).sum(1, keepdims=True, dtype=F32) / C
        rstd = F32(1.0) / np.sqrt(var + F32(eps), dtype=F32)
    y = d * rstd * gamma + beta
    if sc is not None:
        y = y * (F32(1.0) + sc) + sh
    return y.astype(F32)


# ------------------------------------------------------------------------------------------------ im2col
def im2col_index(B, C, Hh, W, P, swap=False):
    """flat source index into img [B, C, H, W] of every element of out [(b, py, px), (c, iy, ix)] (swap: the mutant with iy and ix exchanged)"""
    nh, nw = Hh // P, W // P
    b, py, px, c, iy, ix = np.meshgrid(np.arange(B), np.arange(nh), np.arange(nw), np.arange(C), np.arange(P), np.arange(P), indexing="ij")
    if swap:
        iy, ix = ix, iy
    return ((((b * C + c) * Hh + py * P + iy) * W) + px * P + ix).reshape(B * nh * nw, C * P * P)


def im2col64(img, P, swap=False):
    """fp64 patches of an fp32 image, or of a uint8 image normalised as (p / 255 - 0.5) / 0.5"""
    img = np.asarray(img)
    v = (f64(img) / 255.0 - 0.5) / 0.5 if img.dtype == np.uint8 else f64(img)
    return v.reshape(-1)[im2col_index(*img.shape, P, swap)]


def im2col_u8_f32(img, P):
    """the kernel's fp32 arithmetic on bytes, rounded to fp16"""
    v = ((np.asarray(img).astype(F32) / F32(255.0) - F32(0.5)) / F32(0.5)).astype(np.float16)
    return v.reshape(-1)[im2col_index(*img.shape, P)]


# ------------------------------------------------------------------------------------------------ column mean
def colmean64(x, k=K["colmean"]):
    x = f64(x)
    return x.mean(-2), k * U * np.abs(x).sum(-2) / x.shape[-2]


def colmean_f32(x, drop_tail=False):
    """the kernel's order: 4 row groups (rows rg, rg + 4, ...), each with 4 accumulators over strides of 16 rows and a tail into the first,
    combined as (s0 + s1) + (s2 + s3), then the groups in order (drop_tail: the mutant without the tail loop)"""
    x = np.asarray(x, F32)
    M, C = x.shape
    part = []
    for rg in range(4):
        s = [np.zeros(C, F32) for _ in range(4)]
        m = rg
        while m + 12 < M:
            for j in range(4):
                s[j] = s[j] + x[m + 4 * j]
            m += 16
        while m < M and not drop_tail:
            s[0] = s[0] + x[m]
            m += 4
        part.append((s[0] + s[1]) + (s[2] + s[3]))
    return (((part[0] + part[1]) + part[2]) + part[3]) / F32(M)


# ------------------------------------------------------------------------------------------------ bilinear x2, align_corners
def _axis(n):
    """source coordinates of the 2n outputs along an axis of n inputs: (i0, i1, frac fp64 exact to rounding, knot flag)"""
    o = np.arange(2 * n)
    s = o * (n - 1) / (2 * n - 1) if n > 1 else np.zeros(2 * n)
    i0 = np.minimum(np.floor(s).astype(np.int64), n - 1)
    knot = (o * (n - 1)) % (2 * n - 1) == 0
    s[knot] = np.round(s[knot])
    i0[knot] = s[knot].astype(np.int64)
    return i0, np.minimum(i0 + 1, n - 1), s - i0, knot


def upsample64(x, k=K["upsample"]):
    """x fp16 [B, H, W, C] -> (y fp64 [B, 2H, 2W, C], bound)"""
    v = f64(x)
    B, Hh, W, C = v.shape
    y0, y1, ly, ky = _axis(Hh)
    x0, x1, lx, kx = _axis(W)
    ly_, lx_ = ly[None, :, None, None], lx[None, None, :, None]
    rows = lambda a, i: a[:, i]
    cols = lambda a, i: a[:, :, i]
    top = cols(rows(v, y0), x0) * (1 - lx_) + cols(rows(v, y0), x1) * lx_
    bot = cols(rows(v, y1), x0) * (1 - lx_) + cols(rows(v, y1), x1) * lx_
    y = top * (1 - ly_) + bot * ly_
    a = np.abs(v)
    mag = (cols(rows(a, y0), x0) * (1 - lx_) + cols(rows(a, y0), x1) * lx_) * (1 - ly_) + (cols(rows(a, y1), x0) * (1 - lx_) + cols(rows(a, y1), x1) * lx_) * ly_
    # slopes along each axis; at a knot (a source coordinate that is an integer in exact arithmetic) fp32 may land in the segment before it
    gy = np.abs(bot - top)
    ym = np.maximum(y0 - 1, 0)
    prev = cols(rows(v, ym), x0) * (1 - lx_) + cols(rows(v, ym), x1) * lx_
    gy = np.where(ky[None, :, None, None], np.maximum(gy, np.abs(top - prev)), gy)
    left = cols(rows(v, y0), x0) * (1 - ly_) + cols(rows(v, y1), x0) * ly_
    right = cols(rows(v, y0), x1) * (1 - ly_) + cols(rows(v, y1), x1) * ly_
    gx = np.abs(right - left)
    xm = np.maximum(x0 - 1, 0)
    prevx = cols(rows(v, y0), xm) * (1 - ly_) + cols(rows(v, y1), xm) * ly_
    gx = np.where(kx[None, None, :, None], np.maximum(gx, np.abs(left - prevx)), gx)
    oy, ox = np.arange(2 * Hh)[None, :, None, None], np.arange(2 * W)[None, None, :, None]
    bound = H16 * np.abs(y) + S16 + k * U * mag + U * oy * gy + U * ox * gx
    return y, bound


def upsample_f32(x):
    """the kernel's fp32 arithmetic, rounded to fp16"""
    v = np.asarray(x).astype(F32)
    B, Hh, W, C = v.shape

    def axis(n):
        r = F32(n - 1) / F32(2 * n - 1) if 2 * n > 1 else F32(0)
        s = (r * np.arange(2 * n, dtype=F32)).astype(F32)
        i0 = s.astype(np.int64)
        i1 = i0 + (i0 < n - 1)
        l = (s - i0.astype(F32)).astype(F32)
        return i0, i1, l, (F32(1) - l).astype(F32)
    y0, y1, ly, hy = axis(Hh)
    x0, x1, lx, hx = axis(W)
    ly, hy, lx, hx = ly[None, :, None, None], hy[None, :, None, None], lx[None, None, :, None], hx[None, None, :, None]
    r0, r1 = v[:, y0], v[:, y1]
    return (hy * (hx * r0[:, :, x0] + lx * r0[:, :, x1]) + ly * (hx * r1[:, :, x0] + lx * r1[:, :, x1])).astype(np.float16)


# ------------------------------------------------------------------------------------------------ DPT output stage
CLAMP = float(F32(1e-8))
RGB_EPS = F32(1e-6)


def _g(d):
    """g(d) = expm1(d) / max(d, 1e-8f) and g'(d) on the side of the kink d falls on"""
    big = d >= CLAMP
    dc = np.where(big, d, CLAMP)
    g = np.expm1(d) / dc
    with np.errstate(divide="ignore", invalid="ignore"):
        gp = np.where(big, (np.exp(d) * d - np.expm1(d)) / np.where(d > 0, d * d, 1.0), np.exp(d) / CLAMP)
    # series near 0 for the unclamped side (d >= 1e-8 > 0 there): (e^d d - expm1 d) / d^2 = 1/2 + d/3 + ...
    gp = np.where(big & (d < 1e-4), 0.5 + d / 3.0, gp)
    return g, gp


def points64(a, delta, k=K["pts"]):
    """a fp64 [P, 3] = xyz, delta [P, 3] its error bound -> (pts = xyz g(|xyz|), bound)"""
    d = np.sqrt((a * a).sum(1, keepdims=True))
    g, gp = _g(d)
    out = a * g
    with np.errstate(divide="ignore", invalid="ignore"):
        n = np.where(d > 0, a / np.where(d > 0, d, 1.0), 0.0)              # unit vector (0 at the origin, where a_i a_j / d -> 0)
    # |J| delta with J_ij = delta_ij g + a_i n_j g'
    jd = np.abs(g) * delta + np.abs(a) * np.abs(gp) * (np.abs(n) * delta).sum(1, keepdims=True)
    return out, jd + k * U * (np.abs(out) + np.abs(a) * d * np.abs(gp))


def conf64(c, delta, k=K["conf"]):
    out = 1.0 + np.exp(c)
    return out, np.exp(c) * delta + k * U * np.abs(out)


def rgb64(a, delta, k=K["rgb"]):
    e = float(RGB_EPS)
    c1 = float(F32(1.0) - F32(2.0) * RGB_EPS)
    s = 1.0 / (1.0 + np.exp(-a))
    out = ((s * c1 + e) - 0.5) * 2.0
    return out, 2.0 * c1 * s * (1.0 - s) * delta + k * U * (np.abs(out) + 1.0)


def _k3(k):
    return (K["pts"], K["conf"], K["rgb"]) if k is None else (k, k, k)


def dpt_final64(x, w, b, mode, k=None, bias_per_lane=0, chain=False):
    """x fp16 [P, Cin], w fp32 [nout, Cin], b fp32 [nout] -> mode 0: (pts, pts bound, conf, conf bound); mode 1: (rgb, bound, None, None).
    k: one constant for every output (the measurement), None: each output's own.  The dot product's delta_o carries the k of the output
    it feeds.  bias_per_lane = L: the mutant whose L lanes per pixel each add the bias before the lane sum.
    chain: the PER-LANE kernel's dot product, one fmaf chain of Cin links that STARTS from the bias: s_0 = b, s_j = fl(s_j-1 + x_j w_j).  Every
    link rounds the running sum, so to first order the error is sum_j eps_j s_j, |eps_j| <= u: delta_o = u sum_j |s_j|, a bound without a
    fitted constant.  (The k u (sum |x w| + |b|) of the tree-summing kernels does not hold here: a bias that dominates the sum is rounded
    Cin times, which the GPU measured as 3.4 times that bound at Cin = 1024.  Summation order, not a defect; the recorded bits of
    tests/golden/dpt_final_bits.npz pin this order.)"""
    x, w, b = f64(x), f64(w), f64(b)
    kp, kc, kr = _k3(k)
    a = x @ w.T + b * (bias_per_lane if bias_per_lane else 1)
    if chain:                               # u sum_j |s_j| over the Cin links, constant-free (k = 0 still switches it off for the measurement)
        delta = np.stack([U * np.abs(b[o] + np.cumsum(x * w[o], 1)).sum(1) for o in range(w.shape[0])], 1)
        one = 1.0 if k is None else min(k, 1.0)
        if mode == 1:
            return (*rgb64(a, one * delta, kr), None, None)
        return (*points64(a[:, :3], one * delta[:, :3], kp), *conf64(a[:, 3], one * delta[:, 3], kc))
    delta = U * (np.abs(x) @ np.abs(w).T + np.abs(b))
    if mode == 1:
        return (*rgb64(a, kr * delta, kr), None, None)
    return (*points64(a[:, :3], kp * delta[:, :3], kp), *conf64(a[:, 3], kc * delta[:, 3], kc))


def dpt_final_f32(x, w, b, mode, chain=False):
    x, w, b = np.asarray(x).astype(F32), np.asarray(w, F32), np.asarray(b, F32)
    if chain:                               # the per-lane kernel: an fmaf chain from the bias (the product is exact in fp64, one rounding per link)
        a = np.broadcast_to(b, (x.shape[0], w.shape[0])).astype(F32)
        for j in range(x.shape[1]):
            a = (a.astype(np.float64) + x[:, j:j + 1].astype(np.float64) * w[:, j].astype(np.float64)).astype(F32)
    else:
        a = (x @ w.T + b).astype(F32)
    if mode == 1:
        s = F32(1) / (F32(1) + np.exp(-a, dtype=F32))
        return ((s * (F32(1) - F32(2) * RGB_EPS) + RGB_EPS) - F32(0.5)) * F32(2), None
    return postprocess_pts_f32(a, False)


def postprocess_pts64(raw, pos_z, k=None, ignore_sign=False):
    """raw fp32 [P, 3 | 4] -> (pts, bound, conf | None, bound | None); pos_z: xyz *= sign(z), 0 for +-0 (ignore_sign: the mutant)"""
    a = f64(raw)[:, :3].copy()
    if pos_z and not ignore_sign:
        a = a * np.sign(a[:, 2:3])
    zero = np.zeros_like(a)
    kp, kc, _ = _k3(k)
    c = (conf64(f64(raw)[:, 3], zero[:, 0], kc) if raw.shape[1] > 3 else (None, None))
    return (*points64(a, zero, kp), *c)


def postprocess_pts_f32(raw, pos_z):
    a = np.asarray(raw, F32)
    xyz = a[:, :3] * np.sign(a[:, 2:3]) if pos_z else a[:, :3]
    d = np.sqrt((xyz * xyz).sum(1, keepdims=True, dtype=F32), dtype=F32)
    pts = xyz / np.maximum(d, F32(1e-8)) * np.expm1(d, dtype=F32)
    return pts.astype(F32), ((F32(1) + np.exp(a[:, 3], dtype=F32)) if a.shape[1] > 3 else None)


def postprocess_pose64(raw, k=K["pts"]):
    """raw fp32 [B, 7] = (t, q) -> (t g(|t|) | q / max(|q|, 1e-12f) with q0 >= 0, bound)"""
    r = f64(raw)
    t, tb = points64(r[:, :3], np.zeros_like(r[:, :3]), k)
    qn = np.maximum(np.sqrt((r[:, 3:] ** 2).sum(1, keepdims=True)), float(F32(1e-12)))
    q = r[:, 3:] / qn
    q = np.where(q[:, :1] < 0, -q, q)
    return np.concatenate([t, q], 1), np.concatenate([tb, k * U * np.abs(q)], 1)


def postprocess_pose_f32(raw):
    r = np.asarray(raw, F32)
    t, _ = postprocess_pts_f32(r[:, :3], False)
    qn = np.maximum(np.sqrt((r[:, 3:] * r[:, 3:]).sum(1, keepdims=True, dtype=F32), dtype=F32), F32(1e-12))
    q = r[:, 3:] / qn
    return np.concatenate([t, np.where(q[:, :1] < 0, -q, q)], 1).astype(F32)


def dpt_problem(P, Cin, nout, seed, zero_bias=False):
    """x fp16 [P, Cin], w fp32 [nout, Cin], b fp32 [nout]: per-pixel input scales log-uniform over 1e-7 (fp16 subnormals) .. 1e2 and final weights scaled so that
    d = |xyz| runs from ~1e-9 (below the 1e-8 clamp; only with zero_bias, where xyz is the dot product alone) to ~5 and the confidence
    logit over about -20 .. 20; every 5th pixel (from the 2nd) is exactly 0, which with zero_bias is xyz = 0"""
    g = np.random.default_rng(seed)
    scale = 10.0 ** np.linspace(-7, 2, P)[g.permutation(P)] if P > 1 else np.ones(1)
    x = (g.standard_normal((P, Cin)) * scale[:, None])
    x[1::5] = 0.0
    x = x.astype(np.float16)
    w = g.standard_normal((nout, Cin)) * (0.03 / math.sqrt(Cin))
    if nout == 4:
        w[3] *= 4.0
    b = g.standard_normal(nout) * 1e-4
    if zero_bias:
        b[:3] = 0.0
    return x, w.astype(F32), b.astype(F32)


# ------------------------------------------------------------------------------------------------ GEMV
def _erf(x):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(f64(x)))).numpy()


def _gelu(x):
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def _gelu_d(x):
    return 0.5 * (1.0 + _erf(x / math.sqrt(2.0))) + x * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gemv_interval(X, W, bias, act, res, silu_in, k=K["gemv"], round_act=True):
    """X fp32 [M, K], W fp16 [N, K], bias fp32 [N] | None, res fp32 [M, N] | None -> (lo, hi) fp64 [M, N], ambiguous activation count
    (round_act False: the mutant whose activations are not rounded to fp16 -- a point reference, lo == hi)"""
    x, w = f64(X), f64(W)
    if silu_in:
        s = x / (1.0 + np.exp(-x))
        tau = (np.abs(x) + 4.0) * U
        a_lo = np.minimum(s * (1 - tau), s * (1 + tau))
        a_hi = np.maximum(s * (1 - tau), s * (1 + tau))
    else:
        a_lo = a_hi = x
    if round_act:
        a_lo, a_hi = f64(a_lo.astype(np.float16)), f64(a_hi.astype(np.float16))
    amb = int((a_lo != a_hi).sum())
    wp, wn = np.maximum(w, 0.0), np.minimum(w, 0.0)
    lo = a_lo @ wp.T + a_hi @ wn.T
    hi = a_hi @ wp.T + a_lo @ wn.T
    mag = np.maximum(np.abs(a_lo), np.abs(a_hi)) @ np.abs(w).T
    if bias is not None:
        lo, hi, mag = lo + f64(bias), hi + f64(bias), mag + np.abs(f64(bias))
    mid, rad = 0.5 * (lo + hi), 0.5 * (hi - lo) + k * U * (mag + np.maximum(np.abs(lo), np.abs(hi)))
    if act == 1:
        out = _gelu(mid)
        rad = np.abs(_gelu_d(mid)) * rad + 0.5 * rad * rad + k * U * (np.abs(out) + 0.5 * np.abs(mid))
        mid = out
    elif act != 0:
        raise ValueError("gemv has no such activation")
    if res is not None:
        mid = mid + f64(res)
        rad = rad + k * U * (np.abs(f64(res)) + np.abs(mid))
    return mid - rad, mid + rad, amb


def gemv_f32(X, W, bias, act, res, silu_in):
    x = np.asarray(X, F32)
    if silu_in:
        x = x / (F32(1) + np.exp(-x, dtype=F32))
    y = (x.astype(np.float16).astype(F32) @ np.asarray(W).astype(F32).T).astype(F32)
    if bias is not None:
        y = y + bias
    if act == 1:
        t = torch.from_numpy(np.ascontiguousarray(y, dtype=F32))
        y = (0.5 * t * (1.0 + torch.erf(t * 0.70710678118654752440))).numpy()
    if res is not None:
        y = y + res
    return y.astype(F32)


def interval_ratio(got, lo, hi):
    """how far outside [lo, hi] `got` lies, in units of the interval's half width (<= 1 inside): the ratio() of intervals"""
    mid, rad = 0.5 * (lo + hi), 0.5 * (hi - lo)
    return ratio(got, mid, rad)


# ------------------------------------------------------------------------------------------------ ConvTranspose (kernel == stride)
def conv_transpose64(x, wt, bias, s, k=K["convt"], swap=False):
    """x fp16 [B, H, W, Cin], wt fp16 [s*s*Cout, Cin] ordered (i, j, co), bias fp32 [Cout] -> (y fp64 [B, H s, W s, Cout], bound)
    out[b, h s + i, w s + j, co] = sum_c x[b, h, w, c] wt[(i s + j) Cout + co, c] + bias[co]   (swap: the mutant with i and j exchanged)"""
    x, wt, bias = f64(x), f64(wt), f64(bias)
    B, Hh, W, Cin = x.shape
    Cout = wt.shape[0] // (s * s)

    def scatter(t):                       # [B, H, W, s, s, Cout] -> [B, H s, W s, Cout]
        if swap:
            t = t.transpose(0, 1, 2, 4, 3, 5)
        return t.transpose(0, 1, 3, 2, 4, 5).reshape(B, Hh * s, W * s, Cout)
    y = scatter((x.reshape(-1, Cin) @ wt.T).reshape(B, Hh, W, s, s, Cout) + bias)
    mag = scatter((np.abs(x).reshape(-1, Cin) @ np.abs(wt).T).reshape(B, Hh, W, s, s, Cout) + np.abs(bias))
    return y, H16 * np.abs(y) + S16 + k * U * mag


def conv_transpose_f32(x, wt, bias, s):
    x, wt = np.asarray(x).astype(F32), np.asarray(wt).astype(F32)
    B, Hh, W, Cin = x.shape
    Cout = wt.shape[0] // (s * s)
    t = ((x.reshape(-1, Cin) @ wt.T).astype(F32).reshape(B, Hh, W, s, s, Cout) + np.asarray(bias, F32)).astype(np.float16)
    return t.transpose(0, 1, 3, 2, 4, 5).reshape(B, Hh * s, W * s, Cout)


# ------------------------------------------------------------------------------------------------ inputs shared by the CPU and GPU tests
def colmean_inputs(M, C, seed):
    g = np.random.default_rng(seed)
    x = g.standard_normal((M, C))
    n3 = len(range(0, C, 3))
    x[:, ::3] = 1e3 * np.sign(g.standard_normal((M, n3))) * (1.0 + 0.1 * g.standard_normal((M, n3)))       # |x| ~ 1e3, mean ~ 0: cancellation
    return x.astype(F32)


def upsample_input(B, Hh, W, C, seed):
    g = np.random.default_rng(seed)
    return (g.standard_normal((B, Hh, W, C)) * 10.0 ** g.uniform(-2, 2, (1, 1, 1, C))).astype(np.float16)


def pts_raw(nch, seed):
    g = np.random.default_rng(seed)
    P = 203
    raw = g.standard_normal((P, nch)) * 10.0 ** np.linspace(-9.5, 0.6, P)[:, None]
    if nch == 4:
        raw[:, 3] = g.uniform(-20, 20, P)
    raw[0, :3], raw[1, 2], raw[2, 2] = 0.0, 0.0, -0.0
    return raw.astype(F32)


def pose_raw():
    g = np.random.default_rng(5)
    rows = []
    for tn in (0.0, 1e-9, 1.0, 5.0):
        for q in ("zero", "q0_zero", "q0_neg", "plain"):
            t = g.standard_normal(3)
            t = t / np.linalg.norm(t) * tn
            qq = g.standard_normal(4)
            if q == "zero":
                qq[:] = 0.0
            elif q == "q0_zero":
                qq[0] = 0.0
            elif q == "q0_neg":
                qq[0] = -abs(qq[0])
            else:
                qq[0] = abs(qq[0])
            rows.append(np.concatenate([t, qq]))
    return np.asarray(rows, F32)


def gemv_problem(M, N, Kd, seed, bias=True, res=False):
    g = np.random.default_rng(seed)
    X = (1.5 * g.standard_normal((M, Kd))).astype(F32)
    W = (g.standard_normal((N, Kd)) / np.sqrt(Kd)).astype(np.float16)
    return X, W, (g.standard_normal(N).astype(F32) if bias else None), (g.standard_normal((M, N)).astype(F32) if res else None)


def convt_problem(s, Cin, Cout, Hh, W, B):
    g = np.random.default_rng(s * 100 + Cin)
    x = g.standard_normal((B, Hh, W, Cin)).astype(np.float16)
    w = (g.standard_normal((Cin, Cout, s, s)) / np.sqrt(Cin)).astype(np.float16)             # torch's ConvTranspose2d layout
    wt = np.ascontiguousarray(w.transpose(2, 3, 1, 0).reshape(s * s * Cout, Cin))
    return x, w, wt, g.standard_normal(Cout).astype(F32)


COLMEAN_M = (1, 2, 3, 4, 5, 13, 16, 17, 29, 769)


UPSAMPLE_HW = ((1, 1), (1, 5), (5, 1), (2, 3), (5, 7), (12, 16))


CONVT = ((2, 8, 4, 1, 1, 1), (4, 72, 36, 3, 5, 3), (2, 192, 192, 6, 8, 2))
