"""fp64 evaluation, PER-ELEMENT error bounds and decision margins of the per-Gaussian projection of the Gaussian rasteriser (csrc/gs.hip:
gs_project, sh_basis, gs_preprocess_kernel, gs_project_bwd, gs_preprocess_bwd_kernel, i.e. cut3r_gs_preprocess and
cut3r_gs_preprocess_backward).  CPU only (numpy); shared by tests/test_gs_project_cpu.py and tests/test_gs_project_gpu.py.  Not collected.

The projection of one Gaussian is written ONCE (`project`, `sh_basis`), generic over its number type as the kernel's template is, and
evaluated, vectorised over the Gaussians, on
  (a) fp64 values carried with the first-order bound of their fp32 error (EV of tests/gs_render_oracle.py): the reference and the bound,
  (b) fp32 values in the kernel's order of operations (EV without a bound): the restatement that measures RATIO and carries the mutants,
  (c) forward-mode duals (class Dual: 10 parts mean / scale / quaternion for the projection, 3 parts for the SH basis) whose value and
      parts are EVs of kind (a) or (b), with the operator definitions of csrc/lie_math.h (a / b = a * (1 / b), Sqrt' = 0.5 / sqrt): the
      derivative, contracted with dgeom in the kernel's order, and its bound.
Constants are the fp32 numbers the kernel holds (0.2f, 1.3f * tanfov, 1e-6f, 1e-7f, 1e-8f, 0.1f, the SH constants, fx = W / (2.f * tan)).
`exact_constants=True` takes them as the doubles of oracle/gs_oracle.py instead: only for the cross-check against that module.

Decisions.  A Gaussian is `ambiguous` when one of its deciding quantities lies within MARGIN (4) x its bound of its threshold: z against
0.2; x/z, y/z against the clamp limits; d0, d1 against 1e-6; det against 0; min s^2 against 1e-8; when !well the two comparisons that pick
kmin (bit-equal input scales give bit-equal squares: never ambiguous); mlen against 0; vbn against 1e-7; mid^2 - det against 0.1;
3 sqrt(lambda_max) against the integer its ceiling steps at; each of the four tile quotients against an integer in 1..g (truncation and
the clamp to [0, g] make every other integer irrelevant); colour + 0.5 against 0.  The comparisons are strict in the bound, so an exact
quantity (bound 0) is never ambiguous.  Ambiguous Gaussians are left out of every comparison; integers (radius, rectangle, tiles,
clamp bits) and the culled / visible decision are exact on all the others.

The non-finite `mlen` exit CAN be reached with finite inputs: with !well only g[kmin] = R[:, kmin] . w survives, and it is exactly 0 for a
flat Gaussian whose thin axis is perpendicular to the viewing ray (identity view, identity quaternion, thin x axis, centre on the optical
axis: case `one`); its camera plane, ray plane and normal are 0 and so are their derivatives.

An equivalent mutant: `floor` for the truncation of the tile rectangle differs only for quotients in (-1, 0), which the clamp to [0, g]
sends to 0 either way; no comparison can reject it, so it is not among the mutants.

The constants K.  RATIO per field group is the largest |fp32 restatement - reference| / bound over the unambiguous Gaussians of every
case of tests/gs_project_cases.py, measured by tests/test_gs_project_cpu.py, plus 0.05, rounded up to a decimal; K = max(1, 2 RATIO), the
rule of tests/gs_render_oracle.py (the kernel contracts multiply-adds and the compiler orders sums its own way).

  record field   measured (worst case of)   RATIO  K        gradient     measured (worst case of)   RATIO  K
  xy             0.329  (sh65)              0.4   1.0       d_means      0.146  (scene300)          0.2   1.0
  depth          0.579  (hand257)           0.7   1.4       d_scales     0.055  (one)               0.2   1.0
  ts             0.825  (sh65)              0.9   1.8       d_rots       0.037  (one)               0.1   1.0
  conic          0.338  (hand257)           0.4   1.0       d_opacities  0.041  (sh65)              0.1   1.0
  op             0.048  (sh65)              0.1   1.0       d_shs        0.959  (scene300)          1.1   2.2
  rgb            0.639  (one)               0.7   1.4
  vp             0.593  (hand257)           0.7   1.4
  cp             0.347  (scene300)          0.4   1.0
  rp             0.069  (hand257)           0.2   1.0
  nrm            0.062  (hand257)           0.2   1.0
  (depth, ts, vp, rgb and d_shs are one or two roundings deep, so a single value comes close to its worst case; the conic, the planes
  and the gradients are long chains with cancellations, whose worst-case bound no actual rounding pattern comes near.)
  The kernels on an MI355X against K x bound (tests/test_gs_project_gpu.py): records at most 0.46 (ts, rgb), gradients at most 0.44 (d_shs).
"""
import numpy as np

from tests.gs_render_oracle import (EV, F32, F64, G_CLAMP, G_CONIC, G_CP, G_DEPTH, G_NRM, G_OP, G_RADIUS, G_RECT, G_RGB, G_RP, G_TILES, G_TS, G_VP,
                                    G_XY, GS_REC, MARGIN, ints, ratio)

GS_TILE = 16
FIELDS = (("xy", (0, 1)), ("depth", (2,)), ("ts", (3,)), ("conic", (4, 5, 6)), ("op", (7,)), ("rgb", (8, 9, 10)), ("vp", (11, 12, 13)),
          ("cp", tuple(range(14, 20))), ("rp", (20, 21)), ("nrm", (22, 23, 24)))
GRADS = ("d_means", "d_scales", "d_rots", "d_opacities", "d_shs")
RATIO = {"xy": 0.4, "depth": 0.7, "ts": 0.9, "conic": 0.4, "op": 0.1, "rgb": 0.7, "vp": 0.7, "cp": 0.4, "rp": 0.2, "nrm": 0.2,
         "d_means": 0.2, "d_scales": 0.2, "d_rots": 0.1, "d_opacities": 0.1, "d_shs": 1.1}
K = {name: max(1.0, 2.0 * r) for name, r in RATIO.items()}
SH_C1 = 0.4886025119029199
SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
SH_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
         -0.5900435899266435)
MUTANTS = ("near_ge", "clamp_1", "clamp_value_only", "kmin_largest", "keep_g", "coef_not_zeroed", "no_radius_floor", "sh_stride",
           "clampbit_ignored", "mod_once", "means2d_W")


# ------------------------------------------------------------------------------------------------------------------ number types
class Dual:
    """forward-mode dual of csrc/lie_math.h: value `v` (EV [P]) and parts `d` (EV [N, P], or None: identically zero, a constant)"""
    __slots__ = ("v", "d")

    def __init__(self, v, d=None):
        self.v, self.d = v, d

    def __add__(self, o):
        return Dual(self.v + o.v, self.d if o.d is None else (o.d if self.d is None else self.d + o.d))

    def __sub__(self, o):
        return Dual(self.v - o.v, self.d if o.d is None else (-o.d if self.d is None else self.d - o.d))

    def __neg__(self):
        return Dual(-self.v, None if self.d is None else -self.d)

    def __mul__(self, o):
        if self.d is None or o.d is None:
            d = None if self.d is None and o.d is None else (self.d * o.v if o.d is None else self.v * o.d)
        else:
            d = self.d * o.v + self.v * o.d
        return Dual(self.v * o.v, d)

    def __truediv__(self, o):
        inv = 1.0 / o.v
        v = self.v * inv
        if o.d is None:
            d = None if self.d is None else self.d * inv
        else:
            d = (-(v * o.d)) * inv if self.d is None else (self.d - v * o.d) * inv
        return Dual(v, d)


def val(x):
    return x.v.v if isinstance(x, Dual) else x.v


def ev(x):
    return x.v if isinstance(x, Dual) else x


def _ev_select(m, a, b):
    return a.where(m, b)


class Ctx:
    """what one evaluation needs beside the numbers: the float type (fp64 with bounds or fp32), how many dual parts, the constants,
    the mutants of the restatement and the decision margins it collects"""

    def __init__(self, P, f32, parts=0, exact_constants=False, mutants=()):
        self.P, self.f32, self.parts, self.exact, self.mutants = P, f32, parts, exact_constants, frozenset(mutants)
        self.dt = F32 if f32 else F64
        self.amb = np.zeros(P, dtype=bool)
        self.why = {}

    def k(self, x):
        """the value of a constant the kernel holds in fp32"""
        return float(x) if self.exact else float(F32(x))

    def ev_of(self, a):
        a = np.broadcast_to(np.asarray(a, dtype=self.dt), np.shape(a) if np.ndim(a) else (self.P,)).copy()
        return EV(a, None if self.f32 else np.zeros(a.shape))

    def const(self, x):
        """a constant of the evaluation's number type (x already the value held)"""
        e = self.ev_of(np.full(self.P, x))
        return Dual(e) if self.parts else e

    def seed(self, a, part):
        """input column `a` [P] (exact) as a number; with duals, d[part] = 1"""
        e = self.ev_of(a)
        if not self.parts:
            return e
        d = np.zeros((self.parts, self.P))
        if part is not None:
            d[part] = 1.0
        return Dual(e, self.ev_of(d))

    def zeros_d(self):
        return self.ev_of(np.zeros((self.parts, self.P)))

    def select(self, m, a, b):
        if not isinstance(a, Dual):
            return _ev_select(m, a, b)
        if a.d is None and b.d is None:
            return Dual(_ev_select(m, a.v, b.v))
        ad, bd = (self.zeros_d() if a.d is None else a.d), (self.zeros_d() if b.d is None else b.d)
        return Dual(_ev_select(m, a.v, b.v), _ev_select(m, ad, bd))

    def sqrt(self, x):
        if not isinstance(x, Dual):
            return x.sqrt()
        r = x.v.sqrt()
        return Dual(r, None if x.d is None else (0.5 / r) * x.d)

    def maxc(self, x, c):
        return self.select(val(x) < c, self.const(c), x)

    def clampv(self, x, lo, hi):
        y = self.select(val(x) < lo, self.const(lo), self.select(val(x) > hi, self.const(hi), x))
        if "clamp_value_only" in self.mutants and isinstance(x, Dual):
            y = Dual(y.v, x.d)
        return y

    def note(self, name, q, thr, active=True, tol=None):
        """the decision `q` against `thr`: within MARGIN x its bound is ambiguous"""
        if q.e is None:
            return
        a = (np.abs(q.v - thr) < MARGIN * (q.e if tol is None else tol)) & active
        self.why[name] = self.why.get(name, 0) | a
        self.amb |= a


def camera(view, proj, campos, W, H, tanx, tany, ks, mod, deg, K, exact_constants=False):
    """the GsCam the host fills: fp32 matrices, fx = (float) W / (2.f * tanx) in fp32"""
    view, proj, campos = (np.asarray(a, dtype=F32).reshape(-1) for a in (view, proj, campos))
    tanx, tany, ks, mod = F32(tanx), F32(tany), F32(ks), F32(mod)
    if exact_constants:
        fx, fy = W / (2.0 * float(tanx)), H / (2.0 * float(tany))
    else:
        fx, fy = float(F32(W) / (F32(2.0) * tanx)), float(F32(H) / (F32(2.0) * tany))
    return dict(view=view.astype(F64), proj=proj.astype(F64), campos=campos.astype(F64), W=W, H=H, tanx=float(tanx), tany=float(tany), fx=fx, fy=fy,
                ks=float(ks), mod=float(mod), deg=deg, K=K)


# ------------------------------------------------------------------------------------------------------------------ the projection
def project(mean, scale, rot, cam, cx):
    """gs_project for all Gaussians at once on the numbers of `cx` -> dict of numbers and the boolean arrays in_front, det_ok, bad"""
    c, k, V, PM, mut = cx.const, cx.k, cam["view"], cam["proj"], cx.mutants
    o = {}
    pv = [mean[0] * c(V[i]) + mean[1] * c(V[4 + i]) + mean[2] * c(V[8 + i]) + c(V[12 + i]) for i in range(3)]
    ph = [mean[0] * c(PM[i]) + mean[1] * c(PM[4 + i]) + mean[2] * c(PM[8 + i]) + c(PM[12 + i]) for i in range(4)]
    near = k(0.2)
    front = (val(pv[2]) >= near) if "near_ge" in mut else (val(pv[2]) > near)
    cx.note("z", ev(pv[2]), near)
    p_w = c(1.0) / (ph[3] + c(k(1e-7)))
    o["xy"] = [((ph[0] * p_w + c(1.0)) * c(float(cam["W"])) - c(1.0)) * c(0.5), ((ph[1] * p_w + c(1.0)) * c(float(cam["H"])) - c(1.0)) * c(0.5)]
    o["vp"] = pv
    o["ts"] = cx.sqrt(pv[0] * pv[0] + pv[1] * pv[1] + pv[2] * pv[2])
    r, x, y, z = rot
    one, two = c(1.0), c(2.0)
    R = [[one - two * (y * y + z * z), two * (x * y - r * z), two * (x * z + r * y)],
         [two * (x * y + r * z), one - two * (x * x + z * z), two * (y * z - r * x)],
         [two * (x * z - r * y), two * (y * z + r * x), one - two * (x * x + y * y)]]
    s2 = []
    for kk in range(3):
        if "mod_once" in mut:
            s2.append(c(cam["mod"]) * (scale[kk] * scale[kk]))
        else:
            s = c(cam["mod"]) * scale[kk]
            s2.append(s * s)
    tz = cx.select(front, pv[2], c(1.0))
    f13 = 1.0 if "clamp_1" in mut else 1.3
    if cx.exact:
        limx, limy = f13 * cam["tanx"], f13 * cam["tany"]
    else:
        limx, limy = float(F32(f13) * F32(cam["tanx"])), float(F32(f13) * F32(cam["tany"]))
    rx, ry = pv[0] / tz, pv[1] / tz
    for name, q, lim in (("clamp_x", rx, limx), ("clamp_y", ry, limy)):
        cx.note(name + "_lo", ev(q), -lim, front)
        cx.note(name + "_hi", ev(q), lim, front)
    txtz, tytz = cx.clampv(rx, -limx, limx), cx.clampv(ry, -limy, limy)
    o["clamped"] = (val(rx) != val(txtz)) | (val(ry) != val(tytz))
    tx, ty = txtz * tz, tytz * tz
    fx, fy = c(cam["fx"]), c(cam["fy"])
    j00, j02, j11, j12 = fx / tz, -(fx * tx) / (tz * tz), fy / tz, -(fy * ty) / (tz * tz)
    A = [[j00 * c(V[4 * j + 0]) + j02 * c(V[4 * j + 2]) for j in range(3)], [j11 * c(V[4 * j + 1]) + j12 * c(V[4 * j + 2]) for j in range(3)]]
    B = [[A[i][0] * R[0][kk] + A[i][1] * R[1][kk] + A[i][2] * R[2][kk] for kk in range(3)] for i in range(2)]
    c00 = B[0][0] * B[0][0] * s2[0] + B[0][1] * B[0][1] * s2[1] + B[0][2] * B[0][2] * s2[2]
    c01 = B[0][0] * B[1][0] * s2[0] + B[0][1] * B[1][1] * s2[1] + B[0][2] * B[1][2] * s2[2]
    c11 = B[1][0] * B[1][0] * s2[0] + B[1][1] * B[1][1] * s2[1] + B[1][2] * B[1][2] * s2[2]
    ksn = c(cam["ks"])
    a, b, cc = c00 + ksn, c01, c11 + ksn
    o["cov"] = [a, b, cc]
    e6 = k(1e-6)
    d0r, d1r = c00 * c11 - c01 * c01, a * cc - c01 * c01
    cx.note("d0", ev(d0r), e6, front)
    cx.note("d1", ev(d1r), e6, front)
    d0, d1 = cx.maxc(d0r, e6), cx.maxc(d1r, e6)
    coef = cx.sqrt(d0 / (d1 + c(e6)) + c(e6))
    o["coef_zero"] = (val(d0) <= e6) | (val(d1) <= e6)
    o["coef"] = coef if "coef_not_zeroed" in mut else cx.select(o["coef_zero"], c(0.0), coef)
    det = a * cc - b * b
    cx.note("det", ev(det), 0.0, front)
    det_ok = val(det) != 0.0
    di = c(1.0) / cx.select(det_ok, det, c(1.0))
    o["conic"] = [cc * di, -b * di, a * di]
    v0, v1, v2 = (val(s) for s in s2)
    kmin = np.where(v0 > v1, np.where(v1 > v2, 2, 1), np.where(v0 > v2, 2, 0))
    if "kmin_largest" in mut:
        kmin = np.argmax(np.stack([v0, v1, v2]), axis=0)
    smin = cx.select(kmin == 0, s2[0], cx.select(kmin == 1, s2[1], s2[2]))
    e8 = k(1e-8)
    well = val(smin) > e8
    cx.note("well", ev(smin), e8, front)
    if not cx.f32:                                                             # the comparisons that pick kmin, where it matters
        e = [ev(s) for s in s2]
        sc = [val(s) for s in scale]
        first = (np.abs(v0 - v1) < MARGIN * (e[0].e + e[1].e)) & (sc[0] != sc[1])
        second = np.where(v0 > v1, (np.abs(v1 - v2) < MARGIN * (e[1].e + e[2].e)) & (sc[1] != sc[2]),
                          (np.abs(v0 - v2) < MARGIN * (e[0].e + e[2].e)) & (sc[0] != sc[2]))
        pick = (first | second) & front & ~well
        cx.why["kmin"] = pick
        cx.amb |= pick
    uvh = [txtz, tytz, c(1.0)]
    w = [c(V[4 * j + 0]) * uvh[0] + c(V[4 * j + 1]) * uvh[1] + c(V[4 * j + 2]) * uvh[2] for j in range(3)]
    g = [R[0][kk] * w[0] + R[1][kk] * w[1] + R[2][kk] * w[2] for kk in range(3)]
    for kk in range(3):
        flat = g[kk] if "keep_g" in mut else cx.select(kmin == kk, g[kk], c(0.0))
        g[kk] = cx.select(well, g[kk] / cx.select(well, s2[kk], c(1.0)), flat)
    q = [R[i][0] * g[0] + R[i][1] * g[1] + R[i][2] * g[2] for i in range(3)]
    m = [c(V[0 + i]) * q[0] + c(V[4 + i]) * q[1] + c(V[8 + i]) * q[2] for i in range(3)]
    mlen = cx.sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2])
    mv = val(mlen)
    bad = ~(mv > 0.0) | ~np.isfinite(mv)
    cx.note("mlen", ev(mlen), 0.0, front)
    ml = cx.select(bad, c(1.0), mlen)
    n0, n1, n2 = m[0] / ml, m[1] / ml, m[2] / ml
    u2, vv2, uv = txtz * txtz, tytz * tytz, txtz * tytz
    l = cx.sqrt(tx * tx + ty * ty + tz * tz)
    e7 = k(1e-7)
    vbr = n0 * uvh[0] + n1 * uvh[1] + n2
    cx.note("vbn", ev(vbr), e7, front & ~bad)
    o["vbn_floored"] = val(vbr) < e7
    vbn = cx.maxc(vbr, e7)
    a0, a1, a2 = n0 / vbn, n1 / vbn, n2 / vbn
    p0 = (vv2 + one) * a0 - uv * a1 - txtz * a2
    p1 = (u2 + one) * a1 - uv * a0 - tytz * a2
    nl = u2 + vv2 + one
    if cx.exact:
        ifx, ify = c(1.0 / cam["fx"]) / nl, c(1.0 / cam["fy"]) / nl
    else:
        ifx, ify = c(float(F32(1.0) / F32(cam["fx"]))) / nl, c(float(F32(1.0) / F32(cam["fy"]))) / nl
    cp = [(p0 * tx - (vv2 + one) * tz) * ifx, (uv * tz + p1 * tx) * ify, (uv * tz + p0 * ty) * ifx, (p1 * ty - (u2 + one) * tz) * ify,
          (tx + p0 * tz) * ifx, (ty + p1 * tz) * ify]
    rp = [p0 * l * ifx, p1 * l * ify]
    fn = l / nl
    r0, r1 = -p0 * fn, -p1 * fn
    c0, c1, c2 = r0 / tz - tx / l, r1 / tz - ty / l, -(r0 * tx + r1 * ty) / (tz * tz) - tz / l
    cl = cx.sqrt(c0 * c0 + c1 * c1 + c2 * c2)
    zero = c(0.0)
    o["cp"] = [cx.select(bad, zero, t) for t in cp]
    o["rp"] = [cx.select(bad, zero, t) for t in rp]
    o["nrm"] = [cx.select(bad, zero, t) for t in (c0 / cl, c1 / cl, c2 / cl)]
    o.update(in_front=front, det_ok=det_ok, bad=bad, well=well, kmin=kmin)
    return o


def sh_basis(mean, cam, cx):
    """sh_basis: the (deg + 1)^2 basis values at the unit direction mean - campos"""
    c, k, deg = cx.const, cx.k, cam["deg"]
    d = [mean[i] - c(cam["campos"][i]) for i in range(3)]
    ln = cx.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    x, y, z = d[0] / ln, d[1] / ln, d[2] / ln
    b = [c(k(0.28209479177387814))]
    if deg > 0:
        b += [-c(k(SH_C1)) * y, c(k(SH_C1)) * z, -c(k(SH_C1)) * x]
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        C2 = [c(k(v)) for v in SH_C2]
        b += [C2[0] * xy, C2[1] * yz, C2[2] * (c(2.0) * zz - xx - yy), C2[3] * xz, C2[4] * (xx - yy)]
    if deg > 2:
        C3 = [c(k(v)) for v in SH_C3]
        b += [C3[0] * y * (c(3.0) * xx - yy), C3[1] * xy * z, C3[2] * y * (c(4.0) * zz - xx - yy),
              C3[3] * z * (c(2.0) * zz - c(3.0) * xx - c(3.0) * yy), C3[4] * x * (c(4.0) * zz - xx - yy), C3[5] * z * (xx - yy),
              C3[6] * x * (xx - c(3.0) * yy)]
    return b


def _inputs(case):
    g = lambda name: np.ascontiguousarray(case[name], dtype=F32)
    return g("means"), g("scales"), g("rots"), g("opac").reshape(-1)


def _cam(case, exact_constants=False):
    return camera(case["view"], case["proj"], case["campos"], case["W"], case["H"], case["tanx"], case["tany"], case["ks"], case["mod"],
                  case["deg"], case["K"], exact_constants)


def _sh_rows(case, cx, nb):
    """the coefficients each Gaussian reads: shs + i * K * 3 (stride K, not nb) -> [P, nb, 3]"""
    shs = np.ascontiguousarray(case["shs"], dtype=F32)
    P, K = shs.shape[0], case["K"]
    flat = shs.reshape(-1)
    stride = nb if "sh_stride" in cx.mutants else K
    idx = (np.arange(P)[:, None, None] * stride * 3 + np.arange(nb)[None, :, None] * 3 + np.arange(3)[None, None, :])
    return flat[np.minimum(idx, flat.size - 1)]


# ------------------------------------------------------------------------------------------------------------------ forward
def _forward(case, f32, mutants=(), exact_constants=False):
    means, scales, rots, opac = _inputs(case)
    P, W, H = means.shape[0], case["W"], case["H"]
    cx = Ctx(P, f32, 0, exact_constants, mutants)
    cam = _cam(case, exact_constants)
    c = cx.const
    with np.errstate(all="ignore"):
        o = project([cx.seed(means[:, i], None) for i in range(3)], [cx.seed(scales[:, i], None) for i in range(3)],
                    [cx.seed(rots[:, i], None) for i in range(4)], cam, cx)
        live = o["in_front"] & o["det_ok"]
        cov = o["cov"]
        mid = c(0.5) * (cov[0] + cov[2])
        disc = mid * mid - (cov[0] * cov[2] - cov[1] * cov[1])
        tenth = cx.k(0.1)
        cx.note("radius_floor", disc, tenth, live)
        root = cx.sqrt(cx.maxc(disc, 0.0) if "no_radius_floor" in cx.mutants else cx.maxc(disc, tenth))
        hi, lo = mid + root, mid - root
        r3 = c(3.0) * cx.sqrt(cx.select(hi.v >= lo.v, hi, lo))
        cx.note("radius", r3, np.round(r3.v), live)
        rad = np.where(live, np.ceil(np.where(np.isfinite(r3.v), r3.v, 0.0)), 0.0).astype(np.int64)
        gx, gy = (W + GS_TILE - 1) // GS_TILE, (H + GS_TILE - 1) // GS_TILE
        radn = cx.ev_of(rad.astype(F64))
        rect = []
        for name, qn, g in (("x0", o["xy"][0] - radn, gx), ("y0", o["xy"][1] - radn, gy), ("x1", o["xy"][0] + radn + c(15.0), gx),
                            ("y1", o["xy"][1] + radn + c(15.0), gy)):
            qn = qn / c(16.0)
            n = np.round(qn.v)
            cx.note("tile_" + name, qn, n, live & (n >= 1) & (n <= g))
            rect.append(np.clip(np.trunc(np.where(np.isfinite(qn.v), qn.v, 0.0)).astype(np.int64), 0, g))
        rect = np.stack(rect, 1)
        tiles = (rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1])
        vis = live & (tiles > 0)
        clampbits = np.zeros(P, dtype=np.int64)
        if case.get("colors") is not None:
            col = np.ascontiguousarray(case["colors"], dtype=F32)
            rgb = [cx.ev_of(col[:, ch]) for ch in range(3)]
        else:
            nb = (cam["deg"] + 1) ** 2
            basis = sh_basis([cx.seed(means[:, i], None) for i in range(3)], cam, cx)
            sh = _sh_rows(case, cx, nb)
            rgb = []
            for ch in range(3):
                v = basis[0] * cx.ev_of(sh[:, 0, ch])
                for kk in range(1, nb):
                    v = v + basis[kk] * cx.ev_of(sh[:, kk, ch])
                v = v + c(0.5)
                cx.note("colour%d" % ch, v, 0.0, vis)
                neg = v.v < 0.0
                clampbits |= np.where(neg, 1 << ch, 0)
                rgb.append(c(0.0).where(neg, v))
        op = cx.ev_of(opac) * o["coef"]
    cols = {G_XY: o["xy"][0], G_XY + 1: o["xy"][1], G_DEPTH: o["vp"][2], G_TS: o["ts"], G_OP: op}
    for i in range(3):
        cols[G_CONIC + i], cols[G_RGB + i], cols[G_VP + i], cols[G_NRM + i] = o["conic"][i], rgb[i], o["vp"][i], o["nrm"][i]
    for i in range(6):
        cols[G_CP + i] = o["cp"][i]
    cols[G_RP], cols[G_RP + 1] = o["rp"]
    geom = np.zeros((P, GS_REC), dtype=cx.dt)
    bound = np.zeros((P, GS_REC))
    for s, e in cols.items():
        geom[:, s] = np.where(vis, e.v, 0)
        if not f32:
            bound[:, s] = np.where(vis, e.e, 0.0)
    rad, tiles, rect, clampbits = (np.where(vis.reshape((-1,) + (1,) * (a.ndim - 1)), a, 0) for a in (rad, tiles, rect, clampbits))
    res = dict(geom=geom, radii=rad.astype(np.int32), tiles=tiles.astype(np.uint32), rect=rect.astype(np.int32), clampbits=clampbits.astype(np.uint32),
               visible=vis, offsets=np.cumsum(tiles).astype(np.uint32))
    if not f32:
        res.update(bound=bound, ambiguous=cx.amb.copy(), why={n: np.asarray(a) & np.ones(P, bool) for n, a in cx.why.items()},
                   side={n: o[n] for n in ("in_front", "det_ok", "bad", "well", "kmin", "coef_zero", "vbn_floored", "clamped")})
        res["side"]["radius_floored"] = disc.v < tenth
    return res


def forward_reference(case, exact_constants=False):
    """fp64: `geom` [P, 32] (slots 0..24; culled rows 0), `bound` (per element, to be scaled by K), exact `radii`, `tiles`, `rect`, `clampbits`,
    `offsets`, `visible`, the mask `ambiguous`, `why` (which decision) and `side` (the branch each Gaussian takes)"""
    return _forward(case, False, (), exact_constants)


def forward_f32(case, mutants=()):
    """the kernel's operation order in fp32 numpy, as the outputs of the kernel (geom with its bit-cast integer slots, radii, tiles, offsets);
    `mutants`: near_ge, clamp_1, kmin_largest, keep_g, coef_not_zeroed, no_radius_floor, sh_stride, mod_once"""
    res = _forward(case, True, mutants)
    return dict(res, geom=records_f32(res))


def records_f32(ref):
    """the records a forward result stands for, as the fp32 / bit-cast array the kernel writes (for the backward pass and comparisons)"""
    g = np.ascontiguousarray(ref["geom"], dtype=F32).copy()
    vis = ref["visible"]
    g[:, G_RADIUS] = ref["radii"].astype(F32)
    g[:, G_TILES] = ref["tiles"].astype(np.int32).view(F32)
    g[:, G_RECT:G_RECT + 4] = ref["rect"].astype(np.int32).view(F32)
    g[:, G_CLAMP] = ref["clampbits"].astype(np.uint32).view(F32)
    g[~vis] = 0
    return g


# ------------------------------------------------------------------------------------------------------------------ backward
def _backward(case, geom, dgeom, f32, mutants=(), exact_constants=False):
    means, scales, rots, opac = _inputs(case)
    P = means.shape[0]
    cam = _cam(case, exact_constants)
    cx = Ctx(P, f32, 10, exact_constants, mutants)
    geom, dg = np.ascontiguousarray(geom, dtype=F32), np.ascontiguousarray(dgeom, dtype=F32)
    vis = geom[:, G_RADIUS] > 0
    e1 = lambda a: EV(np.asarray(a, dtype=cx.dt), None if f32 else np.zeros(np.shape(a)))
    with np.errstate(all="ignore"):
        o = project([cx.seed(means[:, i], i) for i in range(3)], [cx.seed(scales[:, i], 3 + i) for i in range(3)],
                    [cx.seed(rots[:, i], 6 + i) for i in range(4)], cam, cx)
        gin = None
        terms = [(o["xy"][0], G_XY), (o["xy"][1], G_XY + 1), (o["ts"], G_TS)] + [(o["conic"][i], G_CONIC + i) for i in range(3)] + [(o["coef"], None)]
        for i in range(3):
            terms += [(o["vp"][i], G_VP + i), (o["nrm"][i], G_NRM + i)]
        terms += [(o["cp"][i], G_CP + i) for i in range(6)] + [(o["rp"][0], G_RP), (o["rp"][1], G_RP + 1)]
        for f, slot in terms:
            gf = e1(dg[:, slot]) if slot is not None else e1(dg[:, G_OP]) * e1(opac)
            if f.d is None:
                continue
            t = gf * f.d
            gin = t if gin is None else gin + t
        out = {"d_opacities": e1(dg[:, G_OP]) * o["coef"].v}
        if case.get("colors") is None:
            c3 = Ctx(P, f32, 3, exact_constants, mutants)
            nb, K = (cam["deg"] + 1) ** 2, cam["K"]
            basis = sh_basis([c3.seed(means[:, i], i) for i in range(3)], cam, c3)
            sh = _sh_rows(case, c3, nb)
            bits = ints(geom[:, G_CLAMP]).astype(np.int64)
            dshv, dshe = np.zeros((P, K, 3), dtype=cx.dt), np.zeros((P, K, 3))
            g3 = [EV(gin.v[i], None if f32 else gin.e[i]) for i in range(3)]
            for ch in range(3):
                keep = np.ones(P, bool) if "clampbit_ignored" in mutants else ((bits >> ch) & 1) == 0
                gc = e1(np.where(keep, dg[:, G_RGB + ch], 0))
                for kk in range(nb):
                    t = gc * basis[kk].v
                    dshv[:, kk, ch] = t.v
                    if not f32:
                        dshe[:, kk, ch] = t.e
                    if basis[kk].d is None:
                        continue
                    wgt = gc * e1(sh[:, kk, ch])
                    for i in range(3):
                        bd = basis[kk].d
                        g3[i] = g3[i] + wgt * EV(bd.v[i], None if f32 else bd.e[i])
            gv = gin.v.copy()
            ge = None if f32 else gin.e.copy()
            for i in range(3):
                gv[i] = g3[i].v
                if not f32:
                    ge[i] = g3[i].e
            gin = EV(gv, ge)
            out["d_shs"] = EV(dshv, None if f32 else dshe)
            out["sh_written"] = np.broadcast_to((np.arange(K) < nb)[None, :, None], (P, K, 3))
        else:
            out["d_colors"] = dg[:, G_RGB:G_RGB + 3].copy()
        out["d_means"], out["d_scales"], out["d_rots"] = (EV(gin.v[a:b].T, None if f32 else gin.e[a:b].T) for a, b in ((0, 3), (3, 6), (6, 10)))
    wx = F32(case["W"]) if "means2d_W" in mutants else None
    m2 = np.stack([(dg[:, G_XY] * F32(0.5) * F32(case["W"])) if wx is None else dg[:, G_XY] * wx, dg[:, G_XY + 1] * F32(0.5) * F32(case["H"]),
                   dg[:, G_DEPTH]], 1).astype(F32)
    res = dict(visible=vis, d_means2D=m2, d_colors=out.get("d_colors"), sh_written=out.get("sh_written"))
    for name in GRADS:
        if name in out:
            t = out[name]
            m = vis.reshape((-1,) + (1,) * (t.v.ndim - 1))
            res[name] = np.where(m, t.v, 0)
            if not f32:
                res[name + "_bound"] = np.where(m, t.e, 0.0)
    return res


def backward_reference(case, geom, dgeom, exact_constants=False):
    """fp64 d_means, d_scales, d_rots, d_opacities, d_shs (and `<name>_bound`, to be scaled by K) of the records `geom` (fp32, as stored) and
    their gradients `dgeom`; exact d_means2D (fp32 products) and d_colors; `sh_written` marks the d_shs entries the kernel writes"""
    return _backward(case, geom, dgeom, False, (), exact_constants)


def backward_f32(case, geom, dgeom, mutants=()):
    """the kernel's operation order in fp32 numpy; `mutants`: clamp_value_only, clampbit_ignored, means2d_W, sh_stride and the forward's"""
    return _backward(case, geom, dgeom, True, mutants)


# ------------------------------------------------------------------------------------------------------------------ comparisons
def compare_forward(got, ref):
    """`got` (geom [P, 32] fp32 as stored, radii, tiles, offsets) against a forward reference on its unambiguous Gaussians ->
    ({field: (largest error / (K bound), elements beyond)}, number of integer / culling mismatches)"""
    keep = ~ref["ambiguous"]
    g = np.asarray(got["geom"], dtype=F32)
    res = {name: ratio(g[:, list(s)], ref["geom"][:, list(s)], K[name] * ref["bound"][:, list(s)], keep[:, None]) for name, s in FIELDS}
    bad = 0
    bad += int((np.asarray(got["radii"]).astype(np.int64) != ref["radii"])[keep].sum())
    bad += int((np.asarray(got["tiles"]).astype(np.int64) != ref["tiles"])[keep].sum())
    bad += int((g[:, G_RADIUS] != ref["radii"].astype(F32))[keep].sum())
    bad += int((ints(g[:, G_TILES]) != ref["tiles"].astype(np.int32))[keep].sum())
    bad += int((ints(g[:, G_RECT:G_RECT + 4]) != ref["rect"])[keep].sum())
    bad += int((ints(g[:, G_CLAMP]) != ref["clampbits"].astype(np.int32))[keep].sum())
    culled = keep & ~ref["visible"]
    bad += int((g[culled].view(np.uint32) != 0).sum())
    bad += int((np.asarray(got["offsets"]).astype(np.int64) != np.cumsum(np.asarray(got["tiles"]).astype(np.int64))).sum())
    return res, bad


def compare_backward(got, ref, keep=None):
    """gradients against a backward reference -> ({name: (largest error / (K bound), elements beyond)}, exact mismatches: d_means2D,
    d_colors)"""
    vis = ref["visible"] if keep is None else ref["visible"] & keep
    res = {}
    for name in GRADS:
        if name in ref:
            m = vis.reshape((-1,) + (1,) * (ref[name].ndim - 1))
            if name == "d_shs":
                m = m & ref["sh_written"]
            res[name] = ratio(got[name], ref[name], K[name] * ref[name + "_bound"], m)
    bad = int((np.asarray(got["d_means2D"], dtype=F32).view(np.uint32) != ref["d_means2D"].view(np.uint32))[vis].sum())
    if ref["d_colors"] is not None:
        bad += int((np.asarray(got["d_colors"], dtype=F32).view(np.uint32) != ref["d_colors"].view(np.uint32))[vis].sum())
    return res, bad


def rejected(res):
    return any(r[1] > 0 for r in res[0].values()) or res[1] > 0
