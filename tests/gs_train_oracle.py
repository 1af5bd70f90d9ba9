"""fp64 references with PER-ELEMENT first-order fp32 error bounds of the trainer-step kernels of csrc/gs_train.hip (cut3r_gs_activate,
cut3r_gs_activate_backward, cut3r_gs_adam, cut3r_gs_pose_step, cut3r_gs_map_coef, cut3r_gs_refine_coef) and of cut3r_normal_agree_forward /
_backward and cut3r_gs_densify_stats (csrc/gs.hip).  CPU only (numpy); shared by tests/test_gs_train_cpu.py and tests/test_gs_train_gpu.py.
Not collected by pytest.

Every function here is written once over the numbers of tests/gs_render_oracle.py (EV: fp64 with a bound, or fp32 in the kernel's order
of operations: the restatement) and, for the pose step, over the duals of tests/gs_project_oracle.py (Dual<6> of csrc/lie_math.h through
se3_exp).  Integer and pass-through outputs are exact.  Error model beyond EV's: expf carries the project's 2 u (EV.exp); sinf / cosf the
same; powf and the sqrtf of the Adam denominators, whose device error nobody has measured, ONE unit in the last place each (2 u |value|);
a sum over Gaussians or pixels that goes through a wave tree and one atomic per workgroup carries u (6 + workgroups) sum |term| on top of
its terms' own bounds.

The isotropy term's signs: sign(s_k - mean) is a decision; a Gaussian whose s_k lies within MARGIN x the error of the mean is
`ambiguous` -- except for three bit-equal scales, where all three signs agree whatever they are and a_k - mean(a) is exactly 0.

The constants K = max(1, 2 RATIO), RATIO = the worst |fp32 restatement - reference| / bound over the cases of tests/test_gs_train_cpu.py
plus 0.05, rounded up to a decimal (the rule of tests/gs_render_oracle.py):

  group       measured (worst case of)                     RATIO  K     what it covers
  activate    0.685  (P = 257, opacity)                    0.8   1.6    means, scales, rots, opac of cut3r_gs_activate
  gtheta      0.998  (P = 257, accumulated d_shs)          1.1   2.2    gtheta of cut3r_gs_activate_backward (pre-fill + one addend: one rounding)
  pose_sums   0.120  (P = 1)                               0.2   1.0    the 16 pose sums
  adam        0.990  (P = 300, first call, theta)          1.1   2.2    theta, m, v of cut3r_gs_adam over six calls
  pose_step   0.569  (step 2, fold 1)                      0.7   1.4    pose_state[0:26] of cut3r_gs_pose_step
  coef        0.564  (refine loss)                         0.7   1.4    cut3r_gs_map_coef, cut3r_gs_refine_coef
  normal_sum  0.004  (3 x 3)                               0.1   1.0    cut3r_normal_agree_forward
  g_nrm       0.348  (37 x 50)                             0.4   1.0    grad_normal of cut3r_normal_agree_backward
  g_d         0.229  (37 x 50)                             0.3   1.0    grad_depth of cut3r_normal_agree_backward
  densify     0.989  (P = 257)                             1.1   2.2    cut3r_gs_densify_stats (a single addition: one rounding)
  The kernels on an MI355X against K x bound, and what that says about powf / sqrtf: see the docstring of tests/test_gs_train_gpu.py.
"""
import numpy as np

from tests import gs_project_oracle as PO
from tests.gs_render_oracle import EV, F32, F64, MARGIN, U, ratio

RATIO = {"activate": 0.8, "gtheta": 1.1, "pose_sums": 0.2, "adam": 1.1, "pose_step": 0.7, "coef": 0.7, "normal_sum": 0.1, "g_nrm": 0.4,
         "g_d": 0.3, "densify": 1.1}
K = {name: max(1.0, 2.0 * r) for name, r in RATIO.items()}
SERIES_X2 = float(F32(0.09))


# ------------------------------------------------------------------------------------------------------------------ numbers
def _ev(a, f32):
    a = np.asarray(a, dtype=F32).astype(F32 if f32 else F64)
    return EV(a, None if f32 else np.zeros(a.shape))


def _unary(x, f, dabs, ulps=1.0):
    """f(x) of a device function that is good to `ulps` units in the last place (fp32 mode: the correctly rounded value)"""
    if x.e is None:
        return EV(f(x.v.astype(F64)).astype(F32))
    v = f(x.v)
    return EV(v, dabs(x.v) * x.e + 2.0 * ulps * U * np.abs(v))


def _sqrt1(x):
    """sqrtf modelled as one unit in the last place"""
    r = x.sqrt()
    if r.e is not None:
        r = EV(r.v, np.where((r.e == 0) & (r.v * r.v == x.v), 0.0, r.e + U * np.abs(r.v)))
    return r


def _pow1(base, n, f32):
    """powf(base, n) of exact arguments, one unit in the last place"""
    v = np.power(np.float64(F32(base)), np.float64(n))
    return EV(np.asarray([v], dtype=F64).astype(F32), None) if f32 else EV(np.asarray([v]), np.asarray([2.0 * U * abs(v)]))


def _sin(cx, x):
    if isinstance(x, PO.Dual):
        return PO.Dual(_sin(cx, x.v), None if x.d is None else _cos(cx, x.v) * x.d)
    return _unary(x, np.sin, lambda t: np.abs(np.cos(t)))


def _cos(cx, x):
    if isinstance(x, PO.Dual):
        return PO.Dual(_cos(cx, x.v), None if x.d is None else (-_sin(cx, x.v)) * x.d)
    return _unary(x, np.cos, lambda t: np.abs(np.sin(t)))


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _qmul(a, b):                                                            # (x, y, z, w)
    return [a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0],
            a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]]


def _qconj(a):
    return [-a[0], -a[1], -a[2], a[3]]


def _qrot(q, v, two):
    u = q[:3]
    uv = _cross(u, v)
    uuv = _cross(u, uv)
    s = two * q[3]
    return [v[i] + (s * uv[i] + two * uuv[i]) for i in range(3)]


def se3_exp(cx, tau, phi):
    """se3_exp of csrc/lie_math.h over the numbers of `cx` (one element): -> t [3], q [4] (x, y, z, w)"""
    c = cx.const
    th2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]
    t2 = float(PO.val(th2)[0])
    if t2 < float(F32(1e-6)) ** 2:
        th4 = th2 * th2
        imag = c(0.5) - th2 * c(cx.k(1.0 / 48.0)) + th4 * c(cx.k(1.0 / 3840.0))
        real = c(1.0) - th2 * c(cx.k(1.0 / 8.0)) + th4 * c(cx.k(1.0 / 384.0))
    else:
        th = cx.sqrt(th2)
        imag = _sin(cx, th * c(0.5)) / th
        real = _cos(cx, th * c(0.5))
    q = [imag * phi[0], imag * phi[1], imag * phi[2], real]
    if t2 < SERIES_X2:
        a = c(0.5) + th2 * (c(cx.k(-1.0 / 24.0)) + th2 * (c(cx.k(1.0 / 720.0)) + th2 * c(cx.k(-1.0 / 40320.0))))
        b = c(cx.k(1.0 / 6.0)) + th2 * (c(cx.k(-1.0 / 120.0)) + th2 * (c(cx.k(1.0 / 5040.0)) + th2 * c(cx.k(-1.0 / 362880.0))))
    else:
        th = cx.sqrt(th2)
        sh = _sin(cx, th * c(0.5))
        a = c(2.0) * sh * sh / th2
        b = (th - _sin(cx, th)) / (th2 * th)
    pt = _cross(phi, tau)
    ppt = _cross(phi, pt)
    return [tau[i] + (a * pt[i] + b * ppt[i]) for i in range(3)], q


def _pose(ps, f32):
    """load_pose: the view's pose (t [3], q [4]) = exp(increment) * base, and the base (tT, qT), as one-element EVs"""
    cx = PO.Ctx(1, f32)
    e = [_ev([v], f32) for v in np.asarray(ps, dtype=F32)[:13]]
    tT, qT = e[0:3], e[3:7]
    tE, qE = se3_exp(cx, e[7:10], e[10:13])
    two = cx.const(2.0)
    q = _qmul(qE, qT)
    t = [a + b for a, b in zip(_qrot(qE, tT, two), tE)]
    return t, q, tT, qT, two


def _norm_quat(th, f32):
    """F.normalize of theta's quaternion (r, x, y, z at 10..13) -> gq (x, y, z, w), inv"""
    qr, qx, qy, qz = (_ev(th[:, 10 + i], f32) for i in range(4))
    n = (qr * qr + qx * qx + qy * qy + qz * qz).sqrt()
    floor = float(F32(1e-12))
    n = EV(np.maximum(n.v, n.v.dtype.type(floor)), None if f32 else np.where(n.v < floor, 0.0, n.e))
    inv = 1.0 / n
    return [qx * inv, qy * inv, qz * inv, qr * inv], inv


# ------------------------------------------------------------------------------------------------------------------ activate
def activate(theta, ps, f32=False):
    """cut3r_gs_activate -> dict(means [P,3], scales [P,3], rots [P,4], opac [P]) of EV, shs [P,3] exact"""
    th = np.ascontiguousarray(theta, dtype=F32)
    with np.errstate(all="ignore"):
        t, q, _, _, two = _pose(ps, f32)
        x = [_ev(th[:, i], f32) for i in range(3)]
        pc = [a + b for a, b in zip(_qrot(q, x, two), t)]
        opac = 1.0 / (1.0 + (-_ev(th[:, 6], f32)).exp())
        sc = [_ev(th[:, 7 + i], f32).exp() for i in range(3)]
        gq, _ = _norm_quat(th, f32)
        c = _qmul(q, gq)
    st = lambda cols: EV(np.stack([a.v for a in cols], 1), None if f32 else np.stack([np.broadcast_to(a.e, a.v.shape) for a in cols], 1))
    return dict(means=st(pc), scales=st(sc), rots=st([c[3], c[0], c[1], c[2]]), opac=opac, shs=th[:, 3:6].copy())


def activate_backward(theta, ps, d, radii, iso_coef, gtheta0, sums0, f32=False, mutants=()):
    """cut3r_gs_activate_backward: d = dict(means, scales, rots, opac, shs) gradients; gtheta0 [P,14] / sums0 [16] the pre-filled values
    (None: that output is not asked for) -> dict(gtheta EV [P,14], sums EV [16], ambiguous [P], nvis)"""
    th = np.ascontiguousarray(theta, dtype=F32)
    P = th.shape[0]
    g = lambda k: np.ascontiguousarray(d[k], dtype=F32).reshape(P, -1)
    res = dict(ambiguous=np.zeros(P, dtype=bool))
    with np.errstate(all="ignore"):
        t, q, tT, qT, two = _pose(ps, f32)
        gm = [_ev(g("means")[:, i], f32) for i in range(3)]
        gq, inv = _norm_quat(th, f32)
        gr = g("rots")
        gc = [_ev(gr[:, 1], f32), _ev(gr[:, 2], f32), _ev(gr[:, 3], f32), _ev(gr[:, 0], f32)]
        if gtheta0 is not None:
            o = [None] * 14
            o[0:3] = _qrot(_qconj(q), gm, two)
            o[3:6] = [_ev(g("shs")[:, i], f32) for i in range(3)]
            sg = 1.0 / (1.0 + (-_ev(th[:, 6], f32)).exp())
            o[6] = _ev(g("opac")[:, 0], f32) * sg * (1.0 - sg)
            s = [_ev(th[:, 7 + i], f32).exp() for i in range(3)]
            iso = [None, None, None]
            if iso_coef != 0.0:
                vis = np.asarray(radii) > 0
                nvis = float(vis.sum())
                res["nvis"] = nvis
                third = _ev(np.full(P, F32(1.0) / F32(3.0)), f32)
                mean = (s[0] + s[1] + s[2]) * third
                a = []
                for k in range(3):
                    diff = s[k].v - mean.v
                    a.append(_ev(np.where(diff > 0, 1.0, np.where(diff < 0, -1.0, 0.0)), f32))
                    if not f32:
                        res["ambiguous"] |= vis & (np.abs(diff) < MARGIN * (s[k].e + mean.e))
                # three bit-equal scales: the three signs agree, whichever they are, and (3 a) * (1 / 3.f) rounds to a: exactly 0
                equal = (th[:, 7] == th[:, 8]) & (th[:, 8] == th[:, 9])
                res["ambiguous"] &= ~equal
                am = (a[0] + a[1] + a[2]) * third
                denom = max(3.0 * nvis, 1.0)
                cc = _ev(np.full(P, F32(iso_coef)), f32) / _ev(np.full(P, F32(denom)), f32)
                zero = _ev(np.zeros(P), f32)
                iso = [(cc * (a[k] - am)).where(vis & ~equal, zero) for k in range(3)]
            for k in range(3):
                gs = _ev(g("scales")[:, k], f32)
                o[7 + k] = (gs + iso[k] if iso[k] is not None else gs) * s[k]
            gh = _qmul(_qconj(q), gc)
            dot = gh[0] * gq[0] + gh[1] * gq[1] + gh[2] * gq[2] + gh[3] * gq[3]
            o[10] = (gh[3] - gq[3] * dot) * inv
            for k in range(3):
                o[11 + k] = (gh[k] - gq[k] * dot) * inv
            pre = np.ascontiguousarray(gtheta0, dtype=F32)
            o = [_ev(pre[:, k], f32) + o[k] for k in range(14)]
            res["gtheta"] = EV(np.stack([np.broadcast_to(a.v, (P,)) for a in o], 1), None if f32 else np.stack([np.broadcast_to(a.e, (P,)) for a in o], 1))
        if sums0 is not None:
            y = [a + b for a, b in zip(_qrot(qT, [_ev(th[:, i], f32) for i in range(3)], two), tT)]
            acc = [gm[a] * y[b] for a in range(3) for b in range(3)] + gm + _qmul(gc, _qconj(_qmul(qT, gq)))
            groups = (P + 255) // 256
            dt = F32 if f32 else F64
            v = np.array([np.broadcast_to(a.v, (P,)).sum(dtype=dt) for a in acc], dtype=dt)
            pre = np.ascontiguousarray(sums0, dtype=F32).astype(dt)
            tot = (pre + v).astype(dt)
            if f32:
                res["sums"] = EV(tot)
            else:
                mag = np.array([np.abs(np.broadcast_to(a.v, (P,))).sum() for a in acc])
                err = np.array([np.broadcast_to(a.e, (P,)).sum() for a in acc])
                res["sums"] = EV(tot, err + U * (6.0 + groups) * (mag + np.abs(pre)) + U * np.abs(tot))
    return res


# ------------------------------------------------------------------------------------------------------------------ Adam
def adam(theta, m, v, grad, lr14, b1, b2, bc1, bc2, eps, f32=False, mutants=()):
    """one cut3r_gs_adam step on EV state (theta, m, v: EV or fp32 arrays) -> (theta, m, v) EV"""
    lift = lambda a: a if isinstance(a, EV) else _ev(a, f32)
    theta, m, v = lift(theta), lift(m), lift(v)
    n = theta.v.shape[0]
    dt = F32 if f32 else F64
    c = lambda x: dt(F32(x))
    g = _ev(grad, f32)
    one_b1, one_b2 = dt(F32(1.0) - F32(b1)), dt(F32(1.0) - F32(b2))
    idx = np.arange(n)
    lr = np.asarray(lr14, dtype=F32)[((idx % 256) % 14) if "mod_per_block" in mutants else (idx % 14)]
    with np.errstate(all="ignore"):
        mi = m * c(b1) + g * one_b1
        vi = v * c(b2) + g * one_b2 * g
        den = (_sqrt1(vi) / c(bc2) if "bc2_outside_root" in mutants else _sqrt1(vi / c(bc2))) + c(eps)
        step = _ev(lr, f32) * (mi / c(bc1)) / den
        new = theta - step
    return new, mi, vi


# ------------------------------------------------------------------------------------------------------------------ pose step
def pose_step(ps, sums, prior, ratio_value, lr_rot, lr_trans, fold, f32=False, mutants=()):
    """cut3r_gs_pose_step -> EV [32] (entries 26..31 untouched, exact)"""
    ps = np.asarray(ps, dtype=F32)
    dt = F32 if f32 else F64
    c1 = lambda x: _ev([x], f32)
    out = [c1(x) for x in ps]
    if "fold_first" in mutants and fold:
        out = _fold(out, f32)
    with np.errstate(all="ignore"):
        if fold != 2:
            cx = PO.Ctx(1, f32, 6)
            inc = [cx.seed(out[7 + k].v, k) for k in range(6)]
            tE, qE = se3_exp(cx, inc[0:3], inc[3:6])
            one, two = cx.const(1.0), cx.const(2.0)
            x, y, z, w = qE
            R = [one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w), two * (x * y + z * w), one - two * (x * x + z * z),
                 two * (y * z - x * w), two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]
            pc = dt(F32(prior)) * (dt(F32(2.0) - F32(ratio_value)) if ratio_value is not None else dt(1.0))
            pc = dt(F32(pc))
            s = [c1(v) for v in np.asarray(sums, dtype=F32)]
            terms = R + tE + qE
            step = float(ps[25]) + 1.0
            bc1, bc2 = 1.0 - _pow1(0.9, step, f32), 1.0 - _pow1(0.999, step, f32)
            b1, b2 = dt(F32(0.9)), dt(F32(0.999))
            ob1, ob2 = dt(F32(1.0) - F32(0.9)), dt(F32(1.0) - F32(0.999))
            for k in range(6):
                a = None
                for e in range(16):
                    dk = terms[e].d
                    if dk is None:
                        continue
                    tk = EV(dk.v[k], None if f32 else dk.e[k]) * s[e]
                    a = tk if a is None else a + tk
                gk = a + (dt(2.0) * pc) * out[7 + k]
                m = out[13 + k] * b1 + gk * ob1
                v = out[19 + k] * b2 + gk * ob2 * gk
                swap = "lr_swapped" in mutants
                lr = dt(F32(lr_trans if (k < 3) != swap else lr_rot))
                out[7 + k] = out[7 + k] - ((lr / bc1) * m) / (_sqrt1(v) / _sqrt1(bc2) + dt(F32(1e-8)))
                out[13 + k], out[19 + k] = m, v
            out[25] = c1(step)
        if fold and "fold_first" not in mutants:
            out = _fold(out, f32)
    return EV(np.array([float(a.v[0]) for a in out], dtype=dt), None if f32 else np.array([float(a.e[0]) for a in out]))


def _fold(out, f32):
    cx = PO.Ctx(1, f32)
    tE, qE = se3_exp(cx, out[7:10], out[10:13])
    two = cx.const(2.0)
    t = [a + b for a, b in zip(_qrot(qE, out[0:3], two), tE)]
    q = _qmul(qE, out[3:7])
    return t + q + [_ev([0.0], f32) for _ in range(6)] + out[13:]


# ------------------------------------------------------------------------------------------------------------------ coefficients
def map_coef(sums, w_rgb, w_depth, w_normal, g, H, W, loss0, f32=False, mutants=()):
    """cut3r_gs_map_coef -> (coef EV [3], loss EV [1] or None)"""
    s = [_ev([x], f32) for x in np.asarray(sums, dtype=F32)]
    dt = F32 if f32 else F64
    c = lambda x: _ev([x], f32)
    hw = c(F32(H) * F32(W))
    nd = s[3] if "nd_not_floored" in mutants else EV(np.maximum(s[3].v, dt(1.0)), s[3].e)
    with np.errstate(all="ignore"):
        den = hw * dt(3.0)
        coef = [c(g) * c(w_rgb) / den, c(g) * c(w_depth) / nd, c(g) * c(w_normal) / nd]
        loss = None
        if loss0 is not None:
            loss = c(loss0) + c(g) * (c(w_rgb) * s[0] / den + (c(w_depth) * s[1] + c(w_normal) * s[2]) / nd)
    return _stack(coef, f32), loss


def refine_coef(sums, g_rgb, g_var, H, W, loss0, f32=False, mutants=()):
    """cut3r_gs_refine_coef -> (coef EV [3], ratio EV [1], loss EV [1] or None)"""
    s = [_ev([x], f32) for x in np.asarray(sums, dtype=F32)]
    dt = F32 if f32 else F64
    c = lambda x: _ev([x], f32)
    hw = c(F32(H) * F32(W))
    fl = lambda a: a if "nd_not_floored" in mutants else EV(np.maximum(a.v, dt(1.0)), a.e)
    na, nm = fl(s[1]), fl(s[4])
    with np.errstate(all="ignore"):
        rat, mean = s[1] / hw, s[2] / nm
        coef = [c(g_rgb) * rat / (na * dt(3.0)), c(g_var) * rat / nm, mean]
        loss = None
        if loss0 is not None:
            loss = c(loss0) + (c(g_rgb) * rat * s[0] / (na * dt(3.0)) + c(g_var) * rat * (s[3] / nm - mean * mean))
    return _stack(coef, f32), rat, loss


def _stack(cols, f32):
    return EV(np.concatenate([a.v for a in cols]), None if f32 else np.concatenate([np.broadcast_to(a.e, a.v.shape) for a in cols]))


# ------------------------------------------------------------------------------------------------------------------ normal agreement
def _roll(a, dy, dx):
    return EV(np.roll(a.v, (dy, dx), (0, 1)), None if a.e is None else np.roll(np.broadcast_to(a.e, a.v.shape), (dy, dx), (0, 1)))


def _normal_parts(depth, H, W, cam, f32, border=False):
    """per pixel q: the central differences dx, dy of the back-projected depth, c = dx x dy, its length; `inner`: the pixels that have them"""
    fx, fy, cx, cy = (F32(v) for v in cam)
    d = _ev(np.asarray(depth, dtype=F32).reshape(H, W), f32)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    full = lambda v: _ev(np.full((H, W), v), f32)
    rx, ry = (_ev(xs, f32) - full(cx)) / full(fx), (_ev(ys, f32) - full(cy)) / full(fy)          # ((float) x - cx) / fx
    one = _ev(np.ones((H, W)), f32)
    P3 = [rx * d, ry * d, one * d]
    dxv = [_roll(p, 0, -1) - _roll(p, 0, 1) for p in P3]
    dyv = [_roll(p, -1, 0) - _roll(p, 1, 0) for p in P3]
    c = _cross(dxv, dyv)
    ln = (c[0] * c[0] + c[1] * c[1] + c[2] * c[2]).sqrt()
    inner = np.ones((H, W), bool) if border else (xs > 0) & (xs < W - 1) & (ys > 0) & (ys < H - 1)
    return dict(dx=dxv, dy=dyv, c=c, len=ln, inner=inner, ray=[rx, ry, one])


def normal_agree_forward(normal, depth, H, W, cam, f32=False, mutants=()):
    """cut3r_normal_agree_forward -> (sum EV [1], ambiguous pixels [H,W]: |c| within MARGIN x its error of 1e-12)"""
    n = np.asarray(normal, dtype=F32).reshape(3, H, W)
    dt = F32 if f32 else F64
    floor = float(F32(1e-12))
    with np.errstate(all="ignore"):
        p = _normal_parts(depth, H, W, cam, f32, "border_normal" in mutants)
        ln = EV(np.maximum(p["len"].v, dt(floor)), None if f32 else np.where(p["len"].v < floor, 0.0, p["len"].e))
        il = 1.0 / ln
        dot = (p["c"][0] * _ev(n[0], f32) + p["c"][1] * _ev(n[1], f32) + p["c"][2] * _ev(n[2], f32)) * il
        v = 1.0 - dot
    tv = np.where(p["inner"], v.v, dt(1.0)).astype(dt)
    tot = tv.sum(dtype=dt)
    if f32:
        return EV(np.array([tot], dtype=F32)), None
    amb = p["inner"] & (np.abs(p["len"].v - floor) < MARGIN * p["len"].e)
    groups = (H * W + 255) // 256
    err = np.where(p["inner"], v.e, 0.0).sum() + U * (6.0 + groups) * np.abs(tv).sum()
    return EV(np.array([tot]), np.array([err])), amb


def normal_agree_backward(normal, depth, H, W, cam, coef, g_d0, f32=False, mutants=()):
    """cut3r_normal_agree_backward -> (g_nrm EV [3,H,W], g_d EV [H,W] = g_d0 + gathered gradient)"""
    n = np.asarray(normal, dtype=F32).reshape(3, H, W)
    dt = F32 if f32 else F64
    floor = float(F32(1e-12))
    cf = dt(F32(coef))
    with np.errstate(all="ignore"):
        p = _normal_parts(depth, H, W, cam, f32, "border_normal" in mutants)
        ln = EV(np.maximum(p["len"].v, dt(floor)), None if f32 else np.where(p["len"].v < floor, 0.0, p["len"].e))
        il = 1.0 / ln
        zero = _ev(np.zeros((H, W)), f32)
        gn = [((-cf) * p["c"][i] * il).where(p["inner"], zero) for i in range(3)]
        ok = p["inner"] & (p["len"].v > floor)
        il2 = 1.0 / EV(np.where(ok, p["len"].v, dt(1.0)), p["len"].e)
        nq = [p["c"][i] * il2 for i in range(3)]
        gq = [_ev(n[i], f32) for i in range(3)]
        ng = nq[0] * gq[0] + nq[1] * gq[1] + nq[2] * gq[2]
        h = [(-(gq[i] - nq[i] * ng)) * il2 for i in range(3)]
        g = None
        for k, (sx, sy) in enumerate(((-1, 0), (1, 0), (0, -1), (0, 1))):    # q = p + (sx, sy): bring q's quantities to p
            at = lambda a: _roll(a, -sy, -sx)
            okq = np.roll(ok, (-sy, -sx), (0, 1))
            dc = _cross(p["ray"], [at(a) for a in p["dy"]]) if k < 2 else _cross([at(a) for a in p["dx"]], p["ray"])
            hq = [at(a) for a in h]
            sgn = dt(1.0) if k in (0, 2) else dt(-1.0)
            term = (hq[0] * dc[0] + hq[1] * dc[1] + hq[2] * dc[2]) * (cf * sgn)
            term = term.where(okq, zero)
            g = term if g is None else EV.where(g + term, okq, g)
        out = _ev(np.asarray(g_d0, dtype=F32).reshape(H, W), f32) + g
    st = EV(np.stack([a.v for a in gn]), None if f32 else np.stack([np.broadcast_to(a.e, (H, W)) for a in gn]))
    return st, out


# ------------------------------------------------------------------------------------------------------------------ densification
def densify_stats(radii, d_means2D, max_radii, grad_accum, grad_abs, denom, f32=False):
    """cut3r_gs_densify_stats -> (max_radii exact fp32, grad_accum EV, grad_abs EV, denom EV)"""
    r = np.asarray(radii)
    vis = r > 0
    d = np.asarray(d_means2D, dtype=F32)
    gx, gy, gz = (_ev(d[:, i], f32) for i in range(3))
    with np.errstate(all="ignore"):
        acc = _ev(grad_accum, f32)
        acc = (acc + (gx * gx + gy * gy).sqrt()).where(vis, acc)
        ab = _ev(grad_abs, f32)
        ab = (ab + gz.abs()).where(vis, ab)
        dn = _ev(denom, f32)
        dn = (dn + 1.0).where(vis, dn)
    mr = np.where(vis, np.maximum(np.asarray(max_radii, dtype=F32), r.astype(F32)), np.asarray(max_radii, dtype=F32)).astype(F32)
    return mr, acc, ab, dn


def within(got, ref, name, keep=None):
    """(largest |got - ref| / (K bound), elements beyond)"""
    return ratio(got, ref.v, K[name] * ref.e, keep)


# ------------------------------------------------------------------------------------------------------------------ cases
SIZES = (1, 63, 64, 65, 257)
NORMAL_SIZES = ((3, 3), (2, 5), (37, 50))
NORMAL_CAM = (41.3, 39.7, 24.6, 18.2)
POSE_STEPS = (1, 2, 10, 1000)


def pose_state(step=1, seed=1):
    """a view: non-identity base pose, non-zero increment, non-zero Adam moments, `step` - 1 steps taken, entries 26..31 marked"""
    r = np.random.default_rng(seed)
    ps = np.zeros(32, dtype=F32)
    q = np.array([0.1, -0.2, 0.15, 0.95])
    ps[0:3], ps[3:7] = (0.3, -0.2, 0.5), q / np.linalg.norm(q)
    ps[7:13] = (0.02, -0.01, 0.03, 0.015, -0.02, 0.01)
    ps[13:19], ps[19:25] = r.normal(size=6) * 0.05, r.random(6) * 0.01 + 1e-4
    ps[25] = step - 1
    ps[26:32] = 7.0 + np.arange(6)
    return ps


def theta_case(P, seed=2):
    """opacity logits in +-20, log-scales in -10..1, quaternion norms 1e-13 / 0.5 / 3 in rows 0 / 1 / 2, three equal scales in row 3, two equal
    scales above the mean in row 4"""
    r = np.random.default_rng(seed + P)
    th = np.zeros((P, 14))
    th[:, 0:3], th[:, 3:6] = r.normal(size=(P, 3)), r.random((P, 3))
    th[:, 6], th[:, 7:10] = r.uniform(-20, 20, P), r.uniform(-10, 1, (P, 3))
    q = r.normal(size=(P, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    for i, nrm in enumerate((1e-13, 0.5, 3.0)):
        if i < P:
            q[i] *= nrm
    th[:, 10:14] = q
    if P > 4:
        th[3, 7:10], th[4, 7:10] = -2.0, (-1.0, -1.0, -3.0)
    return th.astype(F32)


def grads_case(P, seed=3):
    r = np.random.default_rng(seed + P)
    return dict(means=r.normal(size=(P, 3)).astype(F32), scales=r.normal(size=(P, 3)).astype(F32), rots=r.normal(size=(P, 4)).astype(F32),
                opac=r.normal(size=P).astype(F32), shs=r.normal(size=(P, 3)).astype(F32))


def radii_case(P, kind, seed=4):
    r = np.random.default_rng(seed + P)
    if kind == "none":
        return (-r.integers(0, 3, P)).astype(np.int32)
    rad = r.integers(-3, 12, P).astype(np.int32)
    rad[::5] = 0
    if P == 1:
        rad[0] = 7
    if P > 4:
        rad[3], rad[4] = 5, 6
    return rad


def adam_case(P, seed=5):
    """14 distinct learning rates, five gradients with every seventh entry zero throughout (those entries keep theta bit for bit)"""
    r = np.random.default_rng(seed + P)
    n = 14 * P
    lr = (10.0 ** -np.linspace(1.0, 4.0, 14)).astype(F32)
    grads = (r.normal(size=(5, n)) * np.exp(r.normal(size=(5, n)) * 2)).astype(F32)
    grads[:, ::7] = 0
    return dict(n=n, lr14=lr, theta=r.normal(size=n).astype(F32), grads=grads)


def adam_bc(step):
    return float(F32(1.0 - 0.9 ** step)), float(F32(1.0 - 0.999 ** step))


def normal_case(H, W, seed=6):
    r = np.random.default_rng(seed + H * W)
    depth = (1.0 + 2.0 * r.random((H, W))).astype(F32)
    if H > 20:
        depth[10:15, 20:26] = 0                                               # the cross product vanishes: that neighbour is skipped
    return (r.normal(size=(3, H, W))).astype(F32), depth, r.normal(size=(H, W)).astype(F32)


COEF_SUMS = {"map": ((12.5, 3.25, 1.75, 40.0), (12.5, 0.0, 0.0, 0.0)), "refine": ((9.5, 1500.0, -3.2, 2.1, 900.0), (0.0, 0.0, 0.0, 0.0, 0.0),
                                                                                   (9.5, 1500.0, 0.0, 0.0, 0.0))}


def densify_case(P):
    r = np.random.default_rng(9 + P)
    return (radii_case(P, "mixed"), r.normal(size=(P, 3)).astype(F32), (r.random(P) * 8).astype(F32), r.random(P).astype(F32),
            r.random(P).astype(F32), r.integers(0, 5, P).astype(F32))
