"""Lie kernels (csrc/lie_math.h through lie.hip and gs_train.hip) against the fp64 oracle (oracle/lie_oracle.py) where the SE3 / Sim3
coefficient functions change from their Taylor series to their closed forms: rotation angles swept log-uniformly over [1e-5, 1e-1] (8 per
decade), points at 0.9x / 1.01x / 1.5x / 3x every switch the header has or had (theta = 1e-4, 1e-3, 0.3; |sigma| = 1e-4, 0.3), generic angles
0.5 / 2 / 3, each crossed with a translation drawn independently of the rotation, |tau| in {0, 1e-3, 1, 3}, and for Sim3 with 23 log-scales
from 0 to +-0.31.  A closed form that subtracts two nearly equal fp32 numbers is wrong by 1e-4..1e-3 |tau| in value and by 6e-4..1 |tau| in
gradient just above its switch; an O(1) translation makes that visible.

Bounds (set from the number format, not from what the kernels give): a well-conditioned fp32 evaluation is a few dozen operations at 2^-24,
about 1e-6 relative, so
    values     <= 1e-5 * max(1, |tau|)  absolute, on every matrix / tangent entry;
    gradients  <= 2e-4 * max(1, |tau|)  absolute, on every entry of the VJP of a cotangent with N(0, 1) entries.
Gradient references are central differences of the fp64 oracle with step 3e-5; the CPU tests below show that step against twice the step
(difference = 3 x the truncation error) and the logm-free forms used for speed against the oracle functions they stand for.

Every check prints, per angle decade, the worst error per unit max(1, |tau|) (see them with -s; a failure carries the table).
Measured on an MI355X, worst over all checks of a group, theta in [1e-5,1e-4) [1e-4,1e-3) [1e-3,1e-2) [1e-2,1e-1) [1e-1,pi):
    SO3   values 5.3e-8 6.0e-8 6.3e-8 9.0e-8 3.7e-7    gradients 4.2e-7 8.1e-7 5.6e-7 5.0e-7 7.2e-7
    SE3   values 1.5e-7 1.2e-7 1.1e-7 1.1e-7 3.9e-7    gradients 6.6e-7 7.0e-7 5.0e-7 8.1e-7 1.2e-6
    Sim3  values 3.6e-7 3.3e-7 4.4e-7 2.6e-7 6.7e-7    gradients 1.9e-6 3.7e-6 2.4e-6 2.7e-6 4.6e-6
(nothing within 3x of a bound).  With the coefficients as they were before the series switch moved to 0.3 -- closed forms from theta = 1e-4 /
1e-3 and |sigma| = 1e-4 -- the same checks gave: SE3 values 9.2e-5 / 2.1e-5 in the second / third decade, SE3 exp gradients 0.97 / 3.9e-2 /
1.6e-4, SE3 log gradient 3.1e-4 in the third decade and 2.6e-2 next to pi, Sim3 values up to 8.0e-4 and gradients up to 30 in every decade
(its small-angle closed forms in sigma cancel whatever theta is), the pose step's gradient up to 460 x its bound.  Guards, passing before and
after: every SO3 check, the SE3 log of the oracle's element, the SE3 composed loss value and its gradient to b, the Sim3 log value next to pi.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from cut3r_slam_amd.lietorch import SE3, SO3, Sim3
from oracle import lie_oracle as LO

gpu = pytest.mark.gpu
DEV = "cuda:0"
CLS = {0: SO3, 1: SE3, 2: Sim3}
GIDS = [0, 1, 2]
TDIM, DDIM = {0: 3, 1: 6, 2: 7}, {0: 4, 1: 7, 2: 8}
QOFF = {0: 0, 1: 3, 2: 3}                                             # where q_xyzw starts in the data layout

VAL_TOL, GRAD_TOL = 1e-5, 2e-4
FD_STEP = 3e-5

_SWITCHES = (1e-4, 1e-3, 0.3)                                         # theta: se3_coeffs / se3_log before, the common switch now
ANGLES = np.concatenate([np.logspace(-5, -1, 33), [f * t for t in _SWITCHES for f in (0.9, 1.01, 1.5, 3.0)], [0.5, 2.0, 3.0]])
TAU_NORMS = np.array([0.0, 1e-3, 1.0, 3.0])
_SIG = np.array([1e-6, 0.9e-4, 1.01e-4, 1.5e-4, 3e-4, 1e-3, 1e-2, 1e-1, 0.27, 0.3, 0.31])
SIGMAS = np.concatenate([[0.0], _SIG, -_SIG])
DECADES = [(1e-5, 1e-4), (1e-4, 1e-3), (1e-3, 1e-2), (1e-2, 1e-1), (1e-1, 4.0)]


# ------------------------------------------------------------------------------------------------ inputs
def _unit(g, n):
    v = g.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _points(gid, angles, tau_norms, sigmas, seed):
    """tangents [N, tdim]: (random unit direction x prescribed angle) x (independent random direction x |tau|) (x sigma)"""
    g = np.random.default_rng(seed)
    if gid == 0:
        th = np.asarray(angles, np.float64)
        return _unit(g, len(th)) * th[:, None], th, np.zeros_like(th), np.zeros_like(th)
    grids = np.meshgrid(angles, tau_norms, sigmas if gid == 2 else [0.0], indexing="ij")
    th, tn, sg = (x.ravel() for x in grids)
    a = np.concatenate([_unit(g, len(th)) * tn[:, None], _unit(g, len(th)) * th[:, None]], 1)
    if gid == 2:
        a = np.concatenate([a, sg[:, None]], 1)
    return a, th, tn, sg


def _sweep(gid):
    return _points(gid, ANGLES, TAU_NORMS, SIGMAS, 100 + gid)


def _generic(gid, n, seed):
    a = np.random.default_rng(seed).normal(0, 0.4, (n, TDIM[gid]))
    if gid == 2:
        a[:, 6] *= 0.3
    return a


# ------------------------------------------------------------------------------------------------ per-decade report
def _report(name, err, tol, th, tn, sg):
    """err [N]: worst absolute error of each point.  Prints the worst err / max(1, |tau|) of every angle decade and raises if one is above tol."""
    err, scale = np.asarray(err, np.float64), np.maximum(1.0, tn)
    rel = err / scale
    lines, bad = [], ~(rel <= tol)
    for lo, hi in DECADES:
        m = (th >= lo * 0.999) & (th < hi * 0.999)
        if not m.any():
            continue
        i = np.flatnonzero(m)[np.nanargmax(np.where(np.isnan(rel[m]), np.inf, rel[m]))]
        note = "ABOVE" if rel[i] > tol or np.isnan(rel[i]) else ("within 3x" if rel[i] * 3 > tol else "")
        lines.append(f"  theta [{lo:.0e},{hi:.0e}): worst {rel[i]:.2e} per max(1,|tau|) = {rel[i] / tol:.3f} of the bound {tol:.0e} "
                     f"(theta {th[i]:.3e} |tau| {tn[i]:g} sigma {sg[i]:g}); {int(bad[m].sum())}/{int(m.sum())} points above {note}")
    text = f"[{name}]\n" + "\n".join(lines)
    print(text)
    assert not bad.any(), f"{int(bad.sum())}/{len(err)} points above the bound\n{text}"


def _worst(x):
    return np.abs(x).reshape(len(x), -1).max(1)


# ------------------------------------------------------------------------------------------------ the kernels (numpy in, numpy out)
def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)


def _k_exp(gid, a):
    return CLS[gid].exp(_t(a)).data.cpu().numpy().astype(np.float64)


def _k_matrix(gid, d):
    return CLS[gid](_t(d)).matrix().cpu().numpy().astype(np.float64)


def _k_log(gid, d):
    return CLS[gid](_t(d)).log().cpu().numpy().astype(np.float64)


def _k_vjp_exp(gid, a, G):
    """gradient w.r.t. the tangent of sum(G * exp(a).data)"""
    x = _t(a).requires_grad_(True)
    (CLS[gid].exp(x).data * _t(G)).sum().backward()
    return x.grad.cpu().numpy().astype(np.float64)


def _k_vjp_exp_matrix(gid, a, G):
    """gradient w.r.t. the tangent of sum(G * exp(a).matrix())"""
    x = _t(a).requires_grad_(True)
    (CLS[gid].exp(x).matrix() * _t(G)).sum().backward()
    return x.grad.cpu().numpy().astype(np.float64)


def _k_vjp_log(gid, d, G):
    """gradient w.r.t. the data of sum(G * X.log())"""
    x = _t(d).requires_grad_(True)
    (CLS[gid](x).log() * _t(G)).sum().backward()
    return x.grad.cpu().numpy().astype(np.float64)


# ------------------------------------------------------------------------------------------------ fp64 references
def _data64(gid, A):
    return LO.matrix_to_data_batch(gid, LO.exp_matrix_batch(gid, A))


def _fd(f, A, h=FD_STEP):
    """central differences of f: [N, n] -> [N] in every coordinate -> [N, n]"""
    out = np.zeros_like(A)
    for j in range(A.shape[1]):
        e = np.zeros(A.shape[1])
        e[j] = h
        out[:, j] = (f(A + e) - f(A - e)) / (2 * h)
    return out


def _ref_vjp_exp(gid, A, G, h=FD_STEP):
    return _fd(lambda x: (G * _data64(gid, x)).sum(1), A, h)


def _ref_vjp_exp_matrix(gid, A, G, h=FD_STEP):
    return _fd(lambda x: (G * LO.exp_matrix_batch(gid, x)).sum((1, 2)), A, h)


def _ref_log_jacobian(gid, A, h=FD_STEP):
    """d log / d data [N, tdim, ddim] at data = exp(A), from central differences of the fp64 exp alone (logm costs milliseconds a call):
    log(exp(a)) = a for angles below pi gives  J_log J_exp = I  on the tangent space of the data manifold, and log does not depend on the length
    of the quaternion (the kernels' log and the oracle's data_to_matrix both normalise), so  J_log q_radial = 0  fixes the one direction left."""
    n, D = TDIM[gid], DDIM[gid]
    J = np.zeros((len(A), D, D))
    for j in range(n):
        e = np.zeros(n)
        e[j] = h
        J[:, :, j] = (_data64(gid, A + e) - _data64(gid, A - e)) / (2 * h)
    J[:, QOFF[gid]:QOFF[gid] + 4, n] = _data64(gid, A)[:, QOFF[gid]:QOFF[gid] + 4]
    return np.linalg.inv(J)[:, :n, :]


def _loss64(gid, A, B, Wm, pts):
    EA, EB = LO.exp_matrix_batch(gid, A), LO.exp_matrix_batch(gid, B)
    M, Mi = EA @ EB, np.linalg.inv(EA)
    act = np.einsum("nij,pj->npi", M[:, :3, :3], pts) + M[:, None, :3, 3]
    return (Wm * M).sum((1, 2)) + 0.1 * (act ** 2).sum((1, 2)) + 0.3 * (Wm.T * Mi).sum((1, 2))


# ------------------------------------------------------------------------------------------------ CPU: the references themselves
@pytest.mark.parametrize("gid", GIDS)
def test_fast_oracle_forms_equal_the_oracle(gid):
    """exp_matrix_batch / matrix_to_data_batch / adjoint_matrix_exact / the logm-free log Jacobian against exp_matrix, matrix_to_data,
    adjoint_matrix (numerical, logm) and central differences of log_tangent(data_to_matrix(.)) -- at band points and next to pi"""
    a, th, tn, sg = _points(gid, [3e-5, 2e-4, 1.5e-3, 2e-2, 0.5, 3.0, np.pi - 1e-3], [1e-3, 3.0], [0.0, 1.01e-4, -0.3], 7)
    E = LO.exp_matrix_batch(gid, a)
    D = LO.matrix_to_data_batch(gid, E)
    Jl = _ref_log_jacobian(gid, a)
    for i in range(len(a)):
        assert np.abs(E[i] - LO.exp_matrix(gid, a[i])).max() == 0.0
        assert np.abs(LO.data_to_matrix(gid, D[i]) - E[i]).max() < 1e-14 and D[i][QOFF[gid] + 3] >= 0
        assert np.abs(LO.log_tangent(gid, E[i]) - a[i]).max() < 1e-11 * max(1.0, tn[i])          # log(exp(a)) = a in the oracle itself
        assert np.abs(LO.adjoint_matrix_exact(gid, E[i]) - LO.adjoint_matrix(gid, E[i])).max() < 2e-8 * max(1.0, tn[i])
    for i in range(0, len(a), 3):
        Jfd = np.zeros_like(Jl[i])
        h = FD_STEP                                          # (pi - 1e-3: w = 5e-4, the perturbed quaternion stays on its side of the cut;
                                                             #  logm's own noise next to pi, ~1e-12, rules a much smaller step out)
        for j in range(DDIM[gid]):
            e = np.zeros(DDIM[gid])
            e[j] = h
            Jfd[:, j] = (LO.log_tangent(gid, LO.data_to_matrix(gid, D[i] + e)) - LO.log_tangent(gid, LO.data_to_matrix(gid, D[i] - e))) / (2 * h)
        assert np.abs(Jl[i] - Jfd).max() < 1e-7 * max(1.0, tn[i]), (th[i], tn[i], sg[i], np.abs(Jl[i] - Jfd).max())


@pytest.mark.parametrize("gid", GIDS)
def test_central_difference_step_truncation_is_below_1e_7(gid):
    """the references with step h and with 2h differ by 3x the truncation error of step h: below 1e-7 at every sweep point"""
    a, th, tn, sg = _sweep(gid)
    g = np.random.default_rng(50 + gid)
    worst = {}
    G = g.normal(size=(len(a), DDIM[gid]))
    worst["exp"] = _worst(_ref_vjp_exp(gid, a, G) - _ref_vjp_exp(gid, a, G, 2 * FD_STEP)) / 3
    G = g.normal(size=(len(a), 4, 4))
    worst["exp->matrix"] = _worst(_ref_vjp_exp_matrix(gid, a, G) - _ref_vjp_exp_matrix(gid, a, G, 2 * FD_STEP)) / 3
    G = g.normal(size=(len(a), 1, TDIM[gid]))
    worst["log"] = _worst(G @ _ref_log_jacobian(gid, a) - G @ _ref_log_jacobian(gid, a, 2 * FD_STEP)) / 3
    b, Wm, pts = _generic(gid, len(a), 60 + gid), g.normal(size=(4, 4)), g.uniform(-1, 1, (6, 3))
    fa = lambda h: _fd(lambda x: _loss64(gid, x, b, Wm, pts), a, h)
    fb = lambda h: _fd(lambda x: _loss64(gid, a, x, Wm, pts), b, h)
    worst["composed"] = np.maximum(_worst(fa(FD_STEP) - fa(2 * FD_STEP)), _worst(fb(FD_STEP) - fb(2 * FD_STEP))) / 3
    for k, v in worst.items():
        print(f"[fd truncation group {gid}] {k}: worst {v.max():.2e} (theta {th[v.argmax()]:.3e} |tau| {tn[v.argmax()]:g} sigma {sg[v.argmax()]:g})")
        assert v.max() < 1e-7, k


# ------------------------------------------------------------------------------------------------ GPU: values
@gpu
@pytest.mark.parametrize("gid", GIDS)
def test_exp_matrix_log_values_over_the_bands(gid):
    a, th, tn, sg = _sweep(gid)
    assert len(a) % 128 != 0                                                                    # (a partial last block)
    Mref = LO.exp_matrix_batch(gid, a)
    d = _k_exp(gid, a)
    _report(f"group {gid} exp(a).matrix() vs fp64 expm", _worst(_k_matrix(gid, d) - Mref), VAL_TOL, th, tn, sg)
    _report(f"group {gid} exp(a).log() vs a", _worst(_k_log(gid, d) - a), VAL_TOL, th, tn, sg)
    _report(f"group {gid} log of the fp64 oracle's element vs a", _worst(_k_log(gid, LO.matrix_to_data_batch(gid, Mref)) - a), VAL_TOL, th, tn, sg)


@gpu
@pytest.mark.parametrize("gid", GIDS)
def test_retr_and_adjoints_over_the_bands(gid):
    a, th, tn, sg = _sweep(gid)
    n = TDIM[gid]
    E = LO.exp_matrix_batch(gid, a)
    # retr: the band point is the increment, on a generic element
    x = _generic(gid, len(a), 70 + gid)
    R = CLS[gid].exp(_t(x)).retr(_t(a)).matrix().cpu().numpy()
    _report(f"group {gid} X.retr(a) = exp(a) X", _worst(R - E @ LO.exp_matrix_batch(gid, x)), VAL_TOL, th, tn, sg)
    # adjoints of the band element
    X = CLS[gid].exp(_t(a))
    eye = torch.eye(n, device=DEV)
    Ad = X[:, None].adj(eye[None]).cpu().numpy().transpose(0, 2, 1)                             # [N, :, j] = Ad e_j
    AdT = X[:, None].adjT(eye[None]).cpu().numpy().transpose(0, 2, 1)
    ref = np.stack([LO.adjoint_matrix_exact(gid, M) for M in E])
    _report(f"group {gid} adj", _worst(Ad - ref), VAL_TOL, th, tn, sg)
    _report(f"group {gid} adjT", _worst(AdT - ref.transpose(0, 2, 1)), VAL_TOL, th, tn, sg)


@gpu
@pytest.mark.parametrize("gid", GIDS)
def test_single_element_and_broadcast_act_at_band_angles(gid):
    a, th, tn, sg = _points(gid, [2e-4, 1.5e-3, 3e-2], [1.0, 3.0], [0.0, 3e-4, -1e-2], 11)
    d = _k_exp(gid, a)
    G = np.random.default_rng(12).normal(size=(len(a), 4, 4))
    grad = _k_vjp_exp_matrix(gid, a, G)
    for i in range(len(a)):                                                                      # n = 1 launches equal the batched ones
        assert np.array_equal(_k_exp(gid, a[i:i + 1])[0], d[i]) and np.array_equal(_k_log(gid, d[i:i + 1]), _k_log(gid, d)[i:i + 1])
        assert np.array_equal(_k_vjp_exp_matrix(gid, a[i:i + 1], G[i:i + 1])[0], grad[i])
    _report(f"group {gid} n = 1 exp->matrix gradient", _worst(grad - _ref_vjp_exp_matrix(gid, a, G)), GRAD_TOL, th, tn, sg)
    p = np.random.default_rng(13).uniform(-1, 1, (len(a), 5, 3))
    E = LO.exp_matrix_batch(gid, a)
    out = CLS[gid](_t(d))[:, None].act(_t(p)).cpu().numpy()
    _report(f"group {gid} X[:, None].act(points)", _worst(out - (np.einsum("nij,npj->npi", E[:, :3, :3], p) + E[:, None, :3, 3])), VAL_TOL, th, tn, sg)


# ------------------------------------------------------------------------------------------------ GPU: gradients
@gpu
@pytest.mark.parametrize("gid", GIDS)
def test_exp_and_log_vjp_over_the_bands(gid):
    a, th, tn, sg = _sweep(gid)
    g = np.random.default_rng(80 + gid)
    G = g.normal(size=(len(a), DDIM[gid]))
    _report(f"group {gid} VJP of exp", _worst(_k_vjp_exp(gid, a, G) - _ref_vjp_exp(gid, a, G)), GRAD_TOL, th, tn, sg)
    G = g.normal(size=(len(a), 4, 4))
    _report(f"group {gid} VJP of exp -> matrix", _worst(_k_vjp_exp_matrix(gid, a, G) - _ref_vjp_exp_matrix(gid, a, G)), GRAD_TOL, th, tn, sg)
    G = g.normal(size=(len(a), TDIM[gid]))
    ref = (G[:, None, :] @ _ref_log_jacobian(gid, a))[:, 0]
    _report(f"group {gid} VJP of log (at the fp64 oracle's element)", _worst(_k_vjp_log(gid, _data64(gid, a), G) - ref), GRAD_TOL, th, tn, sg)


@gpu
@pytest.mark.parametrize("gid", GIDS)
def test_exp_mul_matrix_act_inv_gradient_over_the_bands(gid):
    """the loss of test_lie_gpu.py's finite-difference test -- (exp(a) exp(b)).matrix(), its action on points, exp(a).inv().matrix() -- with a at
    every sweep point and b generic, gradients to both"""
    cls = CLS[gid]
    a, th, tn, sg = _sweep(gid)
    g = np.random.default_rng(90 + gid)
    b, Wm, pts = _generic(gid, len(a), 60 + gid), g.normal(size=(4, 4)), g.uniform(-1, 1, (6, 3))
    ta, tb = _t(a).requires_grad_(True), _t(b).requires_grad_(True)
    X, Y = cls.exp(ta), cls.exp(tb)
    Z = X * Y
    act = Z[:, None].act(_t(pts)[None])
    loss = (_t(Wm) * Z.matrix()).sum((1, 2)) + 0.1 * (act ** 2).sum((1, 2)) + 0.3 * (_t(Wm.T) * X.inv().matrix()).sum((1, 2))
    loss.sum().backward()
    ref = _loss64(gid, a, b, Wm, pts)
    _report(f"group {gid} composed loss value / max(1, |loss|)", np.abs(loss.detach().cpu().numpy() - ref) / np.maximum(1, np.abs(ref)), 2e-4, th,
            tn * 0, sg)
    _report(f"group {gid} composed gradient to a", _worst(ta.grad.cpu().numpy() - _fd(lambda x: _loss64(gid, x, b, Wm, pts), a)), GRAD_TOL, th, tn, sg)
    _report(f"group {gid} composed gradient to b", _worst(tb.grad.cpu().numpy() - _fd(lambda x: _loss64(gid, a, x, Wm, pts), b)), GRAD_TOL, th, tn, sg)


# ------------------------------------------------------------------------------------------------ GPU: log next to pi
@gpu
@pytest.mark.parametrize("gid", GIDS)
def test_log_next_to_pi_value_gradient_and_double_cover(gid):
    """angles pi - {1e-1, 1e-2, 1e-3} (w down to 5e-4): q and -q give the same tangent; value and gradient against fp64"""
    ang = np.repeat(np.pi - np.array([1e-1, 1e-2, 1e-3]), 3)
    a, th, tn, sg = _points(gid, ang, TAU_NORMS, [0.0, 0.2, -0.2], 21)
    d = _data64(gid, a)
    neg = np.ones(DDIM[gid])
    neg[QOFF[gid]:QOFF[gid] + 4] = -1.0
    assert (d[:, QOFF[gid] + 3] >= 0).all() and d[:, QOFF[gid] + 3].min() < 6e-4
    lp, ln = _k_log(gid, d), _k_log(gid, d * neg)
    assert np.array_equal(lp, ln), f"log(q) != log(-q): {np.abs(lp - ln).max():.3e}"
    _report(f"group {gid} log next to pi vs a", _worst(lp - a), VAL_TOL, th, tn, sg)
    G = np.random.default_rng(22).normal(size=(len(a), TDIM[gid]))
    ref = (G[:, None, :] @ _ref_log_jacobian(gid, a))[:, 0]
    _report(f"group {gid} VJP of log next to pi (w > 0)", _worst(_k_vjp_log(gid, d, G) - ref), GRAD_TOL, th, tn, sg)
    _report(f"group {gid} VJP of log next to pi (w < 0)", _worst(_k_vjp_log(gid, d * neg, G) - ref * neg), GRAD_TOL, th, tn, sg)


# ------------------------------------------------------------------------------------------------ GPU: the Gaussian mapper's pose step
def _pose_step_gradient64(tau, phi, sums):
    """d/d(tau, phi) of <R_E, M> + <t_E, s> + <q_E, r> with (t_E, q_E) = exp(tau, phi) (gs_pose_step_kernel's comment), fp64 autograd"""
    x = torch.tensor(np.concatenate([tau, phi]), dtype=torch.float64, requires_grad=True)
    S = torch.tensor(sums, dtype=torch.float64)
    t, p = x[:3], x[3:]
    z = torch.zeros((), dtype=torch.float64)
    K = torch.stack([torch.stack([z, -p[2], p[1], t[0]]), torch.stack([p[2], z, -p[0], t[1]]), torch.stack([-p[1], p[0], z, t[2]]),
                     torch.zeros(4, dtype=torch.float64)])
    T = torch.linalg.matrix_exp(K)
    th = p.norm()
    q = torch.cat([torch.sin(th / 2) / th * p, torch.cos(th / 2)[None]])
    ((T[:3, :3].reshape(9) * S[:9]).sum() + (T[:3, 3] * S[9:12]).sum() + (q * S[12:16]).sum()).backward()
    return x.grad.numpy()


@gpu
def test_gs_pose_step_gradient_at_band_increments():
    """cut3r_gs_pose_step alone, increments at band magnitudes: the first Adam step from zero moments leaves m = (1 - 0.9) g, which gives the
    gradient the kernel took through the dual numbers of se3_exp"""
    from cut3r_slam_amd import _lib
    lib = _lib.load()
    g = np.random.default_rng(31)
    one_minus_b1 = float(np.float32(1.0) - np.float32(0.9))              # as the kernel forms it
    rows = []
    for pn in (2e-4, 1e-3, 1e-2):
        for tnorm in (1e-3, 0.3):
            for scale in (1.0, 30.0):
                tau, phi = _unit(g, 1)[0] * tnorm, _unit(g, 1)[0] * pn
                sums = g.normal(0, scale, 16)
                ps = torch.zeros(32)
                ps[0:7] = torch.tensor([0.3, -0.2, 0.5, 0.0, 0.0, 0.0, 1.0])
                ps[7:10], ps[10:13] = torch.from_numpy(tau).float(), torch.from_numpy(phi).float()
                ps, ts = ps.to(DEV), _t(sums)
                assert lib.cut3r_gs_pose_step(C.c_void_p(ps.data_ptr()), C.c_void_p(ts.data_ptr()), 0.0, None, 0.0, 0.0, 0,
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
                out = ps.cpu().double().numpy()
                assert out[25] == 1.0 and np.array_equal(out[7:13], np.concatenate([tau, phi]).astype(np.float32).astype(np.float64))
                ref = _pose_step_gradient64(out[7:10], out[10:13], ts.cpu().double().numpy())
                got = out[13:19] / one_minus_b1
                bound = GRAD_TOL * max(1.0, tnorm) * np.abs(sums).max()
                rows.append((pn, tnorm, scale, np.abs(got - ref).max(), bound))
                np.testing.assert_allclose(out[19:25], (1.0 - 0.999) * got ** 2, rtol=1e-4, atol=1e-30)
    text = "\n".join(f"  |phi| {r[0]:.0e} |tau| {r[1]:g} sums x{r[2]:g}: gradient error {r[3]:.2e} = {r[3] / r[4]:.3f} of the bound {r[4]:.1e}" for r in rows)
    print("[gs_pose_step gradient vs fp64 autograd]\n" + text)
    assert all(r[3] <= r[4] for r in rows), text
