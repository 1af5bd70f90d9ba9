"""CPU: the reference-alone checks behind tests/gs_train_oracle.py.

  * the references equal plain fp64 restatements written another way (rotation matrices for the quaternion algebra, torch autograd for
    the rendered-normal term and for the pose gradient, the textbook Adam) at the fp64 level;
  * the fp32 restatements stay inside RATIO x the model bound (the table of the oracle's docstring is printed here);
  * mutants of the restatements are each REJECTED by the comparison the GPU test makes: `i % 14` taken per block, bc2 under the wrong
    root, the fold applied before the step, lr_rot / lr_trans swapped, border pixels given a depth normal, the valid-depth count not
    floored.  Two mutants of the isotropy term have no decidable input and are not among them: `sign(0) = 1` (a scale EQUAL to the mean of
    three unequal scales exists only by fp32 coincidence, which the reference calls ambiguous, and for three equal scales the signs cancel
    whatever they are) and `nvis` not floored (the term is evaluated for visible Gaussians only, that is when nvis >= 1)."""
import numpy as np
import pytest
import torch

from tests import gs_train_oracle as TO
from tests.gs_render_oracle import F32, F64

_WORST = {}


def _note(group, name, got, ref, keep=None):
    r, beyond = TO.ratio(got, ref.v, ref.e, keep)
    if r > _WORST.get(group, (0.0, ""))[0]:
        _WORST[group] = (r, name)
    return r


def _rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _se3_exp64(xi):
    """Rodrigues / the closed-form V matrix"""
    tau, phi = xi[:3], xi[3:]
    th = np.linalg.norm(phi)
    K = np.array([[0, -phi[2], phi[1]], [phi[2], 0, -phi[0]], [-phi[1], phi[0], 0]])
    R = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K
    V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * K + (th - np.sin(th)) / th ** 3 * K @ K
    return R, V @ tau


def _ham(a, b):
    """Hamilton product of (x, y, z, w) quaternions from the scalar / vector form"""
    av, bv = np.asarray(a[:3], dtype=F64), np.asarray(b[:3], dtype=F64)
    return np.concatenate([a[3] * bv + b[3] * av + np.cross(av, bv), [a[3] * b[3] - av @ bv]])


def _pose64(ps, inc=None):
    """exp(increment) * base as (R, t, q): the stored base quaternion is unit only to fp32, so the quaternions are multiplied, not the
    rotation matrices (v + 2 w u x v + 2 u x (u x v) is _rot(q) v for any q)"""
    xi = ps[7:13].astype(F64) if inc is None else np.asarray(inc, dtype=F64)
    th = np.linalg.norm(xi[3:])
    qE = np.concatenate([np.sin(th / 2) / th * xi[3:], [np.cos(th / 2)]])
    _, tE = _se3_exp64(xi)
    q = _ham(qE, ps[3:7].astype(F64))
    return _rot(q), _rot(qE) @ ps[0:3].astype(F64) + tE, q


@pytest.mark.parametrize("P", TO.SIZES)
def test_activate_reference_and_restatement(P):
    ps, th = TO.pose_state(), TO.theta_case(P)
    ref, f32 = TO.activate(th, ps), TO.activate(th, ps, True)
    R, t, qv = _pose64(ps)
    t64 = th.astype(F64)
    assert np.abs(ref["means"].v - (t64[:, 0:3] @ R.T + t)).max() < 1e-13
    assert np.allclose(ref["scales"].v, np.exp(t64[:, 7:10]), rtol=1e-14) and np.allclose(ref["opac"].v, 1 / (1 + np.exp(-t64[:, 6])), rtol=1e-14)
    q = t64[:, 10:14] / np.maximum(np.linalg.norm(t64[:, 10:14], axis=1, keepdims=True), float(F32(1e-12)))
    for i in range(min(P, 8)):                                              # the composed rotation is the product of the rotations
        r, x, y, z = ref["rots"].v[i]
        assert np.abs(np.array([x, y, z, r]) - _ham(qv, (q[i, 1], q[i, 2], q[i, 3], q[i, 0]))).max() < 1e-13 * max(1.0, np.linalg.norm(q[i]))
    assert np.array_equal(ref["shs"], th[:, 3:6])
    worst = max(_note("activate", f"P={P} {k}", f32[k].v, ref[k]) for k in ("means", "scales", "rots", "opac"))
    print(f"[gs train cpu] activate P {P}: restatement error / model bound {worst:.3f}")
    assert worst <= TO.RATIO["activate"]


def _activate_backward_args(P, iso, kind):
    return TO.theta_case(P), TO.pose_state(), TO.grads_case(P), TO.radii_case(P, kind), iso


@pytest.mark.parametrize("P", TO.SIZES)
@pytest.mark.parametrize("iso,kind", ((0.0, "mixed"), (4.0, "mixed"), (4.0, "none")))
def test_activate_backward_reference_and_restatement(P, iso, kind):
    th, ps, d, rad, iso = _activate_backward_args(P, iso, kind)
    g0, s0 = np.full((P, 14), 0.25, dtype=F32), np.arange(16, dtype=F32)
    ref, f32 = TO.activate_backward(th, ps, d, rad, iso, g0, s0), TO.activate_backward(th, ps, d, rad, iso, g0, s0, True)
    keep = ~ref["ambiguous"]
    assert ref["ambiguous"].mean() <= 0.02
    # the chain rule written another way: finite-difference-free check of the linear parts
    R = _pose64(ps)[0]
    assert np.abs(ref["gtheta"].v[:, 0:3] - 0.25 - d["means"].astype(F64) @ R).max() < 1e-12
    sg = 1 / (1 + np.exp(-th[:, 6].astype(F64)))
    assert np.allclose(ref["gtheta"].v[:, 6] - 0.25, d["opac"] * sg * (1 - sg), rtol=1e-13, atol=1e-15)
    if iso == 0.0 or kind == "none":
        assert np.allclose(ref["gtheta"].v[:, 7:10] - 0.25, d["scales"] * np.exp(th[:, 7:10].astype(F64)), rtol=1e-13, atol=1e-15)
    elif P > 4:
        nvis = (rad > 0).sum()
        s = np.exp(th[4, 7:10].astype(F64))
        want = (d["scales"][4] + 4.0 / (3 * nvis) * (np.array([1.0, 1.0, -1.0]) - 1.0 / 3.0)) * s     # two equal scales above the mean
        assert np.allclose(ref["gtheta"].v[4, 7:10] - 0.25, want, rtol=1e-7)
        assert np.allclose(ref["gtheta"].v[3, 7:10] - 0.25, d["scales"][3] * np.exp(-2.0), rtol=1e-13)  # three equal scales: no isotropy term
    a = _note("gtheta", f"P={P} iso={iso} {kind}", f32["gtheta"].v, ref["gtheta"], keep[:, None])
    b = _note("pose_sums", f"P={P}", f32["sums"].v, ref["sums"])
    print(f"[gs train cpu] activate_backward P {P} iso {iso} radii {kind}: gtheta {a:.3f}, pose sums {b:.3f}, ambiguous {int(ref['ambiguous'].sum())}")
    assert a <= TO.RATIO["gtheta"] and b <= TO.RATIO["pose_sums"]
    only = TO.activate_backward(th, ps, d, rad, iso, None, s0)
    assert "gtheta" not in only and np.array_equal(only["sums"].v, ref["sums"].v)


def test_adam_reference_and_restatement():
    for P in (1, 19, 300):
        c = TO.adam_case(P)
        n = c["n"]
        t, m, v = c["theta"], np.zeros(n, dtype=F32), np.zeros(n, dtype=F32)
        t2, m2, v2 = t, m, v
        t64, m64, v64 = t.astype(F64), np.zeros(n), np.zeros(n)
        lr = np.tile(c["lr14"].astype(F64), P)
        for k, step in enumerate((1, 2, 3, 4, 5, 1000)):
            g = c["grads"][k % 5]
            bc1, bc2 = TO.adam_bc(step)
            t, m, v = TO.adam(t, m, v, g, c["lr14"], 0.9, 0.999, bc1, bc2, 1e-15)
            t2, m2, v2 = TO.adam(t2, m2, v2, g, c["lr14"], 0.9, 0.999, bc1, bc2, 1e-15, True)
            b1, b2 = float(F32(0.9)), float(F32(0.999))
            m64 = b1 * m64 + float(F32(1) - F32(0.9)) * g.astype(F64)
            v64 = b2 * v64 + float(F32(1) - F32(0.999)) * g.astype(F64) ** 2
            t64 = t64 - lr * (m64 / bc1) / (np.sqrt(v64 / bc2) + float(F32(1e-15)))
            assert np.allclose(t.v, t64, rtol=1e-13, atol=1e-15) and np.allclose(v.v, v64, rtol=1e-13)
            worst = max(_note("adam", f"P={P} call {k + 1} {nm}", a.v, b) for nm, a, b in (("theta", t2, t), ("m", m2, m), ("v", v2, v)))
            assert worst <= TO.RATIO["adam"], (P, k, worst)
            assert np.array_equal(t.v[::7], c["theta"][::7].astype(F64)) and (t.e[::7] == 0).all()       # g = m = v = 0: theta keeps its bits
        print(f"[gs train cpu] adam P {P}: six calls, restatement error / model bound at most {_WORST['adam'][0]:.3f}")


def _pose_grad64(ps, sums):
    """d/d increment of <R_E, M> + <t_E, s> + <q_E, r> by torch autograd"""
    xi = torch.tensor(ps[7:13].astype(F64), requires_grad=True)
    tau, phi = xi[:3], xi[3:]
    th = phi.norm()
    zero = torch.zeros((), dtype=torch.float64)
    Kx = torch.stack([torch.stack([zero, -phi[2], phi[1]]), torch.stack([phi[2], zero, -phi[0]]), torch.stack([-phi[1], phi[0], zero])])
    R = torch.eye(3, dtype=torch.float64) + torch.sin(th) / th * Kx + (1 - torch.cos(th)) / th ** 2 * Kx @ Kx
    V = torch.eye(3, dtype=torch.float64) + (1 - torch.cos(th)) / th ** 2 * Kx + (th - torch.sin(th)) / th ** 3 * Kx @ Kx
    q = torch.cat([torch.sin(th / 2) / th * phi, torch.cos(th / 2)[None]])
    s = torch.tensor(np.asarray(sums, dtype=F64))
    val = (R.reshape(-1) * s[:9]).sum() + (V @ tau * s[9:12]).sum() + (q * s[12:16]).sum()
    return torch.autograd.grad(val, xi)[0].numpy()


@pytest.mark.parametrize("step", TO.POSE_STEPS)
def test_pose_step_reference_and_restatement(step):
    sums = np.random.default_rng(8).normal(size=16).astype(F32)
    ps32 = TO.pose_state(step)
    ps = ps32.astype(F64)                                                   # (exact: the independent formulas below run in fp64)
    worst = 0.0
    for fold in (0, 1, 2):
        for prior in (0.0, 0.5):
            for rat in (None, 0.3):
                ref = TO.pose_step(ps32, sums, prior, rat, 1e-3, 3e-3, fold)
                f32 = TO.pose_step(ps32, sums, prior, rat, 1e-3, 3e-3, fold, True)
                worst = max(worst, _note("pose_step", f"step {step} fold {fold} prior {prior} ratio {rat}", f32.v, ref))
                assert np.array_equal(ref.v[26:], ps[26:].astype(F64)) and (ref.e[26:] == 0).all()
                if fold:
                    assert (ref.v[7:13] == 0).all() and (ref.e[7:13] == 0).all()
                if fold == 2:
                    assert np.array_equal(ref.v[13:26], ps[13:26].astype(F64))
                else:                                                       # the textbook Adam step on the autograd gradient
                    pc = prior * (2 - float(F32(rat)) if rat is not None else 1.0)
                    g = _pose_grad64(ps, sums) + 2 * float(F32(pc)) * ps[7:13]
                    m = float(F32(0.9)) * ps[13:19] + float(F32(1) - F32(0.9)) * g
                    v = float(F32(0.999)) * ps[19:25] + float(F32(1) - F32(0.999)) * g * g
                    lr = np.array([3e-3] * 3 + [1e-3] * 3, dtype=F32).astype(F64)
                    inc = ps[7:13] - lr / (1 - float(F32(0.9)) ** step) * m / (np.sqrt(v) / np.sqrt(1 - float(F32(0.999)) ** step) + float(F32(1e-8)))
                    assert np.allclose(ref.v[13:19], m, rtol=1e-9) and np.allclose(ref.v[19:25], v, rtol=1e-9) and ref.v[25] == step
                    if not fold:
                        assert np.allclose(ref.v[7:13], inc, rtol=1e-9, atol=1e-12)
                if fold:                                                    # the quaternion is the product, the translation R_E t + t_E
                    new_inc = TO.pose_step(ps, sums, prior, rat, 1e-3, 3e-3, 0).v[7:13] if fold == 1 else ps[7:13].astype(F64)
                    _, t_new, q_new = _pose64(ps, new_inc)
                    assert np.abs(ref.v[3:7] - q_new).max() < 1e-12 and np.abs(ref.v[0:3] - t_new).max() < 1e-12
    print(f"[gs train cpu] pose_step at step {step}: restatement error / model bound {worst:.3f}")
    assert worst <= TO.RATIO["pose_step"]


def test_coefficient_references_and_restatements():
    worst = 0.0
    for sums in TO.COEF_SUMS["map"]:
        for loss0 in (None, 1.5):
            ref, f32 = TO.map_coef(sums, 0.9, 0.5, 0.05, 1.25, 37, 50, loss0), TO.map_coef(sums, 0.9, 0.5, 0.05, 1.25, 37, 50, loss0, True)
            nd = max(sums[3], 1.0)
            assert np.allclose(ref[0].v, [1.25 * 0.9 / (3 * 1850), 1.25 * 0.5 / nd, 1.25 * 0.05 / nd], rtol=1e-7)
            worst = max(worst, _note("coef", "map", f32[0].v, ref[0]))
            if loss0 is not None:
                worst = max(worst, _note("coef", "map loss", f32[1].v, ref[1]))
                assert np.isfinite(ref[1].v).all()
    for sums in TO.COEF_SUMS["refine"]:
        for loss0 in (None, 1.5):
            ref, f32 = TO.refine_coef(sums, 0.9, 0.1, 37, 50, loss0), TO.refine_coef(sums, 0.9, 0.1, 37, 50, loss0, True)
            assert np.isfinite(ref[0].v).all() and np.isfinite(ref[1].v).all()
            worst = max(worst, _note("coef", "refine", f32[0].v, ref[0]), _note("coef", "refine ratio", f32[1].v, ref[1]))
            if loss0 is not None:
                worst = max(worst, _note("coef", "refine loss", f32[2].v, ref[2]))
    print(f"[gs train cpu] coefficient kernels: restatement error / model bound {worst:.3f}")
    assert worst <= TO.RATIO["coef"]


def _normal_autograd(normal, depth, H, W, cam):
    """fp64 autograd of sum (1 - N . depth_to_normal(d)), the border normal zero"""
    fx, fy, cx, cy = (float(F32(v)) for v in cam)
    d = torch.tensor(depth.astype(F64), requires_grad=True)
    N = torch.tensor(normal.astype(F64), requires_grad=True)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    pts = torch.stack([(xs - cx) / fx * d, (ys - cy) / fy * d, d], 0)
    n = torch.zeros(3, H, W, dtype=torch.float64)
    if H > 2 and W > 2:
        dx, dy = pts[:, 1:-1, 2:] - pts[:, 1:-1, :-2], pts[:, 2:, 1:-1] - pts[:, :-2, 1:-1]
        c = torch.cross(dx, dy, dim=0)
        ln = c.norm(dim=0, keepdim=True)
        inner = torch.where(ln > 1e-12, c / torch.where(ln > 1e-12, ln, torch.ones_like(ln)), torch.zeros_like(c))
        n = torch.nn.functional.pad(inner, (1, 1, 1, 1))
    total = (1 - (N * n).sum(0)).sum()
    gN, gd = torch.autograd.grad(total, [N, d], allow_unused=True)
    return float(total), gN.numpy(), (gd.numpy() if gd is not None else np.zeros((H, W)))


@pytest.mark.parametrize("H,W", TO.NORMAL_SIZES)
def test_normal_agreement_reference_is_the_fp64_autograd(H, W):
    normal, depth, g0 = TO.normal_case(H, W)
    coef = 0.37
    total, gN, gd = _normal_autograd(normal, depth, H, W, TO.NORMAL_CAM)
    s, amb = TO.normal_agree_forward(normal, depth, H, W, TO.NORMAL_CAM)
    gn, g_d = TO.normal_agree_backward(normal, depth, H, W, TO.NORMAL_CAM, coef, g0)
    assert not amb.any()
    c = float(F32(coef))
    assert abs(s.v[0] - total) < 1e-11 * H * W and np.abs(gn.v - c * gN).max() < 1e-13 and np.abs(g_d.v - g0 - c * gd).max() < 1e-11
    if min(H, W) < 3:
        assert s.v[0] == H * W and s.e[0] <= 1e-5 and (gn.v == 0).all() and np.array_equal(g_d.v, g0.astype(F64)) and (g_d.e == 0).all()
    s2, _ = TO.normal_agree_forward(normal, depth, H, W, TO.NORMAL_CAM, True)
    gn2, gd2 = TO.normal_agree_backward(normal, depth, H, W, TO.NORMAL_CAM, coef, g0, True)
    r = (_note("normal_sum", f"{H}x{W}", s2.v, s), _note("g_nrm", f"{H}x{W}", gn2.v, gn), _note("g_d", f"{H}x{W}", gd2.v, g_d))
    print(f"[gs train cpu] normal agreement {H} x {W}: sum {s.v[0]:.6f}; restatement error / model bound sum {r[0]:.3f}, g_nrm {r[1]:.3f}, g_d {r[2]:.3f}")
    assert r[0] <= TO.RATIO["normal_sum"] and r[1] <= TO.RATIO["g_nrm"] and r[2] <= TO.RATIO["g_d"]


@pytest.mark.parametrize("P", (1, 257))
def test_densify_reference_and_restatement(P):
    rad, d2, mr, ga, gb, dn = TO.densify_case(P)
    ref, f32 = TO.densify_stats(rad, d2, mr, ga, gb, dn), TO.densify_stats(rad, d2, mr, ga, gb, dn, True)
    vis = rad > 0
    assert np.array_equal(ref[0][~vis], mr[~vis]) and all(np.array_equal(a.v[~vis], b[~vis].astype(F64)) and (a.e[~vis] == 0).all()
                                                          for a, b in zip(ref[1:], (ga, gb, dn)))
    assert np.allclose(ref[1].v[vis], ga[vis] + np.hypot(d2[vis, 0].astype(F64), d2[vis, 1]), rtol=1e-14) and np.array_equal(ref[3].v[vis], dn[vis] + 1.0)
    assert np.array_equal(ref[0], f32[0]) and (ref[3].e == 0).all()
    worst = max(_note("densify", f"P={P}", a.v, b) for a, b in zip(f32[1:], ref[1:]))
    assert worst <= TO.RATIO["densify"]


MUTANTS = ("mod_per_block", "bc2_outside_root", "fold_first", "lr_swapped", "border_normal", "nd_not_floored")


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutant_is_rejected(mutant):
    if mutant in ("mod_per_block", "bc2_outside_root"):
        c = TO.adam_case(300)                                               # 4200 entries: 256 is no multiple of 14
        z = np.zeros(c["n"], dtype=F32)
        bc1, bc2 = TO.adam_bc(3)
        ref = TO.adam(c["theta"], z, z, c["grads"][0], c["lr14"], 0.9, 0.999, bc1, bc2, 1e-15)[0]
        got = TO.adam(c["theta"], z, z, c["grads"][0], c["lr14"], 0.9, 0.999, bc1, bc2, 1e-15, True, (mutant,))[0]
        res = TO.within(got.v, ref, "adam")
    elif mutant in ("fold_first", "lr_swapped"):
        sums = np.random.default_rng(8).normal(size=16).astype(F32)
        ps = TO.pose_state(2)
        ref = TO.pose_step(ps, sums, 0.5, 0.3, 1e-3, 3e-3, 1)
        res = TO.within(TO.pose_step(ps, sums, 0.5, 0.3, 1e-3, 3e-3, 1, True, (mutant,)).v, ref, "pose_step")
    elif mutant == "border_normal":
        normal, depth, g0 = TO.normal_case(37, 50)
        ref = TO.normal_agree_forward(normal, depth, 37, 50, TO.NORMAL_CAM)[0]
        res = TO.within(TO.normal_agree_forward(normal, depth, 37, 50, TO.NORMAL_CAM, True, (mutant,))[0].v, ref, "normal_sum")
    else:
        sums = TO.COEF_SUMS["map"][1]
        ref = TO.map_coef(sums, 0.9, 0.5, 0.05, 1.25, 37, 50, None)[0]
        with np.errstate(all="ignore"):
            res = TO.within(TO.map_coef(sums, 0.9, 0.5, 0.05, 1.25, 37, 50, None, True, (mutant,))[0].v, ref, "coef")
    print(f"[gs train cpu] mutant {mutant}: worst error / bound {res[0]:.3g}, elements beyond {res[1]}")
    assert res[1] > 0


def test_ratio_table_is_the_measured_worst_plus_a_twentieth_rounded_up():
    """runs after the measuring tests of this module (pytest keeps file order)"""
    wrong = []
    for k, ratio in TO.RATIO.items():
        worst, where = _WORST.get(k, (0.0, "not measured"))
        rule = np.ceil((worst + 0.05) * 10 - 1e-9) / 10
        print(f"[gs train cpu] RATIO {k:11s} measured {worst:.3f} ({where}) -> {rule:.1f}, K {max(1.0, 2 * rule):.1f}")
        if abs(ratio - rule) > 1e-9 or where == "not measured":
            wrong.append(k)
    assert not wrong, wrong
