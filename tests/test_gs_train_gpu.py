"""The trainer-step kernels of csrc/gs_train.hip (cut3r_gs_activate, cut3r_gs_activate_backward, cut3r_gs_adam, cut3r_gs_pose_step,
cut3r_gs_map_coef, cut3r_gs_refine_coef) and cut3r_normal_agree_forward / _backward and cut3r_gs_densify_stats (csrc/gs.hip), each called on
its own through the C ABI and compared PER ELEMENT with the fp64 references of tests/gs_train_oracle.py: every element within K x its own
first-order bound, integer and pass-through outputs exact, accumulating outputs checked on top of a pre-filled value, every output inside
a sentinel-filled allocation whose margins must stay intact, refused calls write nothing.  A kernel that carries state over several calls
(Adam, the accumulating gradients) is fed its OWN previous output, and the reference restarts from that output: every call is judged alone.

Measured on an MI355X, largest error / (K x bound) (each test prints its figures as `[gs train] ...`):
  activate 0.428 (opacity, P = 257); activate_backward gtheta 0.454, pose sums 0.138 (P = 1); adam 0.450 (P = 300); pose_step 0.406 (step 2);
  coefficients 0.403; normal agreement sum 0.004, g_nrm 0.217, g_d 0.229 (37 x 50); densify_stats 0.450 (P = 257).
  powf and the Adam sqrtf are modelled as ONE unit in the last place: the pose step, which has both, reaches 0.406 x K = 0.57 of the model
  bound and Adam 0.450 x K = 0.99 (its worst element is the single rounding of theta - step), so the model holds on this device."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pytestmark = pytest.mark.gpu

from cut3r_slam_amd import _lib  # noqa: E402
from tests import gs_train_oracle as TO  # noqa: E402
from tests.test_gs_render_gpu import DEV, Guarded, _dev, _p  # noqa: E402

F32 = np.float32
_LIVE = []


@pytest.fixture(autouse=True)
def _inputs_stay_allocated():
    """a device tensor made inline for one argument would be freed, and its memory handed to the next one, before the kernel has run"""
    yield
    torch.cuda.synchronize()
    _LIVE.clear()


def _d(a, dtype):
    _LIVE.append(_dev(a, dtype))
    return _LIVE[-1]


def _filled(a, dtype=torch.float32):
    """a Guarded allocation holding `a`"""
    a = np.ascontiguousarray(a)
    g = Guarded(a.shape if a.ndim else (1,), dtype)
    g.t.copy_(torch.from_numpy(a.reshape(g.t.shape)).to(DEV))
    return g


def _untouched(outs):
    return all(g.intact() and bool((g.t == g.fill).all()) for g in outs)


def _check(name, got, ref, group, keep=None):
    r, beyond = TO.within(got, ref, group, keep)
    assert beyond == 0, (name, group, r)
    return r


# ------------------------------------------------------------------------------------------------------------------ activate
@pytest.mark.parametrize("P", TO.SIZES)
def test_activate_every_output_per_element(P):
    lib = _lib.load()
    th, ps = TO.theta_case(P), TO.pose_state()
    out = dict(means=Guarded((P, 3), torch.float32), scales=Guarded((P, 3), torch.float32), rots=Guarded((P, 4), torch.float32),
               opac=Guarded((P,), torch.float32), shs=Guarded((P, 3), torch.float32))
    rc = lib.cut3r_gs_activate(P, _p(_d(th, F32)), _p(_d(ps, F32)), *[_p(out[k].t) for k in ("means", "scales", "rots", "opac", "shs")], None)
    torch.cuda.synchronize()
    assert rc == 0 and all(g.intact() and g.written() for g in out.values())
    ref = TO.activate(th, ps)
    r = {k: _check(f"P={P}", out[k].np(), ref[k], "activate") for k in ("means", "scales", "rots", "opac")}
    assert np.array_equal(out["shs"].np(), ref["shs"])                       # passed through
    print(f"[gs train] activate P {P}: error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))


def _activate_backward(P, th, ps, d, rad, iso, gtheta, sums):
    lib = _lib.load()
    nvis = Guarded((1,), torch.float32)
    rc = lib.cut3r_gs_activate_backward(P, _p(_d(th, F32)), _p(_d(ps, F32)), _p(_d(d["means"], F32)), _p(_d(d["scales"], F32)),
                                        _p(_d(d["rots"], F32)), _p(_d(d["opac"], F32)), _p(_d(d["shs"], F32)), _p(_d(rad, np.int32)), iso,
                                        _p(nvis.t), _p(gtheta.t) if gtheta is not None else None, _p(sums.t) if sums is not None else None, None)
    torch.cuda.synchronize()
    assert rc == 0 and nvis.intact() and all(g.intact() for g in (gtheta, sums) if g is not None)
    return nvis.np()[0]


@pytest.mark.parametrize("P", TO.SIZES)
@pytest.mark.parametrize("iso,kind", ((0.0, "mixed"), (4.0, "mixed"), (4.0, "none")))
def test_activate_backward_accumulates_gtheta_and_pose_sums(P, iso, kind):
    th, ps, d, rad = TO.theta_case(P), TO.pose_state(), TO.grads_case(P), TO.radii_case(P, kind)
    g0, s0 = np.random.default_rng(P).normal(size=(P, 14)).astype(F32), np.random.default_rng(P + 1).normal(size=16).astype(F32)
    gtheta, sums = _filled(g0), _filled(s0)
    worst = [0.0, 0.0]
    for call in range(2):                                                    # two calls add: the second starts from the first's output
        nvis = _activate_backward(P, th, ps, d, rad, iso, gtheta, sums)
        ref = TO.activate_backward(th, ps, d, rad, iso, g0, s0)
        assert ref["ambiguous"].mean() <= 0.02
        if iso != 0.0:
            assert nvis == (rad > 0).sum() == ref["nvis"]                    # the partial counts of the workgroups meet
        g0, s0 = gtheta.np().copy(), sums.np().copy()
        worst[0] = max(worst[0], _check(f"P={P} call {call}", g0, ref["gtheta"], "gtheta", ~ref["ambiguous"][:, None]))
        worst[1] = max(worst[1], _check(f"P={P} call {call}", s0, ref["sums"], "pose_sums"))
    print(f"[gs train] activate_backward P {P} iso {iso} radii {kind}: error / bound gtheta {worst[0]:.3f}, pose sums {worst[1]:.3f}")
    # each output alone: the other is NULL
    only_g, only_s = _filled(g0), _filled(s0)
    _activate_backward(P, th, ps, d, rad, iso, only_g, None)
    _activate_backward(P, th, ps, d, rad, iso, None, only_s)
    ref = TO.activate_backward(th, ps, d, rad, iso, g0, s0)
    _check("gtheta alone", only_g.np(), ref["gtheta"], "gtheta", ~ref["ambiguous"][:, None])
    _check("sums alone", only_s.np(), ref["sums"], "pose_sums")


# ------------------------------------------------------------------------------------------------------------------ Adam
@pytest.mark.parametrize("P", (1, 19, 300))
def test_adam_six_calls_each_within_its_bound(P):
    lib = _lib.load()
    c = TO.adam_case(P)
    n = c["n"]
    theta, m, v = _filled(c["theta"]), _filled(np.zeros(n, dtype=F32)), _filled(np.zeros(n, dtype=F32))
    lr = _d(c["lr14"], F32)
    worst = 0.0
    for k, step in enumerate((1, 2, 3, 4, 5, 1000)):
        g = c["grads"][k % 5]
        bc1, bc2 = TO.adam_bc(step)
        before = (theta.np().copy(), m.np().copy(), v.np().copy())
        rc = lib.cut3r_gs_adam(n, _p(theta.t), _p(m.t), _p(v.t), _p(_d(g, F32)), _p(lr), 0.9, 0.999, bc1, bc2, 1e-15, None)
        torch.cuda.synchronize()
        assert rc == 0 and theta.intact() and m.intact() and v.intact()
        ref = TO.adam(*before, g, c["lr14"], 0.9, 0.999, bc1, bc2, 1e-15)
        worst = max([worst] + [_check(f"P={P} call {k + 1} {nm}", got.np(), r, "adam") for nm, got, r in zip(("theta", "m", "v"), (theta, m, v), ref)])
        assert np.array_equal(theta.np()[::7].view(np.uint32), c["theta"][::7].view(np.uint32))      # g = m = v = 0: theta keeps its bits
    print(f"[gs train] adam P {P}: six calls, error / bound at most {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------ pose step
@pytest.mark.parametrize("step", TO.POSE_STEPS)
def test_pose_step_all_of_the_state(step):
    lib = _lib.load()
    sums = np.random.default_rng(8).normal(size=16).astype(F32)
    ps0 = TO.pose_state(step)
    worst = 0.0
    for fold in (0, 1, 2):
        for prior in (0.0, 0.5):
            for rat in (None, 0.3):
                ps = _filled(ps0)
                ratio = _d(np.array([rat], dtype=F32), F32) if rat is not None else None
                rc = lib.cut3r_gs_pose_step(_p(ps.t), _p(_d(sums, F32)), prior, _p(ratio), 1e-3, 3e-3, fold, None)
                torch.cuda.synchronize()
                assert rc == 0 and ps.intact()
                got = ps.np()
                ref = TO.pose_step(ps0, sums, prior, rat, 1e-3, 3e-3, fold)
                worst = max(worst, _check(f"step {step} fold {fold} prior {prior} ratio {rat}", got, ref, "pose_step"))
                assert np.array_equal(got[26:].view(np.uint32), ps0[26:].view(np.uint32))             # untouched
                assert got[25] == (step if fold != 2 else step - 1)
                if fold:
                    assert (got[7:13] == 0).all()
    print(f"[gs train] pose_step at step {step}: error / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------ coefficients
def test_coefficient_kernels_floors_and_loss_accumulation():
    lib = _lib.load()
    worst = 0.0
    for sums in TO.COEF_SUMS["map"]:
        for loss0 in (None, 1.5):
            coef = Guarded((3,), torch.float32)
            loss = _filled(np.array([loss0], dtype=F32)) if loss0 is not None else None
            rc = lib.cut3r_gs_map_coef(_p(_d(np.array(sums), F32)), 0.9, 0.5, 0.05, 1.25, 37, 50, _p(coef.t), _p(loss.t) if loss else None, None)
            torch.cuda.synchronize()
            assert rc == 0 and coef.intact() and coef.written() and (loss is None or loss.intact())
            ref = TO.map_coef(sums, 0.9, 0.5, 0.05, 1.25, 37, 50, loss0)
            worst = max(worst, _check("map", coef.np(), ref[0], "coef"))
            if loss is not None:
                worst = max(worst, _check("map loss", loss.np(), ref[1], "coef"))
    for sums in TO.COEF_SUMS["refine"]:
        for loss0 in (None, 1.5):
            coef, ratio = Guarded((3,), torch.float32), Guarded((1,), torch.float32)
            loss = _filled(np.array([loss0], dtype=F32)) if loss0 is not None else None
            rc = lib.cut3r_gs_refine_coef(_p(_d(np.array(sums), F32)), 0.9, 0.1, 37, 50, _p(coef.t), _p(ratio.t), _p(loss.t) if loss else None, None)
            torch.cuda.synchronize()
            assert rc == 0 and coef.intact() and coef.written() and ratio.intact() and ratio.written() and (loss is None or loss.intact())
            ref = TO.refine_coef(sums, 0.9, 0.1, 37, 50, loss0)
            worst = max(worst, _check("refine", coef.np(), ref[0], "coef"), _check("refine ratio", ratio.np(), ref[1], "coef"))
            if loss is not None:
                worst = max(worst, _check("refine loss", loss.np(), ref[2], "coef"))
    print(f"[gs train] coefficient kernels: error / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------ normal agreement
@pytest.mark.parametrize("H,W", TO.NORMAL_SIZES)
def test_normal_agreement_sum_and_gradients(H, W):
    lib = _lib.load()
    normal, depth, g0 = TO.normal_case(H, W)
    cam, coef = TO.NORMAL_CAM, 0.37
    n_d, d_d = _d(normal, F32), _d(depth, F32)
    total = Guarded((1,), torch.float32)
    rc = lib.cut3r_normal_agree_forward(_p(n_d), _p(d_d), H, W, *cam, _p(total.t), None)
    g_nrm, g_d = Guarded((3, H, W), torch.float32), _filled(g0)
    rc2 = lib.cut3r_normal_agree_backward(_p(n_d), _p(d_d), H, W, *cam, coef, _p(g_nrm.t), _p(g_d.t), None)
    torch.cuda.synchronize()
    assert rc == 0 and rc2 == 0 and total.intact() and g_nrm.intact() and g_nrm.written() and g_d.intact()
    s, amb = TO.normal_agree_forward(normal, depth, H, W, cam)
    assert not amb.any()
    ref_n, ref_d = TO.normal_agree_backward(normal, depth, H, W, cam, coef, g0)
    r = (_check(f"{H}x{W}", total.np(), s, "normal_sum"), _check(f"{H}x{W}", g_nrm.np(), ref_n, "g_nrm"), _check(f"{H}x{W}", g_d.np(), ref_d, "g_d"))
    if min(H, W) < 3:                                                        # no interior pixel: the sum is H W, every gradient 0
        assert total.np()[0] == H * W and (g_nrm.np() == 0).all() and np.array_equal(g_d.np(), g0)
    print(f"[gs train] normal agreement {H} x {W}: sum {total.np()[0]:.4f}; error / bound sum {r[0]:.3f}, g_nrm {r[1]:.3f}, g_d {r[2]:.3f}")


# ------------------------------------------------------------------------------------------------------------------ densification
@pytest.mark.parametrize("P", (1, 257))
def test_densify_stats_rows_of_invisible_gaussians_keep_their_bits(P):
    lib = _lib.load()
    rad, d2, mr, ga, gb, dn = TO.densify_case(P)
    out = [_filled(a) for a in (mr, ga, gb, dn)]
    rc = lib.cut3r_gs_densify_stats(P, _p(_d(rad, np.int32)), _p(_d(d2, F32)), *[_p(g.t) for g in out], None)
    torch.cuda.synchronize()
    assert rc == 0 and all(g.intact() for g in out)
    ref = TO.densify_stats(rad, d2, mr, ga, gb, dn)
    vis = rad > 0
    for g, before in zip(out, (mr, ga, gb, dn)):
        assert np.array_equal(g.np()[~vis].view(np.uint32), before[~vis].view(np.uint32))
    assert np.array_equal(out[0].np(), ref[0]) and np.array_equal(out[3].np(), ref[3].v.astype(F32))
    r = [_check(f"P={P}", g.np(), e, "densify") for g, e in zip(out[1:], ref[1:])]
    print(f"[gs train] densify_stats P {P}: {int(vis.sum())} visible, error / bound {max(r):.3f}")


# ------------------------------------------------------------------------------------------------------------------ refused calls
def _refused(fn, good, changes, outs):
    for change in changes:
        args = list(good)
        for k, v in change.items():
            args[k] = v
        assert fn(*args) == 1, change
        torch.cuda.synchronize()
        assert _untouched(outs), change


def test_refused_trainer_calls_write_nothing():
    lib = _lib.load()
    P = 65
    th, ps, d, rad = _d(TO.theta_case(P), F32), _d(TO.pose_state(), F32), TO.grads_case(P), _d(TO.radii_case(P, "mixed"), np.int32)
    dd = {k: _d(v, F32) for k, v in d.items()}
    G = lambda *s: Guarded(s, torch.float32)
    out = [G(P, 3), G(P, 3), G(P, 4), G(P), G(P, 3)]
    good = [P, _p(th), _p(ps)] + [_p(g.t) for g in out] + [None]
    _refused(lib.cut3r_gs_activate, good, [{0: 0}, {0: -1}] + [{k: None} for k in range(1, 8)], out)
    gtheta, sums, nvis = G(P, 14), G(16), G(1)
    good = [P, _p(th), _p(ps), _p(dd["means"]), _p(dd["scales"]), _p(dd["rots"]), _p(dd["opac"]), _p(dd["shs"]), _p(rad), 4.0, _p(nvis.t), _p(gtheta.t),
            _p(sums.t), None]
    _refused(lib.cut3r_gs_activate_backward, good, [{0: 0}, {0: -5}, {11: None, 12: None}, {8: None}, {10: None}] + [{k: None} for k in range(1, 8)],
             [gtheta, sums, nvis])
    n = 14 * P
    theta, m, v = G(n), G(n), G(n)
    grad, lr = torch.zeros(n, device=DEV), torch.ones(14, device=DEV)
    good = [n, _p(theta.t), _p(m.t), _p(v.t), _p(grad), _p(lr), 0.9, 0.999, 0.1, 0.001, 1e-15, None]
    _refused(lib.cut3r_gs_adam, good, [{0: 0}, {0: -14}, {0: n - 1}, {0: 15}] + [{k: None} for k in range(1, 6)], [theta, m, v])
    state = G(32)
    good = [_p(state.t), _p(sums.t), 0.0, None, 1e-3, 1e-3, 1, None]
    _refused(lib.cut3r_gs_pose_step, good, [{0: None}, {1: None}], [state])
    coef, ratio, loss = G(3), G(1), G(1)
    s5 = torch.ones(5, device=DEV)
    good = [_p(s5), 0.9, 0.5, 0.05, 1.0, 37, 50, _p(coef.t), _p(loss.t), None]
    _refused(lib.cut3r_gs_map_coef, good, [{0: None}, {7: None}, {5: 0}, {6: -1}], [coef, loss])
    good = [_p(s5), 0.9, 0.1, 37, 50, _p(coef.t), _p(ratio.t), _p(loss.t), None]
    _refused(lib.cut3r_gs_refine_coef, good, [{0: None}, {5: None}, {6: None}, {3: 0}, {4: -1}], [coef, ratio, loss])
