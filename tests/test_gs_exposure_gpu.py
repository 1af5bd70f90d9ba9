"""Exposure compensation (Training.compensate_exposure, hislam2/gs_backend_per_frame.py:467-475, :516, :992) in the tape-free GS trainer.
The three kernels -- cut3r_exposure_forward / _backward, cut3r_gs_exposure_step -- per element against fp64 numpy / torch.optim.Adam in
float64, then gs_step.FusedTrainer with exposure=True against the tensor-op formulation (autograd) on the synthetic wall of
tests/test_gs_mapper_gpu.py, routing, the overflow redo, and GSMapper.eval_rendering_kf.  u = 2^-24 throughout."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
from torch.optim.optimizer import register_optimizer_step_pre_hook

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pytestmark = pytest.mark.gpu

from cut3r_slam_amd import _lib  # noqa: E402
from cut3r_slam_amd import gs_mapper as GM  # noqa: E402
from cut3r_slam_amd.gs_step import ES  # noqa: E402
from tests.test_gs_mapper_gpu import CONFIG, CX, CY, DEV, FX, FY, H, W, _observe, _pair, _pose7, _truth  # noqa: E402

U = 2.0 ** -24
ERR_ARG = 1
# (5,7): less than one wave; (3,171): 513 pixels = one more than two 256-pixel workgroups (the kernels' own coverage); the mapper's test size
SHAPES = [(5, 7), (3, 171), (H, W)]


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _state(A, b):
    es = np.zeros(ES, np.float32)
    es[0:9], es[9:12] = np.asarray(A, np.float32).reshape(-1), np.asarray(b, np.float32)
    return es


def _inputs(h, w, seed=0):
    rng = np.random.default_rng(seed)
    color = rng.uniform(0, 1, (3, h, w)).astype(np.float32)
    A = (np.eye(3) + 0.2 * rng.standard_normal((3, 3))).astype(np.float32)
    b = (0.1 * rng.standard_normal(3)).astype(np.float32)
    return rng, color, A, b


def _forward(lib, color, es):
    out = torch.full_like(color, float("nan"))
    assert lib.cut3r_exposure_forward(_ptr(color), _ptr(es), color.shape[1], color.shape[2], _ptr(out), None) == 0
    torch.cuda.synchronize()
    return out


def _backward(lib, color, g1, g2, es, partials=True, alias=False):
    """-> (g_color, partials [rows,12] or None); one sentinel row behind the partials must stay untouched"""
    h, w = color.shape[1:]
    rows = int(lib.cut3r_exposure_partial_rows(h, w))
    assert rows >= 1
    part = torch.full((rows + 1, 12), float("nan"), device=DEV) if partials else None
    g_color = g1.clone() if alias else torch.full_like(color, float("nan"))
    assert lib.cut3r_exposure_backward(_ptr(color), _ptr(g_color if alias else g1), _ptr(g2), _ptr(es), h, w, _ptr(g_color), _ptr(part), None) == 0
    torch.cuda.synchronize()
    if part is not None:
        assert bool(torch.isnan(part[rows]).all()) and bool(torch.isfinite(part[:rows]).all())
        part = part[:rows].contiguous()
    return g_color, part


def _one_step(lib, es0, part, lr=0.0):
    es = es0.clone()
    assert lib.cut3r_gs_exposure_step(_ptr(es), _ptr(part), part.shape[0], lr, None) == 0
    torch.cuda.synchronize()
    return es


@pytest.mark.parametrize("h,w", SHAPES)
def test_forward_matches_fp64_per_element(h, w):
    """|out - out64| <= 5u (sum_i |c_i A_ij| + |b_j|): the rounding bound of a four-term fp32 sum of products; identity is exact"""
    lib = _lib.load()
    _, color, A, b = _inputs(h, w, seed=1)
    out = _forward(lib, _dev(color), _dev(_state(A, b))).cpu().numpy().astype(np.float64)
    c64, A64, b64 = color.astype(np.float64), A.astype(np.float64), b.astype(np.float64)
    ref = np.einsum("ip,ij->jp", c64.reshape(3, -1), A64) + b64[:, None]
    mag = np.einsum("ip,ij->jp", np.abs(c64.reshape(3, -1)), np.abs(A64)) + np.abs(b64)[:, None]
    ratio = float((np.abs(out.reshape(3, -1) - ref) / (5 * U * mag)).max())
    print(f"[exposure fwd {h}x{w}] worst |err| / bound {ratio:.3f}")
    assert ratio <= 1.0
    cd = _dev(color)
    assert torch.equal(_forward(lib, cd, _dev(_state(np.eye(3), np.zeros(3)))), cd)


def _check_backward(lib, h, w, color, A, b, g1, g2, tag):
    es = _dev(_state(A, b))
    g_color, part = _backward(lib, _dev(color), _dev(g1), _dev(g2) if g2 is not None else None, es)
    g64 = g1.astype(np.float64) + (g2.astype(np.float64) if g2 is not None else 0.0)
    g64, c64, A64 = g64.reshape(3, -1), color.astype(np.float64).reshape(3, -1), A.astype(np.float64)
    ref = np.einsum("ij,jp->ip", A64, g64)
    mag = np.einsum("ij,jp->ip", np.abs(A64), np.abs(g64))
    r_col = float((np.abs(g_color.cpu().numpy().astype(np.float64).reshape(3, -1) - ref) / (4 * U * mag)).max())
    # the 12 gradients as the step kernel forms them: first moment after ONE step from a zero state, m = 0.1 g
    stepped = _one_step(lib, es, part)
    got = stepped[12:24].cpu().numpy().astype(np.float64) / 0.1
    terms = np.concatenate([(c64[:, None, :] * g64[None, :, :]).reshape(9, -1), g64], 0)           # [12, HW], the order of A then b
    ref12, abs12 = terms.sum(1), np.abs(terms).sum(1)
    bound = (h * w + 2) * U * abs12 + U * np.abs(ref12)
    r_sum = float((np.abs(got - ref12) / bound).max())
    print(f"[exposure bwd {h}x{w}, {tag}] worst |err| / bound: g_color {r_col:.3f}, the 12 gradients {r_sum:.2e} "
          f"(a dropped pixel of mean size would be {float((np.abs(terms).mean(1) / bound).min()):.1f} bounds)")
    assert r_col <= 1.0 and r_sum <= 1.0
    assert float(stepped[36]) == 1.0 and bool((stepped[37:40] == 0).all())
    return es, g_color, part, stepped


@pytest.mark.parametrize("h,w", SHAPES)
def test_backward_matches_fp64_per_element_and_per_gradient(h, w):
    """g_color = A (g_out + g_out2) to 4u sum_j |A_ij g_j|; every one of the 12 gradients to the any-order summation bound
    (HW + 2) u sum_p |term_p| + u |g64| -- with strictly positive terms a dropped pixel (HW <= 513) or workgroup (96x128) breaks it"""
    lib = _lib.load()
    rng, color, A, b = _inputs(h, w, seed=2)
    g1, g2 = rng.uniform(0.5, 1, (3, h, w)).astype(np.float32), rng.uniform(0.5, 1, (3, h, w)).astype(np.float32)
    es, g_color, part, stepped = _check_backward(lib, h, w, color, A, b, g1, g2, "two positive gradients")
    # mixed sign, no second gradient
    gm = rng.uniform(-1, 1, (3, h, w)).astype(np.float32)
    _check_backward(lib, h, w, color, A, b, gm, None, "mixed sign, g_out2 = NULL")
    # a frozen exposure: only g_color, the same bits
    g_frozen, none = _backward(lib, _dev(color), _dev(g1), _dev(g2), es, partials=False)
    assert none is None and torch.equal(g_frozen, g_color)
    # g_color written over g_out (the trainer's use)
    g_alias, part_alias = _backward(lib, _dev(color), _dev(g1), _dev(g2), es, alias=True)
    assert torch.equal(g_alias, g_color) and torch.equal(part_alias, part)
    if (h, w) == (H, W):                                # no atomics: the same inputs give the same bits
        _, part2 = _backward(lib, _dev(color), _dev(g1), _dev(g2), es)
        assert torch.equal(part2, part) and torch.equal(_one_step(lib, es, part2), stepped)


def test_step_is_torch_adam():
    """five steps, lr 0.01, constant gradients spanning 3e-8 .. 1e-1 (eps = 1e-8 matters at the small end) against torch.optim.Adam on a
    float64 CPU tensor: max |p - p64| <= n (2u max|p| + 16u lr).  (An fp32 emulation of the kernel's arithmetic uses at most 0.34 of this
    over 200 seeds; eps = 1e-15 exceeds it 10^4-fold.)  The gradients arrive as one partial row, and as three rows that sum to them."""
    lib = _lib.load()
    rng = np.random.default_rng(7)
    n, lr = 5, 0.01
    p0 = np.concatenate([(np.eye(3) + 0.1 * rng.standard_normal((3, 3))).ravel(), 0.1 * rng.standard_normal(3)]).astype(np.float32)
    g = (np.array([1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1e-7, 3e-8, 1e-3, 1e-2, 1e-1]) * np.array([1, -1] * 6)).astype(np.float32)
    t = torch.tensor(p0.astype(np.float64), requires_grad=True)
    opt = torch.optim.Adam([t], lr=lr)
    for _ in range(n):
        t.grad = torch.tensor(g.astype(np.float64))
        opt.step()
    ref = t.detach().numpy()
    bound = n * (2 * U * float(np.abs(p0).max()) + 16 * U * lr)
    for tag, rows in (("one row", g[None]), ("three rows", np.stack([0.25 * g, 0.5 * g, 0.25 * g]))):
        es, part = _dev(_state(p0[:9], p0[9:])), _dev(rows)
        for _ in range(n):
            assert lib.cut3r_gs_exposure_step(_ptr(es), _ptr(part), part.shape[0], lr, None) == 0
        torch.cuda.synchronize()
        got = es.cpu().numpy().astype(np.float64)
        err = float(np.abs(got[:12] - ref).max())
        print(f"[exposure step, {tag}] max |p - p64| {err:.3e} = {err / bound:.3f} of the bound")
        assert err <= bound
        assert got[36] == 5.0 and not got[37:40].any()
        assert float(np.abs(got[:12] - p0).min()) > 0.1 * lr                         # (every parameter moved, the 3e-8 one too)


def test_bad_arguments_are_refused_without_launching():
    lib = _lib.load()
    x, es, part = torch.zeros(3, 4, 5, device=DEV), torch.zeros(ES, device=DEV), torch.zeros(1, 12, device=DEV)
    p, e, q = _ptr(x), _ptr(es), _ptr(part)
    for args in ((None, e, 4, 5, p), (p, None, 4, 5, p), (p, e, 4, 5, None), (p, e, 0, 5, p), (p, e, 4, -1, p), (p, e, 65536, 65536, p)):
        assert lib.cut3r_exposure_forward(*args, None) == ERR_ARG, args
    for args in ((None, p, p, e, 4, 5, p, q), (p, None, p, e, 4, 5, p, q), (p, p, p, None, 4, 5, p, q), (p, p, p, e, 4, 5, None, q),
                 (p, p, p, e, 0, 5, p, q), (p, p, p, e, 4, -1, p, q), (p, p, p, e, 65536, 65536, p, q)):
        assert lib.cut3r_exposure_backward(*args, None) == ERR_ARG, args
    for args in ((None, q, 1, 0.01), (e, None, 1, 0.01), (e, q, 0, 0.01), (e, q, -3, 0.01)):
        assert lib.cut3r_gs_exposure_step(*args, None) == ERR_ARG, args
    # the size query has no status to return: a refused size gives -1 (1 is a valid row count)
    assert lib.cut3r_exposure_partial_rows(0, 5) == -1 and lib.cut3r_exposure_partial_rows(4, -1) == -1
    assert lib.cut3r_exposure_partial_rows(65536, 65536) == -1 and lib.cut3r_exposure_partial_rows(3, 171) == 3
    torch.cuda.synchronize()
    assert not x.any() and not es.any() and not part.any()


# ---------------------------------------------------------------------------------------------------------------- trainer
CFG_X = dict(CONFIG, Training=dict(CONFIG["Training"], compensate_exposure=True), opt_params=dict(CONFIG["opt_params"], exposure_lr=0.01))
_PATTERN = torch.tensor([[1.0, -2.0, 0.5], [0.75, -1.0, 1.5], [-0.5, 2.0, -1.25]])
_OFFSET = torch.tensor([0.02, -0.03, 0.01])
NAMES = {"xyz": (0, 3), "colour": (3, 6), "opacity": (6, 7), "log scale": (7, 10), "quaternion": (10, 14)}


def _pair_x():
    """_pair() with the flag on and the same non-identity exposure on both views of both mappers"""
    a, b = _pair()
    for m in (a, b):
        m.config = CFG_X
        for v in m.viewpoints.values():
            v.exposure_a.data.copy_(torch.eye(3) + 0.05 * _PATTERN)
            v.exposure_b.data.copy_(_OFFSET)
    return a, b


def _exposures(m):
    return torch.stack([torch.cat([m.viewpoints[k].exposure_a.detach().reshape(-1), m.viewpoints[k].exposure_b.detach()]) for k in sorted(m.viewpoints)]).cpu()


class _AutogradExposureGrads:
    """.grad of exposure_a / exposure_b as torch.optim.Adam sees them, by parameter"""

    def __init__(self):
        self.grads = {}

    def __enter__(self):
        def hook(opt, args, kwargs):
            for grp in opt.param_groups:
                for p in grp["params"]:
                    if p.grad is not None:
                        self.grads[id(p)] = p.grad.detach().clone()
        self.handle = register_optimizer_step_pre_hook(hook)
        return self

    def __exit__(self, *exc):
        self.handle.remove()

    def of(self, v):
        if id(v.exposure_a) not in self.grads:
            return None
        return torch.cat([self.grads[id(v.exposure_a)].reshape(-1), self.grads[id(v.exposure_b)]]).cpu()


def _compare_one_iteration(a, b, la, lb, pa0, grads, drawn, names):
    ga, gb = a.gaussians.m / 0.1, b.gaussians.m / 0.1
    for name in names:
        c0, c1 = NAMES[name]
        sc, err = float(ga[:, c0:c1].abs().max()), float((ga[:, c0:c1] - gb[:, c0:c1]).abs().max())
        print(f"[gs fused exposure] d loss / d {name}: scale {sc:.3e}, max |autograd - fused| {err:.3e}")
        assert sc > 0 and err <= 2e-4 * sc + 1e-9, (name, sc, err)
    assert abs(la - lb) <= 1e-5 * abs(la) + 1e-6, (la, lb)
    da, db = a.trajectory().detach() - pa0, b.trajectory().detach() - pa0
    assert float(da.abs().max()) > 1e-5
    torch.testing.assert_close(db, da, atol=1e-5, rtol=0)
    es = b._fused_trainer().exposure_state.cpu()
    for k in drawn:
        g_auto, g_fused = grads.of(a.viewpoints[k]), es[k, 12:24] / 0.1
        sc, err = float(g_auto.abs().max()), float((g_auto - g_fused).abs().max())
        print(f"[gs fused exposure] view {k}: d loss / d exposure: scale {sc:.3e}, max |autograd - fused| {err:.3e}")
        assert sc > 0 and err <= 2e-4 * sc, (k, sc, err)
        assert float(es[k, 36]) == 1.0


def test_one_window_iteration_matches_the_tensor_op_formulation():
    a, b = _pair_x()
    pa0 = a.trajectory().detach().clone()
    with _AutogradExposureGrads() as grads:
        la = a.optimization(1, optimize_pose=True, current_window=[0, 1])
    lb = b.optimization(1, optimize_pose=True, current_window=[0, 1])
    _compare_one_iteration(a, b, la, lb, pa0, grads, (0, 1), NAMES)
    # the stepped parameters went back into the views: the first Adam step moves a parameter by about lr
    moved = (_exposures(b) - torch.cat([(torch.eye(3) + 0.05 * _PATTERN).reshape(-1), _OFFSET])).abs()
    assert 0.5 * 0.01 < float(moved.max()) < 1.5 * 0.01


def test_forty_window_iterations_follow_the_tensor_op_formulation():
    a, b = _pair_x()
    la, lb = a.optimization(40, optimize_pose=True, current_window=[0, 1]), b.optimization(40, optimize_pose=True, current_window=[0, 1])
    d = float((_exposures(a) - _exposures(b)).abs().max())
    print(f"[gs fused exposure] 40 iterations: autograd loss {la:.5f}, fused {lb:.5f}; exposure parameters max |diff| {d:.3e} (allowed {0.05 * 0.01 * 40:.3e})")
    assert abs(la - lb) < 0.02 * la
    torch.testing.assert_close(b.trajectory().detach(), a.trajectory().detach(), atol=2e-4, rtol=0)
    assert d <= 0.05 * 0.01 * 40
    assert bool((b._fused_trainer().exposure_state[:, 36] == 40).all())


def test_one_global_ba_iteration_matches_the_tensor_op_formulation():
    a, b = _pair_x()
    pa0 = a.trajectory().detach().clone()
    x0 = _exposures(b)
    with _AutogradExposureGrads() as grads:
        la = a.global_BA(1, densify=True, densify_every=None, opacity_reset=False, seed=3)
    lb = b.global_BA(1, densify=True, densify_every=None, opacity_reset=False, seed=3)
    drawn = [k for k in (0, 1) if grads.of(a.viewpoints[k]) is not None]
    assert len(drawn) == 1
    other = 1 - drawn[0]
    _compare_one_iteration(a, b, la, lb, pa0, grads, drawn, ("xyz", "colour", "opacity", "log scale"))
    es = b._fused_trainer().exposure_state.cpu()
    assert float(es[other, 36]) == 0.0 and not es[other, 12:36].any() and torch.equal(es[other, :12], x0[other])
    assert torch.equal(_exposures(b)[other], x0[other]) and torch.equal(_exposures(a)[other], x0[other])
    assert not torch.equal(_exposures(b)[drawn[0]], x0[drawn[0]])


def test_a_frozen_pose_freezes_the_exposure():
    a, b = _pair_x()
    x0 = _exposures(a)
    la, lb = a.optimization(5, optimize_pose=False, current_window=[0]), b.optimization(5, optimize_pose=False, current_window=[0])
    assert torch.equal(_exposures(a), x0) and torch.equal(_exposures(b), x0)
    assert abs(la - lb) <= 1e-5 * abs(la) + 1e-6, (la, lb)


def test_the_flag_stays_on_the_tape_free_trainer(monkeypatch):
    _, b = _pair_x()
    assert b.fused

    def no_render(*args, **kw):
        raise AssertionError("GSMapper fell back to the tensor-op formulation")
    monkeypatch.setattr(GM, "render", no_render)
    assert np.isfinite(b.optimization(5, optimize_pose=True, current_window=[0, 1]))
    assert np.isfinite(b.global_BA(5, densify=False, opacity_reset=False))
    assert b._fused_trainer().exposure_state is not None


def test_an_overflowed_capacity_restarts_the_exposures_too():
    ref, b = _pair_x()                                    # the same state twice; both on the tape-free trainer, one with no capacity
    ref.fused = True
    b._fused_trainer().capacity = (0.0, 64)
    lb = b.optimization(12, optimize_pose=True, current_window=[0, 1])
    lr_ = ref.optimization(12, optimize_pose=True, current_window=[0, 1])
    assert b._fused_trainer().redone == 1 and ref._fused_trainer().redone == 0
    steps = b._fused_trainer().exposure_state[:, 36].cpu().tolist()
    assert steps == [12.0, 12.0], steps                   # (23 = the state was not restored before the redo)
    assert abs(lb - lr_) < 0.02 * lr_
    assert float((_exposures(b) - _exposures(ref)).abs().max()) <= 0.05 * 0.01 * 12


def test_eval_rendering_kf_scores_the_compensated_image():
    """the mapper IS the ground-truth map; view 0 holds 0.85 img with exposure 0.85 I (the compensated rendering then equals it), view 1
    the same image with a full affine model.  Flag on: the PSNR of clamp(render @ A + b) (eval_utils.py:127); off: of clamp(render)"""
    truth = _truth()
    pose = _pose7(0, 0, 0, 0, 0)
    img, depth = _observe(truth, pose)
    w2c = torch.inverse(GM.pose_vec_to_matrix(pose[None].to(DEV))[0])
    bg = torch.zeros(3, device=DEV)
    models = [(0.85 * torch.eye(3), torch.zeros(3)), (0.85 * torch.eye(3) + 0.03 * _PATTERN, _OFFSET)]

    def psnr(x, gt):
        mask = gt > 0
        return float(20 * torch.log10(1.0 / torch.sqrt(((x[mask] - gt[mask]) ** 2).mean().clamp_min(1e-12))))
    res = {}
    for flag in (True, False):
        cfg = dict(CONFIG, Training=dict(CONFIG["Training"], compensate_exposure=flag))
        m = GM.GSMapper(cfg, FX, FY, CX, CY, downsample_ratio=2, device=DEV)
        m.gaussians = truth
        want = []
        for k, (A, b) in enumerate(models):
            v = m.viewpoints[k] = GM.Camera(k, 0.85 * img, depth, w2c, FX, FY, CX, CY, device=DEV)
            v.exposure_a.data.copy_(A)
            v.exposure_b.data.copy_(b)
            with torch.no_grad():
                r = GM.render(v, truth, bg)["render"]
                x = (r.permute(1, 2, 0) @ v.exposure_a + v.exposure_b).permute(2, 0, 1) if flag else r
            if flag and k == 0:
                x = 0.85 * r
            want.append(psnr(torch.clamp(x, 0.0, 1.0), v.original_image))
        ev = m.eval_rendering_kf()
        got = [row[1] for row in ev["per_view"]]
        res[flag] = ev["mean_psnr"]
        print(f"[gs exposure] eval_rendering_kf, flag {flag}: {got[0]:.3f} / {got[1]:.3f} dB, expected {want[0]:.3f} / {want[1]:.3f} dB")
        assert len(got) == 2 and abs(got[0] - want[0]) <= 1e-3 and abs(got[1] - want[1]) <= 1e-3
        assert abs(ev["mean_psnr"] - sum(want) / 2) <= 1e-3
    assert res[True] > res[False] + 10.0                   # (the 15 % gain is explained only with the flag on)
