"""The loss kernels of csrc/gs.hip (cut3r_ssim_forward / _backward, cut3r_pixel_loss_forward / _backward, cut3r_refine_loss_forward /
_backward) and the 3-NN (cut3r_knn3_mean_dist2, cut3r_knn3_grid_mean_dist2 with the grid build of csrc/knn_grid.h), each called on its
own through the C ABI and compared PER ELEMENT with the fp64 references of tests/gs_loss_oracle.py: every element within K x its own
first-order bound (only the reference's ambiguous pixels left out), outputs the oracle marks as exact compared for equality, every
output inside a sentinel-filled allocation whose margins must stay intact, the sums started from garbage that the entry points clear
themselves, refused calls write nothing.  The SSIM backward pass is fed the forward kernel's OWN maps, and the reference restarts from
them: each kernel is judged alone.

Measured on an MI355X, largest error / (K x bound) (each test prints its figures as `[gs loss] ...`):
  ssim: map 0.201, d_mu1 0.142, d_x11 0.197 (values up to 4), d_x12 0.382 (two black images: one rounding of 2 C1 / (C1 C2)), grad_a 0.259
  (flat bright); pixel loss: sums 0.198 (3 x 40), g_d 0.423 (fx = fy = 2500, K = 1.6: 0.68 of the model bound); refine loss: sums 0.231
  (16 x 16), g_d 0.718 (41 x 53); 3-NN: exhaustive 0.366 (P = 32769), grid 0.376 (clusters); grid and exhaustive results bit-equal on all
  four shared clouds.
  logf is modelled as ONE unit in the last place: the refine loss's g_d, whose bound is dominated by the two logarithms, reaches 0.72 of
  the model bound on the device where the correctly rounded restatement reaches 0.39 -- the device's logf is not correctly rounded, and
  the one-ulp model holds with room to spare."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pytestmark = pytest.mark.gpu

from cut3r_slam_amd import _lib  # noqa: E402
from tests import gs_loss_oracle as LO  # noqa: E402
from tests.test_gs_render_gpu import DEV, Guarded, _p  # noqa: E402
from tests.test_gs_train_gpu import _d, _filled, _inputs_stay_allocated, _refused  # noqa: E402,F401  (the fixture keeps inputs allocated)

F32 = np.float32
GARBAGE = 1234.5


def _check(name, got, ref, group, keep=None):
    r, beyond = LO.within(got, ref, group, keep)
    assert beyond == 0, (name, group, r)
    return r


def _G(*shape):
    return Guarded(shape, torch.float32)


# ------------------------------------------------------------------------------------------------------------------ SSIM
def _ssim_one(lib, name, Cn, H, W, a, b):
    """forward, then backward on the forward's own maps -> worst error / (K bound) of the five outputs"""
    a_d, b_d = _d(a, F32), _d(b, F32)
    out = [_G(Cn, H, W) for _ in range(4)]
    rc = lib.cut3r_ssim_forward(_p(a_d), _p(b_d), Cn, H, W, *[_p(g.t) for g in out], None)
    torch.cuda.synchronize()
    assert rc == 0 and all(g.intact() and g.written() for g in out), name
    ref = LO.ssim_forward(a, b, Cn, H, W)
    got = [g.np() for g in out]
    r = [_check(name, x, y, grp) for grp, x, y in zip(("ssim_map", "d_mu1", "d_x11", "d_x12"), got, ref)]
    if name.endswith("black"):                                               # every pass runs over zeros
        assert (got[0] == 1).all() and (got[1] == 0).all(), name
    gs = LO.ssim_cotangent(Cn, H, W)
    grad = _G(Cn, H, W)
    rc = lib.cut3r_ssim_backward(_p(a_d), _p(b_d), *[_p(g.t) for g in out[1:]], Cn, H, W, _p(_d(gs, F32)), _p(grad.t), None)
    torch.cuda.synchronize()
    assert rc == 0 and grad.intact() and grad.written() and all(g.intact() for g in out), name
    r.append(_check(name, grad.np(), LO.ssim_backward(a, b, *got[1:], gs, Cn, H, W), "ssim_grad"))
    return r


@pytest.mark.parametrize("content", LO.SSIM_CONTENTS + ("impulse",))
def test_ssim_maps_and_gradient_per_element(content):
    lib = _lib.load()
    worst = np.zeros(5)
    n = 0
    for name, Cn, H, W, a, b in LO.ssim_cases():
        if content in name:
            worst = np.maximum(worst, _ssim_one(lib, name, Cn, H, W, a, b))
            n += 1
    assert n == (len(LO.SSIM_IMPULSES) if content == "impulse" else len(LO.SSIM_SHAPES))
    print(f"[gs loss] ssim {content}, {n} cases: error / (K bound) " + ", ".join(f"{k} {v:.3f}" for k, v in zip(("map", "d_mu1", "d_x11", "d_x12", "grad"), worst)))


# ------------------------------------------------------------------------------------------------------------------ pixel loss
_PIXEL = {name: (H, W, c) for name, H, W, c in LO.pixel_cases()}


@pytest.mark.parametrize("name", tuple(_PIXEL))
def test_pixel_loss_sums_and_gradients_per_element(name):
    lib = _lib.load()
    H, W, c = _PIXEL[name]
    dev = [_p(_d(c[k], F32)) for k in ("img", "gt", "depth", "gt_depth", "gn")]
    cam = [float(v) for v in c["cam"]]
    sums = _filled(np.full(4, GARBAGE, dtype=F32))
    ref = LO.pixel_loss_forward(c["img"], c["gt"], c["depth"], c["gt_depth"], c["gn"], H, W, c["cam"])
    r_s = 0.0
    for call in range(2):                                                    # the entry point clears the sums: garbage, then its own result
        rc = lib.cut3r_pixel_loss_forward(*dev, H, W, *cam, _p(sums.t), None)
        torch.cuda.synchronize()
        assert rc == 0 and sums.intact()
        r_s = max(r_s, _check(f"{name} call {call}", sums.np(), ref, "pix_sums"))
        assert sums.np()[3] == ref.v[3]
    g_img, g_d = _G(3, H, W), _G(H, W)
    rc = lib.cut3r_pixel_loss_backward(*dev, H, W, *cam, _p(_d(np.array(LO.PIXEL_COEF), F32)), _p(g_img.t), _p(g_d.t), None)
    torch.cuda.synchronize()
    assert rc == 0 and g_img.intact() and g_img.written() and g_d.intact() and g_d.written()
    ri, rd, amb = LO.pixel_loss_backward(c["img"], c["gt"], c["depth"], c["gt_depth"], c["gn"], H, W, c["cam"], LO.PIXEL_COEF)
    assert amb.mean() <= LO.MAX_AMBIGUOUS
    assert np.array_equal(g_img.np(), ri)
    r_d = _check(name, g_d.np(), rd, "pix_g_d", ~amb)
    # without the normal term: the gradient is exactly 0 where d == gt_d, and nowhere else on the valid pixels
    coef0 = LO.PIXEL_COEF[:2] + (0.0,)
    g_d0 = _G(H, W)
    rc = lib.cut3r_pixel_loss_backward(*dev, H, W, *cam, _p(_d(np.array(coef0), F32)), _p(g_img.t), _p(g_d0.t), None)
    torch.cuda.synchronize()
    assert rc == 0 and g_d0.intact() and g_d0.written()
    _, rd0, amb0 = LO.pixel_loss_backward(c["img"], c["gt"], c["depth"], c["gt_depth"], c["gn"], H, W, c["cam"], coef0)
    r_d = max(r_d, _check(name + " depth term alone", g_d0.np(), rd0, "pix_g_d", ~amb0))
    mask = LO._valid(c["depth"], c["gt_depth"])
    same = mask & (c["depth"] == c["gt_depth"])
    assert (g_d0.np()[same] == 0).all() and (g_d0.np()[~mask] == 0).all() and (g_d0.np()[mask & ~same & ~amb0] != 0).all()
    print(f"[gs loss] pixel loss {name}: sums {sums.np()}, error / (K bound) sums {r_s:.3f}, g_d {r_d:.3f}, ambiguous {int(amb.sum())} of {H * W}")


# ------------------------------------------------------------------------------------------------------------------ refine loss
@pytest.mark.parametrize("H,W", LO.REFINE_SHAPES)
def test_refine_loss_sums_and_gradients_per_element(H, W):
    lib = _lib.load()
    worst = [0.0, 0.0]
    for content in LO.REFINE_CONTENTS:
        c = LO.refine_case(H, W, content)
        name = f"{H}x{W} {content}"
        dev = [_p(_d(c[k], F32)) for k in ("img", "gt", "depth", "gt_depth", "alpha")]
        args = (c["img"], c["gt"], c["depth"], c["gt_depth"], c["alpha"], LO.REFINE_TH, H, W)
        sums = _filled(np.full(5, GARBAGE, dtype=F32))
        ref = LO.refine_loss_forward(*args)
        for call in range(2):
            rc = lib.cut3r_refine_loss_forward(*dev, LO.REFINE_TH, H, W, _p(sums.t), None)
            torch.cuda.synchronize()
            assert rc == 0 and sums.intact()
            worst[0] = max(worst[0], _check(f"{name} call {call}", sums.np(), ref, "ref_sums"))
            assert sums.np()[1] == ref.v[1] and sums.np()[4] == ref.v[4]
        g_img, g_d = _G(3, H, W), _G(H, W)
        rc = lib.cut3r_refine_loss_backward(*dev, LO.REFINE_TH, H, W, _p(_d(np.array(LO.REFINE_COEF), F32)), _p(g_img.t), _p(g_d.t), None)
        torch.cuda.synchronize()
        assert rc == 0 and g_img.intact() and g_img.written() and g_d.intact() and g_d.written()
        ri, rd = LO.refine_loss_backward(*args, LO.REFINE_COEF)
        assert np.array_equal(g_img.np(), ri)
        worst[1] = max(worst[1], _check(name, g_d.np(), rd, "ref_g_d"))
        if content == "below":                                               # no covered pixel: every sum and gradient exactly 0
            assert (sums.np() == 0).all() and (g_img.np() == 0).all() and (g_d.np() == 0).all()
        if content == "no_depth":
            assert (sums.np()[2:] == 0).all() and sums.np()[1] == H * W and (g_d.np() == 0).all()
    print(f"[gs loss] refine loss {H} x {W}: error / (K bound) sums {worst[0]:.3f}, g_d {worst[1]:.3f}")


# ------------------------------------------------------------------------------------------------------------------ 3-NN
def _knn_exhaustive(lib, p):
    P = len(p)
    chunks = lib.cut3r_knn3_chunks(P)
    assert chunks == LO.knn3_chunks(P)
    out, ws = _G(P), _G(chunks * P * 3)
    rc = lib.cut3r_knn3_mean_dist2(_p(_d(p, F32)), P, _p(out.t), _p(ws.t), None)
    torch.cuda.synchronize()
    assert rc == 0 and out.intact() and out.written() and ws.intact()
    return out.np()


class _Bytes:
    """exactly n bytes inside a sentinel-filled allocation"""
    PAD = 256

    def __init__(self, n):
        self.n = n
        self.whole = torch.full((n + 2 * self.PAD,), 0x5a, dtype=torch.uint8, device=DEV)

    def ptr(self):
        return C.c_void_p(self.whole.data_ptr() + self.PAD)

    def intact(self):
        return bool((self.whole[:self.PAD] == 0x5a).all()) and bool((self.whole[self.PAD + self.n:] == 0x5a).all())


def _knn_grid(lib, p):
    P = len(p)
    n = lib.cut3r_knn3_grid_workspace_bytes(P)
    out, ws = _G(P), _Bytes(n)
    rc = lib.cut3r_knn3_grid_mean_dist2(_p(_d(p, F32)), P, _p(out.t), ws.ptr(), n, None)
    torch.cuda.synchronize()
    assert rc == 0 and out.intact() and out.written() and ws.intact()
    return out.np()


@pytest.mark.parametrize("P", LO.KNN_SIZES)
def test_knn_exhaustive_every_chunk_count(P):
    lib = _lib.load()
    p = LO.knn_surface(P)
    got = _knn_exhaustive(lib, p)
    r = _check(f"P={P}", got, LO.knn3_mean_dist2(p), "knn")
    print(f"[gs loss] knn exhaustive P {P}: {LO.knn3_chunks(P)} chunks of {LO.knn3_chunk_size(P)}, error / (K bound) {r:.3f}")


@pytest.mark.parametrize("name", LO.KNN_GRID)
def test_knn_grid_degenerate_and_outlier_clouds(name):
    """the grid search at every case, whatever the size at which the mapper switches to it"""
    lib = _lib.load()
    p = LO.knn_grid_case(name)
    ref = LO.knn3_mean_dist2(p)
    got = _knn_grid(lib, p)
    r = _check(name, got, ref, "knn")
    note = ""
    if name in LO.KNN_SHARED:
        ex = _knn_exhaustive(lib, p)
        r = max(r, _check(name + " exhaustive", ex, ref, "knn"))
        note = f", grid and exhaustive bit-equal: {np.array_equal(ex.view(np.uint32), got.view(np.uint32))}"
    print(f"[gs loss] knn grid {name}: P {len(p)}, error / (K bound) {r:.3f}{note}")


# ------------------------------------------------------------------------------------------------------------------ refused calls
def test_refused_loss_and_knn_calls_write_nothing():
    lib = _lib.load()
    Cn, H, W = 2, 11, 11
    a, b = (_d(x, F32) for x in LO.ssim_case("random", Cn, H, W))
    maps = [_G(Cn, H, W) for _ in range(4)]
    good = [_p(a), _p(b), Cn, H, W] + [_p(g.t) for g in maps] + [None]
    _refused(lib.cut3r_ssim_forward, good, [{k: None} for k in (0, 1, 5, 6, 7, 8)] + [{2: 0}, {3: 0}, {4: -1}], maps)
    grad, gs = _G(Cn, H, W), torch.ones(1, device=DEV)
    z = torch.zeros(Cn, H, W, device=DEV)
    good = [_p(a), _p(b), _p(z), _p(z), _p(z), Cn, H, W, _p(gs), _p(grad.t), None]
    _refused(lib.cut3r_ssim_backward, good, [{k: None} for k in (0, 1, 2, 3, 4, 8, 9)] + [{5: 0}, {6: -3}, {7: 0}], [grad])

    H, W, c = _PIXEL["17x16 mixed"]
    dev = [_p(_d(c[k], F32)) for k in ("img", "gt", "depth", "gt_depth", "gn")]
    cam = [float(v) for v in c["cam"]]
    sums, g_img, g_d = _G(4), _G(3, H, W), _G(H, W)
    good = dev + [H, W] + cam + [_p(sums.t), None]
    _refused(lib.cut3r_pixel_loss_forward, good, [{k: None} for k in (0, 1, 2, 3, 4, 11)] + [{5: 2}, {6: 2}, {5: 0}, {6: -1}], [sums])
    coef = torch.ones(3, device=DEV)
    good = dev + [H, W] + cam + [_p(coef), _p(g_img.t), _p(g_d.t), None]
    _refused(lib.cut3r_pixel_loss_backward, good, [{k: None} for k in (0, 1, 2, 3, 4, 11, 12, 13)] + [{5: 2}, {6: 2}], [g_img, g_d])

    r = LO.refine_case(H, W, "mixed")
    dev = [_p(_d(r[k], F32)) for k in ("img", "gt", "depth", "gt_depth", "alpha")]
    sums5 = _G(5)
    good = dev + [LO.REFINE_TH, H, W, _p(sums5.t), None]
    _refused(lib.cut3r_refine_loss_forward, good, [{k: None} for k in (0, 1, 2, 3, 4, 8)] + [{6: 0}, {7: -1}], [sums5])
    good = dev + [LO.REFINE_TH, H, W, _p(coef), _p(g_img.t), _p(g_d.t), None]
    _refused(lib.cut3r_refine_loss_backward, good, [{k: None} for k in (0, 1, 2, 3, 4, 8, 9, 10)] + [{6: 0}, {7: 0}], [g_img, g_d])

    P = 300
    pts = _d(LO.knn_surface(P), F32)
    out, ws = _G(P), _G(3 * P)
    good = [_p(pts), P, _p(out.t), _p(ws.t), None]
    _refused(lib.cut3r_knn3_mean_dist2, good, [{0: None}, {2: None}, {3: None}, {1: 3}, {1: 0}, {1: -1}], [out, ws])
    n = lib.cut3r_knn3_grid_workspace_bytes(P)
    wb = _Bytes(n)
    good = [_p(pts), P, _p(out.t), wb.ptr(), n, None]
    _refused(lib.cut3r_knn3_grid_mean_dist2, good, [{0: None}, {2: None}, {3: None}, {1: 3}, {4: n - 1}, {4: 0}], [out])
    assert wb.intact() and bool((wb.whole == 0x5a).all())
