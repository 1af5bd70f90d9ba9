"""GPU: csrc/lpips.hip (fp32-MFMA convolutions, max-pool, tail) through cut3r_slam_amd.lpips.LPIPS against the numpy oracle, bit for bit.
Synthetic weights at the real AlexNet widths."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cut3r_slam_amd import _lib, ops  # noqa: E402
from cut3r_slam_amd import lpips as LP  # noqa: E402
from tests import lpips_ref as LR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_L = {}


def _lpips(norm="torchmetrics", impl=0):
    if (norm, impl) not in _L:
        _L[(norm, impl)] = LP.LPIPS(LR.weights(), DEV, norm, impl)
    return _L[(norm, impl)]


def _gpu(*imgs):
    return [torch.from_numpy(np.ascontiguousarray(i)).to(DEV) for i in imgs]


def _mismatch(got, want):
    got = got.cpu().numpy()
    return f"{int((got != want).sum())} of {want.size} differ, max |diff| {float(np.abs(got.astype(np.float64) - want).max()):.3e}"


@pytest.mark.parametrize("size", LR.SIZES)
@pytest.mark.parametrize("norm", LP.NORMS)
def test_maps_equal_the_oracle_bit_for_bit(size, norm):
    """M below one tile (31x31: 98 rows of conv1, 2 of conv3-5), M no multiple of 32, K = 363 (odd), every border tap, and right and bottom
    columns that the stride drops ((W + 4 - 11) % 4 != 0).  The score: every term is >= 0, so any summation order is within N 2^-52."""
    H, W = size
    a, b = _gpu(*LR.pair(H, W))
    fa, fb, vs, score = LR.oracle(H, W, norm)
    pairs, v = _lpips(norm).maps(a, b)
    for l in range(5):
        assert pairs[l][0].shape == fa[l].shape and v[l].shape == vs[l].shape
        assert np.array_equal(pairs[l][0].cpu().numpy(), fa[l]), f"conv{l + 1} of the first image: {_mismatch(pairs[l][0], fa[l])}"
        assert np.array_equal(pairs[l][1].cpu().numpy(), fb[l]), f"conv{l + 1} of the second image: {_mismatch(pairs[l][1], fb[l])}"
        assert np.array_equal(v[l].cpu().numpy(), vs[l]), f"v{l + 1}: {_mismatch(v[l], vs[l])}"
    got = _lpips(norm)(a, b)
    assert isinstance(got, float) and score > 1e-3
    assert abs(got - score) <= vs[0].size * 2.0 ** -52 * score


@pytest.mark.parametrize("impl", [1, 2, 3])
def test_every_convolution_path_gives_the_same_bits(impl):
    """impl=1 (explicit fmaf on the VALU, one thread per output), 2 and 3 (the MFMA kernel in 128- and 64-row tiles, between which impl=0
    chooses by the number of rows) on three pairs of 67 x 95: conv1 has 2208 rows = 17.25 tiles of 128"""
    prs = [LR.pair(67, 95, seed) for seed in (0, 1, 2)]
    A, B = _gpu(np.stack([p[0] for p in prs]), np.stack([p[1] for p in prs]))
    p0, v0 = _lpips().maps(A, B)
    p1, v1 = _lpips(impl=impl).maps(A, B)
    for l in range(5):
        assert torch.equal(p0[l][0], p1[l][0]) and torch.equal(p0[l][1], p1[l][1]) and torch.equal(v0[l], v1[l]), f"layer {l + 1}"


def test_a_larger_pair_against_fp64():
    """128 x 160 spans many M tiles (conv1: 2 x 31 x 39 = 2418 rows = 19 tiles).  The rule of tests/test_lpips_cpu.py: the relative error
    against the fp64 formulation is at most 4 x that of torch's own fp32 formulation."""
    sd = LR.weights()
    a, b = LR.pair(128, 160)
    for norm in LP.NORMS:
        ref = LR.torch_score(sd, a, b, norm, torch.float64)
        t32 = LR.torch_score(sd, a, b, norm, torch.float32)
        got = _lpips(norm)(*_gpu(a, b))
        e, e32 = abs(got - ref) / ref, abs(t32 - ref) / ref
        print(f"[lpips] 128x160 {norm}: fp64 {ref:.9f}, HIP rel err {e:.2e}, torch fp32 rel err {e32:.2e}")
        assert ref > 1e-3 and e <= 4 * e32


def test_batch_invariance_and_repeatability():
    """three pairs in one call = three single calls, bit for bit (maps and scores); a second run gives the same bits"""
    H, W = 67, 95
    prs = [LR.pair(H, W, seed) for seed in (0, 1, 2)]
    A, B = _gpu(np.stack([p[0] for p in prs]), np.stack([p[1] for p in prs]))
    L = _lpips()
    pairs, vs = L.maps(A, B)
    scores = L(A, B)
    assert scores.shape == (3,) and scores.dtype == torch.float64
    for i in range(3):
        p1, v1 = L.maps(A[i], B[i])
        for l in range(5):
            assert torch.equal(pairs[l][0][i], p1[l][0]) and torch.equal(pairs[l][1][i], p1[l][1]) and torch.equal(vs[l][i], v1[l])
        assert L(A[i], B[i]) == float(scores[i])
    pairs2, vs2 = L.maps(A, B)
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(pairs, pairs2))
    assert all(torch.equal(x, y) for x, y in zip(vs, vs2)) and torch.equal(L(A, B), scores)
    assert len({float(s) for s in scores}) == 3


def test_identical_images_and_an_all_zero_tap():
    a, b = _gpu(*LR.pair(35, 47))
    sd = dict(LR.weights())
    sd["features.10.weight"] = torch.zeros_like(sd["features.10.weight"])
    sd["features.10.bias"] = -torch.ones_like(sd["features.10.bias"])
    for norm in LP.NORMS:
        assert _lpips(norm)(a, a.clone()) == 0.0
        L = LP.LPIPS(sd, DEV, norm)
        pairs, vs = L.maps(a, b)
        assert float(pairs[4][0].abs().max()) == 0.0 and float(pairs[4][1].abs().max()) == 0.0 and float(vs[4].abs().max()) == 0.0
        s = L(a, b)
        assert np.isfinite(s) and s > 0 and all(bool(torch.isfinite(v).all()) for v in vs)


def test_refusals():
    L = _lpips()
    with pytest.raises(ValueError, match="31x31"):
        L(torch.rand(3, 30, 40, device=DEV), torch.rand(3, 30, 40, device=DEV))
    with pytest.raises(ValueError, match="31x31"):
        L(torch.rand(3, 40, 30, device=DEV), torch.rand(3, 40, 30, device=DEV))
    with pytest.raises(ValueError, match="shape"):
        L(torch.rand(3, 40, 40, device=DEV), torch.rand(3, 40, 41, device=DEV))
    sd = dict(LR.weights())
    sd["lin4.model.1.weight"] = torch.zeros(1, 255, 1, 1)
    with pytest.raises(ValueError, match=r"lin4\.model\.1\.weight has shape"):
        LP.LPIPS(sd, DEV)
    lib = _lib.load()
    x = torch.zeros(2, 8, 8, 8, device=DEV)
    w = torch.zeros(3, 3, 8, 64, device=DEV)
    bias = torch.zeros(64, device=DEV)
    y = torch.zeros(2, 8, 8, 64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    ok = (p(x), p(w), p(bias), p(y), 2, 8, 8, 8, 64, 3, 3, 1, 1, 0, None)
    assert lib.cut3r_lpips_conv(*ok) == 0
    for i in range(4):                                                                      # a null pointer in each place
        assert lib.cut3r_lpips_conv(*[None if j == i else v for j, v in enumerate(ok)]) == 1
    assert lib.cut3r_lpips_conv(p(x), p(w), p(bias), p(y), 2, 2, 8, 8, 64, 5, 5, 1, 0, 0, None) == 1       # 2 rows, 5x5 kernel: no output
    assert lib.cut3r_lpips_conv(p(x), p(w), p(bias), p(y), 0, 8, 8, 8, 64, 3, 3, 1, 1, 0, None) == 1
    assert lib.cut3r_lpips_conv(p(x), p(w), p(bias), p(y), 2, 8, 8, 8, 60, 3, 3, 1, 1, 0, None) == 1       # the MFMA tile needs Co % 64 == 0
    assert lib.cut3r_lpips_conv(p(x), p(w), p(bias), p(y), 2, 8, 8, 8, 64, 3, 3, 1, 1, 4, None) == 1       # no such path
    assert lib.cut3r_lpips_conv_out(2, 5, 1, 0) == 0 and lib.cut3r_lpips_conv_out(31, 11, 4, 2) == 7
    assert lib.cut3r_lpips_pool(p(x), p(y), 2, 2, 8, 8, None) == 1 and lib.cut3r_lpips_pool(None, p(y), 2, 8, 8, 8, None) == 1
    assert lib.cut3r_lpips_input(None, p(x), 1, 8, 8, p(y), None) == 1 and lib.cut3r_lpips_input(p(x), p(x), 1, 0, 8, p(y), None) == 1
    sc = torch.zeros(1, dtype=torch.float64, device=DEV)
    assert lib.cut3r_lpips_tail(p(x), p(bias), 1, 64, 8, 0, 0, None, p(sc), None) == 1
    assert lib.cut3r_lpips_tail(p(x), p(bias), 1, 0, 8, 0, 0, p(y), p(sc), None) == 1
    assert lib.cut3r_lpips_tail(p(x), p(bias), 1, 64, 8, 2, 0, p(y), p(sc), None) == 1
    with pytest.raises(ValueError):
        ops.lpips_pool(torch.zeros(2, 2, 8, 8, device=DEV))
    torch.cuda.synchronize()
