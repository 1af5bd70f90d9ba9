"""No GPU: the live TSDF volume's numpy oracle (tests/tsdf_live_oracle.py) commutes and inverts exactly, its resolve is the correctly
rounded mean (against Python fractions), the new entry points are in the ctypes table and the header, and LiveTSDFVolume refuses on
the host what needs no device."""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from cut3r_slam_amd import _lib, ops
from cut3r_slam_amd import tsdf as T
from tests import tsdf_live_oracle as L
from tests import tsdf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scene():
    depth, rgb, w2c, K = O.sphere_scene(n_views=3, H=48, W=64, f=55.0)
    origin, dims, trunc = O.sphere_grid(0.08)
    return depth, rgb, w2c, K, origin, dims, trunc


def test_the_oracle_commutes_and_subtracting_is_the_exact_inverse():
    depth, rgb, w2c, K, origin, dims, trunc = _scene()
    args = (origin, 0.08)
    a = L.integrate(L.new_acc(dims), *args, depth, w2c, K, trunc, 5.0, rgb=rgb)
    assert (a[1] > 0).mean() > 0.05 and (a[0] < 0).any() and a[1].max() == 3 and a[2:].max() > 0
    p = [2, 0, 1]
    b = L.new_acc(dims)
    for i in p:
        L.integrate(b, *args, depth[i:i + 1], w2c[i:i + 1], K, trunc, 5.0, rgb=rgb[i:i + 1])
    assert np.array_equal(a, b)
    # out again, in another order: back to zero on the way through the partial sums
    L.integrate(b, *args, depth[1:2], w2c[1:2], K, trunc, 5.0, rgb=rgb[1:2], sign=-1)
    two = L.integrate(L.new_acc(dims), *args, depth[[0, 2]], w2c[[0, 2]], K, trunc, 5.0, rgb=rgb[[0, 2]])
    assert np.array_equal(b, two)
    L.integrate(b, *args, depth[[2, 0]], w2c[[2, 0]], K, trunc, 5.0, rgb=rgb[[2, 0]], sign=-1)
    assert not b.any()
    # a window of the lattice holds the window of the whole
    w = L.integrate(np.zeros((5, 6, 7, 5), np.int32), *args, depth, w2c, K, trunc, 5.0, rgb=rgb, offset=(3, 2, 4))
    assert np.array_equal(w, a[:, 4:10, 2:9, 3:8])


def _round_f32(fr):
    """the fp32 nearest to a Fraction (ties to even), by integer arithmetic alone"""
    if fr == 0:
        return np.float32(0)
    s, fr = (-1, -fr) if fr < 0 else (1, fr)
    e = fr.numerator.bit_length() - fr.denominator.bit_length() - 24
    while fr / Fraction(2) ** e >= 2 ** 24:
        e += 1
    while fr / Fraction(2) ** e < 2 ** 23:
        e -= 1
    x = fr / Fraction(2) ** e
    n = x.numerator // x.denominator
    r = x - n
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return np.float32(s * math.ldexp(n, e))


def test_resolve_is_the_correctly_rounded_mean():
    """One fp64 division and one rounding to fp32 round p / q correctly whenever the fp64 quotient cannot land on an fp32 midpoint
    that p / q is not: a midpoint M / 2^k (M < 2^25) differs from p / q by at least 1 / (M q) relatively, above the fp64 half-ulp 2^-53 for
    q = count * 32768 <= 2^27, i.e. up to 4096 views -- the counts here."""
    g = np.random.default_rng(0)
    n = 4000
    count = g.integers(1, 4097, n).astype(np.int32)
    count[:8] = (1, 2, 3, 7, 24, 4096, 4095, 1000)
    acc = np.zeros((5, 1, 1, n + 2), np.int32)
    acc[1, 0, 0, :n] = count
    acc[0, 0, 0, :n] = np.rint(g.uniform(-1, 1, n) * count * L.Q)
    acc[0, 0, 0, :4] = (L.Q, -L.Q * 2, 1, -1)
    acc[2:, 0, 0, :n] = g.integers(0, 256 * count[None], (3, n))
    tsdf, weight, color = L.resolve(acc)
    assert tsdf.dtype == weight.dtype == color.dtype == np.float32
    assert np.all(tsdf[0, 0, n:] == 1) and np.all(weight[0, 0, n:] == 0) and np.all(color[:, 0, 0, n:] == 0)
    assert tsdf[0, 0, 0] == 1 and tsdf[0, 0, 1] == -1
    for i in range(n):
        c = int(count[i])
        assert tsdf[0, 0, i] == _round_f32(Fraction(int(acc[0, 0, 0, i]), c * L.Q)), i
        assert weight[0, 0, i] == c
        for p in range(3):
            assert color[p, 0, 0, i] == _round_f32(Fraction(int(acc[2 + p, 0, 0, i]), c)), (i, p)


def test_the_entry_points_are_declared():
    header = open(os.path.join(ROOT, "include", "cut3r_hip.h")).read()
    for name, nargs in (("cut3r_tsdf_live_integrate", 28), ("cut3r_tsdf_live_resolve", 8)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == nargs
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert decl is not None and decl.group(1).count(",") + 1 == nargs
    assert ops.TSDF_LIVE_MAX_VIEWS * ops.TSDF_LIVE_Q < 2 ** 31 <= (ops.TSDF_LIVE_MAX_VIEWS + 1) * ops.TSDF_LIVE_Q
    assert 255 * ops.TSDF_LIVE_MAX_VIEWS < 2 ** 31


def test_host_side_refusals():
    with pytest.raises(ValueError, match="table limit|bricks"):
        T.LiveTSDFVolume.around((0, 0, 0), 60.0, 0.01, device="cpu")                  # 12001^3 voxels: 1501^3 bricks > 2^28
    with pytest.raises(ValueError, match=str(ops.TSDF_SPARSE_MAX_TABLE)):
        T.LiveTSDFVolume.around((0, 0, 0), 60.0, 0.01, device="cpu")
    with pytest.raises(ValueError):
        T.LiveTSDFVolume.around((0, 0, 0), 0.0, 0.01, device="cpu")
    with pytest.raises(ValueError):
        T.LiveTSDFVolume((0, 0, 0), 0.02, (0, 8, 8), device="cpu")
    vol = T.LiveTSDFVolume.around((1.0, -2.0, 0.5), 0.5, 0.02, device="cpu")
    assert isinstance(vol, T._Volume) and vol.dims == (51, 51, 51) and vol.n_bricks == 0 and vol.colored
    assert vol.origin == (0.5, -2.5, 0.0) and vol.acc.shape == (5, 0, 512) and vol.acc.dtype == torch.int32
    assert vol.nbytes == 5 * 7 ** 3
    d, w, K = torch.ones(2, 4, 6), torch.eye(4)[:3].reshape(1, 12).repeat(2, 1), torch.tensor([5.0, 5.0, 2.5, 1.5])
    rgb = torch.zeros(2, 3, 4, 6, dtype=torch.uint8)
    with pytest.raises(ValueError, match="twice"):
        vol.add([3, 3], d, w, K, rgb=rgb)
    with pytest.raises(ValueError, match="rgb"):
        vol.add([0, 1], d, w, K)
    with pytest.raises(ValueError, match="rgb"):
        T.LiveTSDFVolume.around((0, 0, 0), 0.5, 0.02, device="cpu", color=False).add([0, 1], d, w, K, rgb=rgb)
    with pytest.raises(ValueError, match="2 ids, 1 depth"):
        vol.add([0, 1], d[:1], w[:1], K, rgb=rgb[:1])
    rec = T.LiveRecord(d[0], w[0], K, rgb[0], None, 1, 0.0)
    vol.records = {i: rec for i in range(ops.TSDF_LIVE_MAX_VIEWS - 1)}
    with pytest.raises(ValueError, match="already in"):
        vol.add([7], d[:1], w[:1], K, rgb=rgb[:1])
    with pytest.raises(ValueError, match="65535"):
        vol.add([70000, 70001], d, w, K, rgb=rgb)
    with pytest.raises(ValueError, match="not in"):
        vol.remove([70000])
    with pytest.raises(ValueError, match="not in"):
        vol.update([70000], w2c=w[:1])
    with pytest.raises(ValueError, match="the store has"):
        vol.sync(None, 5)
    vol.records = {0: rec, 2: rec}
    with pytest.raises(ValueError, match="keyframes 0"):
        vol.sync(None, 5)
    assert vol.nbytes == 5 * 7 ** 3 + 2 * rec.nbytes
