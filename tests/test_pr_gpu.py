"""GPU: the reductions of csrc/prstats.hip against the numpy oracle (tests/pr_oracle.py) -- counts, histogram and the four moments of
dist_stats bit for bit, the median ranks exactly, the eighteen ICP moments bit for bit, refused arguments with untouched outputs."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cut3r_slam_amd import _lib, ops  # noqa: E402
from tests import pr_oracle as PO  # noqa: E402
from tests import recon_oracle as RO  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 70001]


def _g(a, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dt).contiguous()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _check_stats(d2, tau, w, nbins):
    counts, moments, hist = ops.dist_stats(_g(d2), tau, w, nbins)
    counts, moments, hist = counts.cpu().numpy(), moments.cpu().numpy(), hist.cpu().numpy()
    oc, om, oh = PO.dist_stats(d2, tau, w, nbins)
    assert np.array_equal(counts, oc), (counts, oc)
    assert np.array_equal(hist, oh), np.flatnonzero(hist != oh)
    assert np.array_equal(_bits(moments), _bits(om)), (moments, om)
    return counts, moments, hist


def _exact_input(Q, tau, w, nbins, seed):
    """random distances up to 1.3 (some beyond the last edge nbins w = 1.25) with the edge cases written over the first entries"""
    rng = np.random.default_rng(seed)
    d2 = (rng.uniform(0, 1.3, Q).astype(np.float32)) ** 2
    f = np.float32
    pred = lambda x: np.nextafter(f(x), f(0))
    special = [f(tau * tau), pred(tau * tau)]                               # d == tau is not below, its predecessor is
    for k in (1, 2, 100, nbins - 1):
        special += [f((k * w) ** 2), pred((k * w) ** 2)]                   # bin k and bin k - 1
    special += [f((nbins * w) ** 2), f(4.0)]                               # at and beyond the last edge: no bin, still in the sums
    special += [f(0.0), f(-0.0), f(1e-45)]
    special += [f(np.nan), f(-1.0), f(np.inf)]                             # bad: counts[2] only
    special = np.array(special, np.float32)
    n = min(Q, len(special))
    at = rng.permutation(Q)[:n]
    d2[at] = np.roll(special, -Q)[:n]                                      # Q = 1, 2: another part of the list
    return d2, at, special


@pytest.mark.parametrize("Q", SIZES)
def test_dist_stats_exact_edges_bit_for_bit(Q):
    tau, w, nbins = 0.25, 2.0 ** -9, 5 * 128                               # tau^2 and every (k w)^2, k < 4096, are exact in fp32
    d2, at, special = _exact_input(Q, tau, w, nbins, Q)
    counts, moments, hist = _check_stats(d2, tau, w, nbins)
    if Q >= len(special):
        # the edge cases one by one, each alone in a call
        f = np.float32
        one = lambda v: [x.cpu().numpy() for x in ops.dist_stats(_g(np.array([v], np.float32)), tau, w, nbins)]
        assert one(f(tau * tau))[0].tolist() == [1, 0, 0] and one(np.nextafter(f(tau * tau), f(0)))[0].tolist() == [1, 1, 0]
        for k in (1, 2, 100, nbins - 1):
            assert np.flatnonzero(one(f((k * w) ** 2))[2]).tolist() == [k]
            assert np.flatnonzero(one(np.nextafter(f((k * w) ** 2), f(0)))[2]).tolist() == [k - 1]
        for v in (f((nbins * w) ** 2), f(4.0)):
            c, m, h = one(v)
            assert c.tolist() == [1, 0, 0] and h.sum() == 0 and m[0] == np.sqrt(np.float64(v)) and m[1] == np.float64(v)
        for v in (f(0.0), f(-0.0), f(1e-45)):
            c, m, h = one(v)
            assert c.tolist() == [1, 1, 0] and h[0] == 1 and h.sum() == 1
            assert _bits(m[2:]).tolist() == _bits(np.sqrt(np.abs(np.float64(v))) * np.ones(2)).tolist()
        for v in (f(np.nan), f(-1.0), f(np.inf)):
            c, m, h = one(v)
            assert c.tolist() == [0, 0, 1] and h.sum() == 0 and m.tolist() == [0.0, 0.0, np.inf, -np.inf]


@pytest.mark.parametrize("Q", SIZES + [1024 * 1024 + 4099])                # the last: every thread takes a second quad of its own
def test_dist_stats_random_bit_for_bit_and_inside_the_fsum_bound(Q):
    rng = np.random.default_rng(1000 + Q)
    tau, w, nbins = 0.05, 5e-4, 500
    d2 = (rng.gamma(2.0, 0.02, Q).astype(np.float32)) ** 2
    counts, moments, hist = _check_stats(d2, tau, w, nbins)
    assert counts[2] == 0 and counts[0] == Q and hist.sum() <= Q
    fs = PO.fsum_sums(d2)
    # any order of Q non-negative terms stays within (Q - 1) 2^-53 of the exact sum, relative
    assert abs(moments[0] - fs[0]) <= (Q - 1) * 2.0 ** -53 * fs[0]
    assert abs(moments[1] - fs[1]) <= (Q - 1) * 2.0 ** -53 * fs[1]
    # no histogram asked for
    c0, m0, h0 = ops.dist_stats(_g(d2), tau)
    assert np.array_equal(c0.cpu().numpy(), counts) and np.array_equal(_bits(m0.cpu().numpy()), _bits(moments)) and h0.numel() == 0


def test_dist_stats_same_bits_on_every_run_and_for_every_alignment():
    rng = np.random.default_rng(5)
    Q = 70001
    d2 = (rng.uniform(0, 0.3, Q + 3).astype(np.float32)) ** 2
    d2[::11] = np.nan
    big = _g(d2)
    for off in range(4):                                                   # off != 0: the view does not start on a 16-byte boundary
        view = big[off:off + Q]
        a = [x.cpu().numpy() for x in ops.dist_stats(view, 0.05, 5e-4, 500)]
        b = [x.cpu().numpy() for x in ops.dist_stats(view, 0.05, 5e-4, 500)]
        o = PO.dist_stats(d2[off:off + Q], 0.05, 5e-4, 500)
        for x, y, z in zip(a, b, o):
            assert np.array_equal(x, y, equal_nan=True) and np.array_equal(x, z)
        assert np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(_bits(a[1]), _bits(o[1]))
        m = ops.dist_median(view).cpu().numpy()
        assert np.array_equal(_bits(m), _bits(PO.median_ranks(d2[off:off + Q])))


def _median_input(kind, Q, rng):
    f = np.float32
    if kind == "equal":
        return np.full(Q, f(0.3), np.float32)
    if kind == "tied":                                                     # for an even Q the two ranks straddle the two values
        return rng.permutation(np.concatenate([np.full(Q // 2, f(0.25)), np.full(Q - Q // 2, f(0.5))]).astype(np.float32))
    if kind == "low_byte":                                                 # only the last radix pass tells them apart
        return (np.uint32(0x3F000000) | rng.integers(0, 256, Q).astype(np.uint32)).view(np.float32)
    if kind == "top_byte":                                                 # only the first one does
        return ((rng.integers(0, 0x7F, Q).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00123456)).view(np.float32)
    if kind == "bad_interleaved":
        d2 = (rng.uniform(0, 2, Q).astype(np.float32)) ** 2
        d2[1::3] = np.resize(np.float32([np.nan, -1.0, np.inf, -np.inf]), len(d2[1::3]))
        d2[::5] = f(-0.0) if Q > 4 else d2[::5]
        return d2
    if kind == "all_bad":
        return np.resize(np.float32([np.nan, -1.0, np.inf]), Q)
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["equal", "tied", "low_byte", "top_byte", "bad_interleaved", "all_bad"])
@pytest.mark.parametrize("Q", [1, 2, 3, 4, 255, 256, 257, 70001])
def test_dist_median_is_the_sorted_ranks(kind, Q):
    d2 = _median_input(kind, Q, np.random.default_rng(Q))
    got = ops.dist_median(_g(d2)).cpu().numpy()
    ref = PO.median_ranks(d2)                                              # np.sort of the good entries
    if kind == "all_bad":
        assert np.isnan(got).all() and np.isnan(ref).all()
        return
    assert np.array_equal(_bits(got), _bits(ref)), (got, ref)
    if kind == "tied" and Q % 2 == 0:
        assert got.tolist() == [0.25, 0.5]


def _cloud_pair(Q, P, seed):
    rng = np.random.default_rng(seed)
    ref = rng.uniform(-1, 1, (P, 3)).astype(np.float32)
    src = rng.uniform(-1.2, 1.2, (Q, 3)).astype(np.float32)
    M = np.eye(4)
    M[:3, :3] = 1.05 * RO.rot([1, 1, 0.3], 0.2)
    M[:3, 3] = [0.1, -0.2, 0.05]
    return ref, src, M


@pytest.mark.parametrize("Q,P,max_dist", [(1, 7, None), (257, 300, 0.2), (5000, 6000, 0.1), (300001, 20000, 0.08)])
def test_moments_scaled_keeps_the_seventeen_and_adds_the_eighteenth(Q, P, max_dist):
    ref, src, M = _cloud_pair(Q, P, Q)
    grid = ops.NNGrid(_g(ref), Q)
    for T34 in (M, None):
        d2, idx = grid.query(_g(src), max_dist, transform=T34)
        if max_dist is not None:
            share = float((idx < 0).float().mean())
            assert 0.02 < share < 0.98, share                              # some queries without a correspondence, some with
        m17 = grid.moments(_g(src), d2, idx, transform=T34).cpu().numpy()
        m18 = grid.moments_scaled(_g(src), d2, idx, transform=T34).cpu().numpy()
        assert m18.shape == (18,) and np.array_equal(_bits(m18[:17]), _bits(m17))
        o = PO.moments18(src, ref, d2.cpu().numpy(), idx.cpu().numpy(), T34)
        assert np.array_equal(_bits(m18), _bits(o)), (m18 - o)
        assert np.array_equal(_bits(m18), _bits(grid.moments_scaled(_g(src), d2, idx, transform=T34).cpu().numpy()))


def test_refused_arguments_leave_the_outputs_untouched():
    lib = _lib.load()
    p, s = ops._p, ops._stream()
    Q = 100
    d2 = _g(np.linspace(0, 1, Q, dtype=np.float32))
    counts = torch.full((3,), -7, dtype=torch.int64, device=DEV)
    moments = torch.full((4,), -7.0, dtype=torch.float64, device=DEV)
    hist = torch.full((4096,), -7, dtype=torch.int32, device=DEV)
    med = torch.full((2,), -7.0, device=DEV)
    out18 = torch.full((18,), -7.0, dtype=torch.float64, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    nb = ws.numel()
    assert lib.cut3r_dist_stats_workspace_bytes(0) == -1 and lib.cut3r_dist_median_workspace_bytes(-1) == -1
    assert lib.cut3r_icp_moments_scaled_workspace_bytes(0) == -1
    need = lib.cut3r_dist_stats_workspace_bytes(Q)
    assert 0 < need <= nb and 0 < lib.cut3r_dist_median_workspace_bytes(Q) <= nb

    def stats(dist2=d2, Q=Q, tau=0.05, w=5e-4, nbins=500, counts=counts, moments=moments, hist=hist, ws=ws, nbytes=nb):
        return lib.cut3r_dist_stats(p(dist2), Q, tau, w, nbins, p(counts), p(moments), p(hist), p(ws), nbytes, s)

    for bad in (dict(dist2=None), dict(counts=None), dict(moments=None), dict(hist=None), dict(ws=None), dict(Q=0), dict(Q=-1),
                dict(tau=0.0), dict(tau=-1.0), dict(tau=float("nan")), dict(w=0.0), dict(w=-1.0), dict(w=float("nan")), dict(nbins=-1),
                dict(nbins=4097), dict(nbytes=need - 1), dict(ws=ws[4:])):
        assert stats(**bad) == 1, bad
    assert stats(hist=None, nbins=0, ws=torch.empty_like(ws)) == 0         # no histogram: hist may be NULL
    torch.cuda.synchronize()
    assert (hist == -7).all() and int(counts[0]) == Q
    counts.fill_(-7), moments.fill_(-7.0)

    need = lib.cut3r_dist_median_workspace_bytes(Q)
    for args in ((None, Q, p(med), p(ws), nb), (p(d2), Q, None, p(ws), nb), (p(d2), Q, p(med), None, nb), (p(d2), 0, p(med), p(ws), nb),
                 (p(d2), Q, p(med), p(ws), need - 1), (p(d2), Q, p(med), p(ws[4:]), nb)):
        assert lib.cut3r_dist_median(*args, s) == 1

    pts = _g(np.zeros((4, 3), np.float32))
    idx = torch.zeros(4, dtype=torch.int32, device=DEV)
    d4 = torch.zeros(4, device=DEV)
    need = lib.cut3r_icp_moments_scaled_workspace_bytes(4)
    good = [p(pts), 4, p(pts), 4, None, p(d4), p(idx), p(out18), p(ws), nb]
    for i, v in ((0, None), (2, None), (5, None), (6, None), (7, None), (8, None), (1, 0), (3, 0), (9, need - 1), (8, p(ws[4:]))):
        a = list(good)
        a[i] = v
        assert lib.cut3r_icp_moments_scaled(*a, s) == 1, i
    torch.cuda.synchronize()
    assert (counts == -7).all() and (moments == -7).all() and (hist == -7).all() and (med == -7).all() and (out18 == -7).all()
    assert (ws == 0).all()
    # the same refusals through ops
    for call in (lambda: ops.dist_stats(d2, 0.0), lambda: ops.dist_stats(d2, float("nan")), lambda: ops.dist_stats(d2, 0.05, 0.0, 10),
                 lambda: ops.dist_stats(d2, 0.05, 5e-4, 4097), lambda: ops.dist_stats(d2, 0.05, None, 10),
                 lambda: ops.dist_stats(d2.cpu(), 0.05), lambda: ops.dist_stats(d2.double(), 0.05), lambda: ops.dist_stats(d2[:0], 0.05),
                 lambda: ops.dist_median(d2[::2]), lambda: ops.dist_median(d2[:0])):
        with pytest.raises(ValueError):
            call()
