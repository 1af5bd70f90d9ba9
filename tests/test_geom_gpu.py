"""The tracking-geometry kernels of csrc/geometry.hip through cut3r_slam_amd.ops, on the paths production runs and the existing
bit-exact tests (tests/test_kernels_gpu.py) do not reach: the device-side keyframe chain, patch overlap per element, camera chunks
beyond 64, the grid-stride loops, and cut3r_window_update in every way track_frontend calls it.

References and tolerances: tests/geom_oracle.py (derived there, none measured).  Cases: tests/geom_cases.py; each test asserts the
conditions of its case again before it launches (tests/test_geom_cases_cpu.py proves them without a GPU).  Everything integer,
every stored pointmap, confidence and depth is compared bit for bit with oracle/oracle_geom.c.  Each test prints its figures as
`[geom] ...`.

Measured on an MI355X: the 70 tests of this file take 4.3 s together (the slowest 0.4 s).  Largest error / bound: normalised rows 0.41
(C = 8), 0.09 (C = 64), 0.005 (C = 1024); row maxima 1.1e-6 of 1.2e-4 at C = 1024, 3e-7 of 8e-6 at C = 64; the marked log-depth sum is
-4 logf(2) to the last bit; the random one lies 1.8e-8 per term from the libm sum."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pytestmark = pytest.mark.gpu

from cut3r_slam_amd import _lib, ops  # noqa: E402
from oracle import geom as G  # noqa: E402
from tests import geom_cases as GC  # noqa: E402
from tests import geom_oracle as GO  # noqa: E402

DEV = "cuda:0"
REFUSED = (ValueError, _lib.Cut3rHipError)
GUARD = 64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def nan_ws(n):
    """a workspace of n floats followed by GUARD more, all NaN: what is still NaN afterwards was not written"""
    return torch.full((n + GUARD,), float("nan"), device=DEV)


def ints(n, fill=-1):
    return torch.full((n,), fill, dtype=torch.int32, device=DEV)


def check_rows(got, feat, Cc, what):
    """normalised rows per element: (C/2 + 3) u relative + 2^-126"""
    ref = GO.normalised_rows64(feat)
    err = np.abs(got.double().cpu().numpy() - ref)
    bound = GO.row_bound(Cc) * np.abs(ref) + GO.TINY
    worst = float((err / bound).max())
    print(f"[geom] {what}: worst row error / bound {worst:.3f}")
    assert (err <= bound).all(), f"{what}: {int((err > bound).sum())} elements beyond (C/2+3)u, worst {worst:.3f} x bound"
    return ref


# ------------------------------------------------------------------------------------------------ patch overlap, per element
@pytest.mark.parametrize("N,Cc", GC.OVERLAP_SHAPES)
@pytest.mark.parametrize("variant", GC.OVERLAP_VARIANTS)
def test_patch_overlap_rows_maxima_and_count(N, Cc, variant):
    case = GC.overlap_case(N, Cc, variant)
    Nv, thr = N - 1, case["thr"]
    mx = GO.row_maxima64(case["feat0"], case["feat1"])
    assert np.abs(mx - thr).min() > GO.max_bound(Cc)                        # the condition that makes the count exact
    ws, cnt = nan_ws(2 * Nv * Cc + Nv), ints(1 + GUARD)
    ops.patch_overlap_count(dev(case["feat0"]), dev(case["feat1"]), thr, ws, cnt[:1])
    torch.cuda.synchronize()
    # the documented workspace layout (include/cut3r_hip.h): n0 [Nv,C], n1 [Nv,C], row maxima [Nv]
    n0, n1, rmax = ws[:Nv * Cc].view(Nv, Cc), ws[Nv * Cc:2 * Nv * Cc].view(Nv, Cc), ws[2 * Nv * Cc:2 * Nv * Cc + Nv]
    assert bool(torch.isnan(ws[2 * Nv * Cc + Nv:]).all()) and bool((cnt[1:] == -1).all())
    check_rows(n0, case["feat0"], Cc, f"n0 {N}x{Cc} {variant}")
    check_rows(n1, case["feat1"], Cc, f"n1 {N}x{Cc} {variant}")
    got = rmax.double().cpu().numpy()
    err = np.abs(got - np.maximum(mx, 0.0))
    print(f"[geom] row maxima {N}x{Cc} {variant}: worst error {err.max():.3e}, bound {GO.max_bound(Cc):.3e}")
    assert (err <= GO.max_bound(Cc)).all()
    assert int(cnt[0]) == int((mx > thr).sum())
    p = case["planted"]
    if "zero0" in p:
        assert bool((n0[p["zero0"]] == 0).all()) and got[p["zero0"]] == 0.0
    if "zero1" in p:
        assert bool((n1[p["zero1"]] == 0).all())
    if "negative" in p:
        assert mx[p["negative"]] < -0.1 and got[p["negative"]] == 0.0       # clamped: exactly 0
    for r in p.get("duplicate", ()):
        assert abs(got[r] - 1.0) <= GO.max_bound(Cc)


# ------------------------------------------------------------------------------------------------ keyframe chain
def run_chain(case, thr_ratio, forced, ws=None):
    B, Nv, Cc = len(case["feats"]), case["Nv"], case["C"]
    need = (B + 1) * Nv * Cc + Nv
    if ws is None:
        ws = nan_ws(need)
    out = ints(2 * B + 1 + GUARD, -7)                                        # counts, decisions, state: one allocation, as motion_filter
    ops.patch_overlap_chain(dev(case["feat_last"]), dev(case["feats"]), case["thr_sim"], thr_ratio, forced, ws, out[2 * B:2 * B + 1], out[:B],
                            out[B:2 * B])
    torch.cuda.synchronize()
    assert bool((out[2 * B + 1:] == -7).all()) and bool(torch.isnan(ws[need:]).all())
    assert bool((ws[need - Nv:need].view(torch.int32) == 0).all()), "the row maxima are left cleared"
    h = out.cpu().numpy()
    return h[:B], h[B:2 * B], int(h[2 * B]), ws


@pytest.mark.parametrize("name,Nv,Cc", GC.CHAIN_CASES)
def test_keyframe_chain_counts_decisions_and_state(name, Nv, Cc):
    case = GC.chain_case(name, Nv, Cc)
    scan = GO.chain_scan(case["feat_last"], case["feats"], case["thr_sim"], case["thr_ratio"], case["forced"])
    assert GO.min_distance(scan) > GO.max_bound(Cc)                          # no row of any step near thr_sim: counts are exact
    assert scan["decisions"].tolist() == case["decisions"] and 0 < scan["decisions"].sum() < len(case["feats"])
    counts, decisions, state, ws = run_chain(case, case["thr_ratio"], case["forced"])
    print(f"[geom] chain {name} Nv={Nv} C={Cc}: counts {counts.tolist()} decisions {decisions.tolist()} state {state}"
          f" (reference {scan['counts'].tolist()} {scan['decisions'].tolist()} {scan['state']})")
    np.testing.assert_array_equal(counts, scan["counts"])
    np.testing.assert_array_equal(decisions, scan["decisions"])
    assert state == scan["state"]
    B = len(case["feats"])
    sets = ws[:(B + 1) * Nv * Cc].view(B + 1, Nv, Cc)
    check_rows(sets[0], case["feat_last"], Cc, f"chain set 0 {name}")
    check_rows(sets[B], case["feats"][B - 1], Cc, f"chain set {B} {name}")
    # the same call on the same workspace: the same result (the row maxima were left cleared, the state starts at -1 again)
    counts2, decisions2, state2, _ = run_chain(case, case["thr_ratio"], case["forced"], ws)
    np.testing.assert_array_equal(counts2, counts)
    np.testing.assert_array_equal(decisions2, decisions)
    assert state2 == state
    # and a plain pair count on that workspace afterwards gives its own count
    mx = GO.row_maxima64(case["feat_last"], case["feats"][1])
    assert np.abs(mx - case["thr_sim"]).min() > GO.max_bound(Cc)
    cnt = ints(1)
    ops.patch_overlap_count(dev(case["feat_last"]), dev(case["feats"][1]), case["thr_sim"], ws, cnt)
    assert int(cnt[0]) == int((mx > case["thr_sim"]).sum())


@pytest.mark.parametrize("Nv,Cc", [(31, 8), (70, 64)])
def test_keyframe_chain_that_never_takes_equals_separate_pair_counts(Nv, Cc):
    """thr_ratio = -1, forced = None (track_backend._feat_overlap): B counts against feat_last, the state stays -1"""
    case = GC.chain_case("mixed", Nv, Cc)
    scan = GO.chain_scan(case["feat_last"], case["feats"], case["thr_sim"], -1.0, None)
    assert GO.min_distance(scan) > GO.max_bound(Cc)
    counts, decisions, state, _ = run_chain(case, -1.0, None)
    B = len(case["feats"])
    ws, cnt = nan_ws(2 * Nv * Cc + Nv), ints(B)
    f0 = dev(case["feat_last"])
    for i in range(B):
        ops.patch_overlap_count(f0, dev(case["feats"][i]), case["thr_sim"], ws, cnt[i:i + 1])
    np.testing.assert_array_equal(counts, cnt.cpu().numpy())
    np.testing.assert_array_equal(counts, scan["counts"])
    assert not decisions.any() and state == -1 and len(set(counts.tolist())) > 1


def test_negative_similarity_threshold_is_refused_with_nothing_launched():
    """the clamp at 0 and the unsigned maximum on float bits would count every row for thr < 0"""
    case = GC.chain_case("mixed", 31, 8)
    B, Nv, Cc = len(case["feats"]), 31, 8
    f0, fs = dev(case["feat_last"]), dev(case["feats"])
    lib = _lib.load()
    for thr in (-0.25, float("nan")):
        ws, out, cnt = nan_ws((B + 1) * Nv * Cc + Nv), ints(2 * B + 1, -7), ints(1, -7)
        with pytest.raises(REFUSED):
            ops.patch_overlap_count(f0, fs[0], thr, ws, cnt)
        with pytest.raises(REFUSED):
            ops.patch_overlap_chain(f0, fs, thr, 0.5, None, ws, out[2 * B:], out[:B], out[B:2 * B])
        # the C entry points themselves, below the wrappers' own check
        assert lib.cut3r_patch_overlap(ops._p(f0), ops._p(fs[0]), Nv + 1, Cc, thr, ops._p(ws), ops._p(cnt), ops._stream()) == 1
        assert lib.cut3r_patch_overlap_chain(ops._p(f0), ops._p(fs), B, Nv + 1, Cc, thr, 0.5, None, ops._p(ws), ops._p(out[2 * B:]), ops._p(out),
                                             ops._p(out[B:]), ops._stream()) == 1
        torch.cuda.synchronize()
        assert bool(torch.isnan(ws).all()) and bool((out == -7).all()) and int(cnt[0]) == -7


def test_patch_overlap_argument_refusals():
    """C not a multiple of 8 (the k loop takes 8 channels a step) and a feature pointer off the 16-byte grid: refused, nothing launched"""
    N = 33
    for Cc, shift in ((12, 0), (16, 1)):
        base = torch.randn(3 * N * Cc + 8, device=DEV)
        f0 = base[shift:shift + N * Cc].view(N, Cc)
        fs = base[N * Cc + shift:3 * N * Cc + shift].view(2, N, Cc)
        assert f0.is_contiguous() and fs.is_contiguous() and (f0.data_ptr() % 16 != 0) == bool(shift)
        ws, out, cnt = nan_ws(3 * (N - 1) * Cc + N), ints(5, -7), ints(1, -7)
        with pytest.raises(REFUSED):
            ops.patch_overlap_count(f0, fs[0], 0.7, ws, cnt)
        with pytest.raises(REFUSED):
            ops.patch_overlap_chain(f0, fs, 0.7, 0.5, None, ws, out[4:], out[:2], out[2:4])
        torch.cuda.synchronize()
        assert bool(torch.isnan(ws).all()) and bool((out == -7).all()) and int(cnt[0]) == -7


# ------------------------------------------------------------------------------------------------ forward overlap, camera chunks
@pytest.mark.parametrize("B,N,has_align,clamp_z", GC.FWD_CASES)
def test_overlap_fwd_beyond_one_camera_chunk(B, N, has_align, clamp_z):
    case = GC.fwd_case(B, N, has_align)
    ref = GC.fwd_reference(case, clamp_z)
    assert GC.chunks_not_vacuous(ref, N)
    cnt = ints(B + GUARD)
    ops.overlap_fwd(dev(case["pm"]), dev(case["w2c"]), case["K4"], case["W"], case["H"], cnt, P12=case["P12"], s_align=case["s"], clamp_z=clamp_z)
    torch.cuda.synchronize()
    got = cnt.cpu().numpy()
    print(f"[geom] overlap_fwd B={B} N={N} align={has_align} clamp={clamp_z}: {int((got[:B] > 0).sum())} cameras see something, sum {int(got[:B].sum())}")
    np.testing.assert_array_equal(got[:B], ref)
    assert (got[B:] == -1).all()


# ------------------------------------------------------------------------------------------------ backward overlap
@pytest.mark.parametrize("name", ["stride", "slots", "one"])
def test_overlap_bwd_grid_stride_and_slots(name):
    case = GC.bwd_case(name)
    B, N = case["B"], case["N"]
    slots = [GO.slot_of(b, case["grp"], case["grp_stride"]) for b in range(B)]
    ref = G.overlap_bwd(case["store"][slots], case["w2c"], case["K4"], case["W"], case["H"])
    assert ((ref > 0) & (ref < N)).all()
    if name == "stride":
        tail = G.overlap_bwd(case["store"][:, 65536:], case["w2c"], case["K4"], case["W"], case["H"])
        assert N > 65536 and (tail > 0).all()                                # the points only the second pass reaches count
    if name == "slots":
        assert G.overlap_bwd(case["store"][5:6], case["w2c"], case["K4"], case["W"], case["H"])[0] == N      # the unused slot would show
    cnt = ints(B + GUARD)
    ops.overlap_bwd(dev(case["store"]), dev(case["w2c"]), case["K4"], case["W"], case["H"], cnt, B=B, N=N, grp=case["grp"], grp_stride=case["grp_stride"])
    torch.cuda.synchronize()
    got = cnt.cpu().numpy()
    print(f"[geom] overlap_bwd {name}: {got[:B].tolist()} of {N}")
    np.testing.assert_array_equal(got[:B], ref)
    assert (got[B:] == -1).all()


def test_overlap_bwd_refuses_a_group_stride_below_the_group():
    case = GC.bwd_case("slots")
    cnt = ints(8)
    with pytest.raises(REFUSED):
        ops.overlap_bwd(dev(case["store"]), dev(case["w2c"]), case["K4"], case["W"], case["H"], cnt, B=5, N=case["N"], grp=5, grp_stride=4)
    torch.cuda.synchronize()
    assert bool((cnt == -1).all())


# ------------------------------------------------------------------------------------------------ window update
CONF_FILL, DEPTH_FILL, W2C_FILL, LSUM_FILL = -7.0, -9.0, 7.0, 3.0


def window_reference(case):
    v = GC.window_views(case)
    new = v["w2c"][v["t0"]:v["t0"] + case["V"]] if case["has_w2c"] else None
    return GO.window_reference(case["pts"], case["conf"], case["P"], case["s"], case["ds"], v["store"], v["dst_slot"], v["w2c"], v["t0"], case["first"],
                               case["K4"], case["ldc"], w2c_new=new)


def launch_window(case, lsum=None):
    """the call of track_frontend: pm_ds / conf_ds = store[sub, a:a+V], depth rows, the store and w2c from the base on, t0 relative"""
    t0, V, b0, ds = case["t0"], case["V"], case["b0"], case["ds"]
    h, w = case["H"] // ds, case["W"] // ds
    store = dev(case["store"])
    conf_store = torch.full(tuple(store.shape[:4]), CONF_FILL, device=DEV)
    depth = torch.full((V, case["H"], case["W"]), DEPTH_FILL, device=DEV)
    w2c = dev(case["w2c"])
    if case["has_w2c"]:
        w2c[t0:] = W2C_FILL                       # the rows of the window's keyframes arrive through the kernel arguments
    counts = torch.full((V, 2, case["ldc"]), -1, dtype=torch.int32, device=DEV)
    sub, a = divmod(t0, 5)
    ops.window_update(dev(case["pts"]), dev(case["conf"]), case["P"].reshape(-1).tolist(), case["s"], ds, store[sub, a:a + V], conf_store[sub, a:a + V], depth,
                      store[b0 // 5:], w2c[b0:], t0 - b0, case["first"], case["K4"], counts,
                      w2c_new=case["w2c"][t0:t0 + V].reshape(-1).tolist() if case["has_w2c"] else None, lsum_reset=lsum)
    torch.cuda.synchronize()
    return store, conf_store, depth, w2c, counts


@pytest.mark.parametrize("name", sorted(GC.WINDOW_CASES))
def test_window_update_against_the_oracle(name):
    case = GC.window_case(name)
    ref = window_reference(case)
    t0, V, b0 = case["t0"], case["V"], case["b0"]
    if case["first"] > t0 + V:
        assert not ref["counts"].any()
    else:
        assert GC.counted_rows_not_vacuous(case, ref["counts"])
    lsum = torch.full((1,), LSUM_FILL, dtype=torch.float64, device=DEV)
    store, conf_store, depth, w2c, counts = launch_window(case, lsum if case["has_lsum"] else None)
    got = counts.cpu().numpy()
    print(f"[geom] window {name}: forward sums {got[:, 0].sum(1).tolist()} backward sums {got[:, 1].sum(1).tolist()}")
    # whole rows, all 2 * ldc entries of each: the counts, zeros beyond kfi, zero rows below `first`
    np.testing.assert_array_equal(got, ref["counts"])
    # stores: the window's slots hold G.align_view's bits, everything else (the slots before the base included) is as it was
    exp_store = case["store"].copy()
    exp_store[b0 // 5:] = ref["store"].reshape((-1,) + case["store"].shape[1:])
    np.testing.assert_array_equal(store.cpu().numpy(), exp_store)
    sub, a = divmod(t0, 5)
    exp_conf = np.full(conf_store.shape, CONF_FILL, np.float32)
    exp_conf[sub, a:a + V] = ref["conf_ds"]
    np.testing.assert_array_equal(conf_store.cpu().numpy(), exp_conf)
    np.testing.assert_array_equal(depth.cpu().numpy(), ref["depth"])
    for v in range(V):                             # and directly, view by view
        pm, cd, dp = G.align_view(case["pts"][v], case["conf"][v], case["P"][v], case["s"], case["ds"])
        assert np.array_equal(store[sub, a + v].cpu().numpy(), pm) and np.array_equal(conf_store[sub, a + v].cpu().numpy(), cd)
        assert np.array_equal(depth[v].cpu().numpy(), dp)
    # w2c: given -> rows t0.. written from the arguments; not given -> untouched.  Either way the table is the case's own
    np.testing.assert_array_equal(w2c.cpu().numpy(), case["w2c"])
    assert float(lsum) == (0.0 if case["has_lsum"] else LSUM_FILL)


def _raw_window(case, V=None, ldc=None):
    """cut3r_window_update itself with an argument the Python wrapper would stop first; returns the code and the outputs"""
    V = case["V"] if V is None else V
    H, W, ds, t0 = case["H"], case["W"], case["ds"], case["t0"]
    h, w = H // ds, W // ds
    pts, conf = torch.ones(7, H, W, 3, device=DEV), torch.ones(7, H, W, device=DEV)
    outs = [torch.full((7, h, w, 3), DEPTH_FILL, device=DEV), torch.full((7, h, w), DEPTH_FILL, device=DEV), torch.full((7, H, W), DEPTH_FILL, device=DEV),
            torch.full((7, 2, 96), -1, dtype=torch.int32, device=DEV), torch.full((1,), LSUM_FILL, dtype=torch.float64, device=DEV)]
    store, w2c = dev(case["store"]), torch.full((32, 12), W2C_FILL, device=DEV)
    arr = (C.c_float * 84)(*([0.0] * 84))
    rc = _lib.load().cut3r_window_update(ops._p(pts), ops._p(conf), V, H, W, arr, 1.0, ds, ops._p(outs[0]), ops._p(outs[1]), ops._p(outs[2]), ops._p(store), 5, 6,
                                         ops._p(w2c), arr, t0, 3, *case["K4"], ops._p(outs[3]), 96 if ldc is None else ldc, ops._p(outs[4]), ops._stream())
    torch.cuda.synchronize()
    return rc, outs + [w2c]


def _untouched(outs):
    fills = (DEPTH_FILL, DEPTH_FILL, DEPTH_FILL, -1, LSUM_FILL, W2C_FILL)
    return all(bool((o == f).all()) for o, f in zip(outs, fills))


def test_window_update_argument_refusals():
    case = GC.window_case("no_lsum_reset")                                   # t0 = 10, V = 6
    rc, outs = _raw_window(case, V=7)
    assert rc == 1 and _untouched(outs)
    rc, outs = _raw_window(case, ldc=15)                                     # ldc < t0 + V = 16
    assert rc == 1 and _untouched(outs)
    t0 = case["t0"]

    def call(H=case["H"], W=case["W"], ds=2, V=6, ldc=80, **kw):
        h, w = H // ds, W // ds
        store = torch.zeros(4, 6, h, w, 3, device=DEV)
        outs = [torch.full((V, h, w, 3), DEPTH_FILL, device=DEV), torch.full((V, h, w), DEPTH_FILL, device=DEV), torch.full((V, H, W), DEPTH_FILL, device=DEV),
                torch.full((V, 2, ldc), -1, dtype=torch.int32, device=DEV), torch.full((1,), LSUM_FILL, dtype=torch.float64, device=DEV),
                torch.full((t0 + V, 12), W2C_FILL, device=DEV)]
        with pytest.raises(REFUSED):
            ops.window_update(torch.ones(V, H, W, 3, device=DEV), torch.ones(V, H, W, device=DEV), [0.0] * (12 * V), 1.0, ds, outs[0], outs[1], outs[2], store,
                              outs[5], t0, 3, case["K4"], outs[3], w2c_new=[0.0] * (12 * V), lsum_reset=outs[4], **kw)
        torch.cuda.synchronize()
        assert _untouched(outs)

    call(V=7)
    call(ldc=15)
    call(H=26, W=36, ds=4)                                                   # stored maps of 6 x 9 x 12 bytes = 648: not a multiple of 16
    call(grp=5, grp_stride=4)


def test_window_update_refuses_more_than_65535_pointmaps_before_its_first_launch():
    """win_bwd_kernel's grid.y is the newest keyframe's index: beyond 65535 the call returns the argument error, and it does so before the
    align kernel has zeroed the counts, written w2c rows or reset the accumulator"""
    H = W = 4
    V, t0, ds = 6, 65531, 2
    nsub = (t0 + V) // 5 + 2
    store = torch.zeros(nsub, 6, 2, 2, 3, device=DEV)
    outs = [torch.full((V, 2, 2, 3), DEPTH_FILL, device=DEV), torch.full((V, 2, 2), DEPTH_FILL, device=DEV), torch.full((V, H, W), DEPTH_FILL, device=DEV),
            torch.full((V, 2, t0 + V), -1, dtype=torch.int32, device=DEV), torch.full((1,), LSUM_FILL, dtype=torch.float64, device=DEV),
            torch.full((t0 + V, 12), W2C_FILL, device=DEV)]
    with pytest.raises(REFUSED):
        ops.window_update(torch.ones(V, H, W, 3, device=DEV), torch.ones(V, H, W, device=DEV), [0.0] * (12 * V), 1.0, ds, outs[0], outs[1], outs[2], store,
                          outs[5], t0, 3, GC.intrinsics(W, H), outs[3], w2c_new=[0.0] * (12 * V), lsum_reset=outs[4])
    torch.cuda.synchronize()
    assert _untouched(outs)


# ------------------------------------------------------------------------------------------------ log depth
LOG2F = float(np.log(np.float32(2.0)))                                       # logf(2), correctly rounded
MARKED_TOL = 4 * 2.0 ** -24                                                  # 4 ulp of logf(2): one per marked term


def test_logdepth_sum_visits_every_element_once():
    """n = 512 * 256 + 333: the capped grid takes a second pass.  Every term is an exact 0 but the first and last element of each pass"""
    prev, pts = GC.logdepth_marked()
    out = torch.full((1,), 123.0, dtype=torch.float64, device=DEV)
    ops.logdepth_sum(dev(prev), dev(pts), out)
    got = float(out)
    print(f"[geom] logdepth marked: {got!r}, expected {-4 * LOG2F!r}, off by {abs(got + 4 * LOG2F) / 2.0 ** -24:.2f} ulp of logf(2)")
    assert abs(got + 4 * LOG2F) <= MARKED_TOL
    prev, pts = GC.logdepth_random()
    ops.logdepth_sum(dev(prev), dev(pts), out)
    ref = G.logdepth_sum(prev, pts)
    print(f"[geom] logdepth random: {float(out)!r} vs {ref!r}: {abs(float(out) - ref) / prev.size:.3e} per term")
    assert abs(float(out) - ref) <= 2e-6 * prev.size


def test_logdepth_accum_adds_sum_overwrites_window_update_resets():
    prev, pts = GC.logdepth_marked()
    dprev, dpts = dev(prev), dev(pts)
    out = torch.full((1,), 5.0, dtype=torch.float64, device=DEV)
    ops.logdepth_accum(dprev, dpts, out)
    assert abs(float(out) - (5.0 - 4 * LOG2F)) <= MARKED_TOL                 # it adds to what the buffer holds
    ops.logdepth_accum(dprev, dpts, out)
    assert abs(float(out) - (5.0 - 8 * LOG2F)) <= 2 * MARKED_TOL             # twice
    rprev, rpts = GC.logdepth_random()
    ops.logdepth_accum(dev(rprev), dev(rpts), out)
    assert abs(float(out) - (5.0 - 8 * LOG2F + G.logdepth_sum(rprev, rpts))) <= 2e-6 * rprev.size + 2 * MARKED_TOL
    ops.logdepth_sum(dprev, dpts, out)
    assert abs(float(out) + 4 * LOG2F) <= MARKED_TOL                         # logdepth_sum overwrites
    launch_window(GC.window_case("mid_submap_1"), out)
    assert float(out) == 0.0                                                 # window_update resets
    ops.logdepth_accum(dprev, dpts, out)
    assert abs(float(out) + 4 * LOG2F) <= MARKED_TOL                         # the state track_frontend relies on
