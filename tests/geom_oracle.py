"""TEST INFRASTRUCTURE ONLY -- references of the tracking-geometry kernels (csrc/geometry.hip) for tests/test_geom_gpu.py and
tests/test_geom_cases_cpu.py.  Float64 numpy for the patch-overlap arithmetic; oracle.geom (oracle/oracle_geom.c) for everything
that is bit-exact.

Tolerances (u = 2^-24, C feature channels), derived from the arithmetic and never from what a kernel returned:

* normalised rows:  |got - ref64| <= (C/2 + 3) u |ref64| + 2^-126.
  The fp32 sum of C squares, in any order, has relative error <= C u (one rounding per square, C - 1 per addition chain at
  worst); the square root halves that and adds u; the division adds u; one u of slack.  2^-126 covers a quotient that lands in
  the denormal range (rounded there with an absolute, not a relative, error -- or flushed).  A zero row divides 0 by the 1e-12
  floor: exactly 0.
* row maxima:  |got - max(ref64, 0)| <= (2C + 6) u.
  The dot product of two unit rows accumulates at most C u, whatever the order, because sum |a_i b_i| <= 1; each operand
  carries the row bound above, (C/2 + 3) u relative, i.e. (C + 6) u for the two.  8e-6 at C = 64, 1.2e-4 at C = 1024.  The
  kernels report max(0, maximum): a row whose every similarity is negative reads exactly 0.
* counts and decisions: exact.  chain_scan returns every row's distance |maximum - thr_sim|; a case is valid only when no
  distance is within (2C + 6) u, a condition on the INPUTS that the CPU test proves and the GPU test asserts again before it
  launches.  It is not a band a test may subtract from a count.
* decision:  ratio = fp32(count) / fp32(Nv) widened to double, take = forced or ratio < thr_ratio (double).  63 of 70 at 0.9
  is taken (0.89999998 < 0.9); 16 of 32 at 0.5 is not (0.5 is exact in both precisions and the comparison is strict).
* log-depth sums:  device logf and libm logf differ by <= 2 ulp per term: 2e-6 per term against G.logdepth_sum (the bound of
  test_align_view_bit_exact_and_logdepth).  That cannot notice one lost element, so the marked case of the GPU test makes
  every term an exact 0 but four, and bounds the sum by 4 ulp of logf(2) = 4 * 2^-24 (logf(2) lies in [0.5, 1), ulp 2^-24 at
  its upper end: 1 ulp of device logf per marked term).
* overlap counts, stored pointmaps, confidences, depths: bit for bit (geometry.hip is built without contraction and repeats
  the operation order of oracle_geom.c).
"""
from __future__ import annotations

import numpy as np

from oracle import geom as G

U = 2.0 ** -24
TINY = 2.0 ** -126


def row_bound(C):
    """relative bound of one normalised element (add TINY absolute)"""
    return (C / 2 + 3) * U


def max_bound(C):
    """absolute bound of one row maximum, and the half-width of the band around thr_sim no row of a valid case lies in"""
    return (2 * C + 6) * U


def normalised_rows64(feat):
    """rows 1.. of feat in float64, divided by max(norm, 1e-12) (F.normalize; row 0 is dropped as the reference drops it)"""
    a = np.asarray(feat, np.float64)[1:]
    return a / np.maximum(np.sqrt((a * a).sum(axis=1, keepdims=True)), 1e-12)


def row_maxima64(f0, f1):
    """for each normalised row of f0 the maximum similarity over the normalised rows of f1: sim.max(dim=1) of
    compute_patch_overlap_ratio.  Not clamped: a row whose every similarity is negative returns that negative maximum."""
    return (normalised_rows64(f0) @ normalised_rows64(f1).T).max(axis=1)


def ratio_of(count, Nv):
    """the quotient the decision is taken on: fp32 / fp32, widened"""
    return float(np.float32(count) / np.float32(Nv))


def chain_scan(feat_last, feats, thr_sim, thr_ratio, forced=None):
    """The sequential scan of cut3r_patch_overlap_chain.  Candidate i is compared with the last kept set -- feat_last at first,
    then the most recent taken or forced candidate; count = #row maxima above thr_sim; take = forced[i] or
    ratio_of(count, Nv) < thr_ratio.  A forced candidate reports count 0 and take 1 (no similarity is computed for it).
    Returns counts [B], decisions [B], the final state (-1 | index of the last kept candidate), per step every row's
    distance |maximum - thr_sim| (None for a forced step) and, per step, the index of the set compared with (-1 = feat_last)."""
    B = len(feats)
    Nv = np.asarray(feat_last).shape[0] - 1
    counts, decisions, dist, against = np.zeros(B, np.int32), np.zeros(B, np.int32), [], []
    state = -1
    for i in range(B):
        against.append(state)
        if forced is not None and forced[i]:
            counts[i], decisions[i] = 0, 1
            dist.append(None)
        else:
            mx = row_maxima64(feat_last if state < 0 else feats[state], feats[i])
            counts[i] = int((mx > thr_sim).sum())
            decisions[i] = int(ratio_of(counts[i], Nv) < thr_ratio)
            dist.append(np.abs(mx - thr_sim))
        if decisions[i]:
            state = i
    return dict(counts=counts, decisions=decisions, state=state, dist=dist, against=against)


def min_distance(scan):
    d = [x.min() for x in scan["dist"] if x is not None]
    return min(d) if d else np.inf


def slot_of(b, grp, grp_stride):
    """store slot of keyframe b (cut3r_overlap_bwd)"""
    return b if grp == 0 else (b // grp) * grp_stride + b % grp


def window_reference(pts, conf, P12s, s, ds, store, dst_slot, w2c, t0, first, K4, ldc, grp=5, grp_stride=6, w2c_new=None):
    """cut3r_window_update from oracle.geom alone, so that every comparison is bit for bit.
    pts [V,H,W,3], conf [V,H,W]; store [slots,h,w,3] (the view cut3r_window_update is given, slot 0 = its first pointmap);
    dst_slot: slot of `store` that receives view 0 (views are consecutive); w2c [>= t0+V, 12]; w2c_new [V,12] or None.
    Returns the store, the w2c table, conf_ds [V,h,w], depth [V,H,W] after the call and counts [V,2,ldc]:
      forward   G.overlap_fwd of the view's full-resolution aligned pointmap (G.align_view with ds = 1: the same FMA chain)
                against cameras 0..kfi-1 with the z clamp;
      backward  G.overlap_bwd of the stored pointmaps 0..kfi-1 (slot addressing, AFTER this window's views are stored) against
                camera kfi with bounds W/ds x H/ds and the full-resolution intrinsics;
      zero rows for kfi < first, zeros from kfi to ldc."""
    pts, conf = np.asarray(pts, np.float32), np.asarray(conf, np.float32)
    V, H, W = conf.shape
    h, w = H // ds, W // ds
    P = np.asarray(P12s, np.float32).reshape(V, 12)
    store = np.array(store, np.float32).reshape(-1, h, w, 3)
    w2c = np.array(w2c, np.float32)
    if w2c_new is not None:
        w2c[t0:t0 + V] = np.asarray(w2c_new, np.float32).reshape(V, 12)
    conf_ds, depth = np.zeros((V, h, w), np.float32), np.zeros((V, H, W), np.float32)
    for v in range(V):
        store[dst_slot + v], conf_ds[v], depth[v] = G.align_view(pts[v], conf[v], P[v], s, ds)
    counts = np.zeros((V, 2, ldc), np.int32)
    ones = np.ones((H, W), np.float32)
    for v in range(V):
        kfi = t0 + v
        if kfi < first or kfi < 1:
            continue
        full = G.align_view(pts[v], ones, P[v], s, 1)[0]
        counts[v, 0, :kfi] = G.overlap_fwd(full, w2c[:kfi], K4, W, H, clamp_z=True)
        slots = [slot_of(b, grp, grp_stride) for b in range(kfi)]
        counts[v, 1, :kfi] = G.overlap_bwd(store[slots], w2c[kfi], K4, w, h)
    return dict(store=store, w2c=w2c, conf_ds=conf_ds, depth=depth, counts=counts)
