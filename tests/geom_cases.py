"""TEST INFRASTRUCTURE ONLY -- inputs of tests/test_geom_gpu.py, built on the host with fixed seeds.  Every condition a case has to
meet (no row maximum near the threshold, the mix of decisions, counts that are neither empty nor full in every camera chunk) is a
property of these arrays and of tests/geom_oracle.py: tests/test_geom_cases_cpu.py proves it without a GPU, the GPU tests assert
it again before they launch.

Patch features of the keyframe chain are TYPED rows: row = scale * (e_t + noise) with e_t a unit axis, |noise| ~ 0.2 and a
random scale in [0.5, 2] (so the normalisation matters).  Two rows of one type have similarity ~0.96, rows of different types
stay below 0.5, so with thr_sim = 0.7 the count of set K against candidate X is exactly the number of rows of K whose type
occurs in X -- planted well away from the threshold and a function of BOTH sets.  A set "at position p" holds the types
p, p+1, p+2 in near-equal shares: two sets d positions apart share 3 - d types (ratio about 1, 2/3, 1/3, 0).
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import geom as G

THR_SIM = 0.7
MATCHED_ABOVE, UNMATCHED_BELOW = 0.8, 0.5


# ------------------------------------------------------------------------------------------------ patch overlap, per element
OVERLAP_SHAPES = ((2, 8), (32, 8), (33, 16), (34, 64), (71, 64), (130, 1024))
OVERLAP_VARIANTS = ("zero", "negative", "duplicate")


@functools.lru_cache(maxsize=None)
def overlap_case(N, C, variant):
    """feat0, feat1 fp32 [N,C] and the planted rows (indices into rows 1..): half of feat1's rows are noisy copies of rows of
    feat0 (similarity ~0.9), the rest are independent; row 0 of both, which the operation drops, holds large garbage.
      zero       the last row of feat0 and (Nv >= 2) the first row of feat1 are zero: they normalise to zeros, maximum 0
      negative   channel 0 of every row of feat1 is large and positive and one row of feat0 is -e_0: every similarity of
                 that row is negative, the reported maximum is exactly 0
      duplicate  rows of feat1 are positive multiples of rows of feat0: maximum 1"""
    Nv = N - 1
    g = np.random.default_rng(1000 * N + C + 17 * OVERLAP_VARIANTS.index(variant))
    f0 = g.normal(0, 1, (N, C))
    f1 = g.normal(0, 1, (N, C))
    perm = g.permutation(Nv)
    half = Nv // 2
    f1[1 + np.arange(half)] = f0[1 + perm[:half]] + 0.48 * g.normal(0, 1, (half, C))
    f0[1:] *= g.uniform(0.25, 4.0, (Nv, 1))
    f1[1:] *= g.uniform(0.25, 4.0, (Nv, 1))
    f0[0], f1[0] = 1e3, -1e3
    planted = {}
    if variant == "zero":
        f0[Nv] = 0.0
        planted["zero0"] = Nv - 1
        if Nv >= 2:
            f1[1] = 0.0
            planted["zero1"] = 0
    elif variant == "negative":
        f1[1:, 0] = np.abs(f1[1:, 0]) + 0.4 * np.linalg.norm(f1[1:], axis=1)      # more than a third of the row's norm
        r = Nv // 2
        f0[1 + r] = 0.0
        f0[1 + r, 0] = -2.5
        planted["negative"] = r
    else:
        rows = sorted({0, Nv - 1, Nv // 3})
        for k, r in enumerate(rows):
            f1[1 + (r + 1) % Nv] = (0.5 + k) * f0[1 + r]
        planted["duplicate"] = rows
    return dict(feat0=f0.astype(np.float32), feat1=f1.astype(np.float32), planted=planted, thr=THR_SIM)


# ------------------------------------------------------------------------------------------------ keyframe chain
def typed_set(hist, Nv, C, g):
    """[Nv + 1, C] features: hist = {type: rows}; rows shuffled; row 0 garbage"""
    assert sum(hist.values()) == Nv and max(hist) < C
    types = g.permutation(np.concatenate([np.full(n, t) for t, n in sorted(hist.items())]))
    rows = (0.2 / np.sqrt(C)) * g.normal(0, 1, (Nv, C))
    rows[np.arange(Nv), types] += 1.0
    rows *= g.uniform(0.5, 2.0, (Nv, 1))
    return np.concatenate([np.full((1, C), 50.0), rows]).astype(np.float32), types


def at(p, Nv):
    a = Nv // 3
    return {p: a, p + 1: a, p + 2: Nv - 2 * a}


def expected_count(types_k, types_x):
    return int(np.isin(types_k, np.unique(types_x)).sum())


# name -> (hist of feat_last | None = candidate 0 itself, hists of the candidates, thr_ratio, forced, Nv it is tied to | None)
def _chain_spec(name, Nv):
    if name == "mixed":            # T S S S T S; candidates 2 and 3 differ from the scan against feat_last AND the previous candidate
        return at(0, Nv), [at(p, Nv) for p in (3, 2, 4, 2, 5, 4)], 0.5, None
    if name == "forced_mid":       # candidate 1 would be skipped (2/3 overlap) and is forced; candidate 2 is compared with it
        return at(0, Nv), [at(p, Nv) for p in (1, 1, 2, 3, 4)], 0.5, [0, 1, 0, 0, 0]
    if name == "forced_first":     # the empty-store start of prefetch: feat_last = feats[0], candidate 0 forced
        return None, [at(p, Nv) for p in (2, 3, 4, 5, 2)], 0.5, [1, 0, 0, 0, 0]
    if name == "tie70":            # 63 of 70 at 0.9: fp32 quotient 0.89999998 -> taken; the later counts depend on it
        assert Nv == 70
        return {0: 32, 1: 31, 7: 7}, [{0: 24, 1: 23, 2: 23}, {2: 30, 3: 40}, {3: 70}, {3: 35, 4: 35}, {3: 10, 5: 60}], 0.9, None
    if name == "tie32":            # 16 of 32 at 0.5: not taken (strict <), twice; the later counts depend on it
        assert Nv == 32
        return {0: 16, 7: 16}, [{0: 10, 1: 22}, {7: 32}, {0: 5, 7: 5, 2: 22}, {1: 32}, {1: 10, 2: 22}], 0.5, None
    raise KeyError(name)


CHAIN_CASES = tuple([("mixed", Nv, C) for Nv in (31, 33, 70) for C in (8, 64)]
                    + [("forced_mid", 33, 8), ("forced_mid", 70, 64), ("forced_first", 31, 64), ("forced_first", 33, 8)]
                    + [("tie70", 70, 8), ("tie70", 70, 64), ("tie32", 32, 8), ("tie32", 32, 64)])
# decisions worked out by hand from the positions / histograms above
CHAIN_DECISIONS = {"mixed": [1, 0, 0, 0, 1, 0], "forced_mid": [0, 1, 0, 1, 0], "forced_first": [1, 0, 1, 0, 1],
                   "tie70": [1, 1, 1, 0, 0], "tie32": [0, 0, 0, 1, 0]}


@functools.lru_cache(maxsize=None)
def chain_case(name, Nv, C):
    last_hist, hists, thr_ratio, forced = _chain_spec(name, Nv)
    g = np.random.default_rng(7919 * Nv + 31 * C + sum(map(ord, name)))
    sets = [typed_set(h, Nv, C, g) for h in hists]
    feats = np.stack([s[0] for s in sets])
    types = [s[1] for s in sets]
    if last_hist is None:
        feat_last, types_last = feats[0].copy(), types[0]
    else:
        feat_last, types_last = typed_set(last_hist, Nv, C, g)
    return dict(name=name, Nv=Nv, C=C, feat_last=feat_last, feats=feats, types_last=types_last, types=types, thr_sim=THR_SIM,
                thr_ratio=thr_ratio, forced=forced, decisions=CHAIN_DECISIONS[name])


# ------------------------------------------------------------------------------------------------ cameras and pointmaps
def rotation(r):
    """Rodrigues: rotation vector -> 3x3"""
    th = float(np.linalg.norm(r))
    if th < 1e-12:
        return np.eye(3)
    k = np.asarray(r, np.float64) / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def pose(r, t):
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = rotation(r), t
    return m


def intrinsics(W, H):
    return [0.9 * W, 0.9 * W, W / 2 - 0.5, H / 2 - 0.5]


def camera_points(K4, H, W, g, step=1):
    """camera-space points of the pixels (x*step, y*step) at depths in [2, 3]: [H/step, W/step, 3] float64"""
    ys, xs = np.meshgrid(np.arange(0, H - step + 1, step), np.arange(0, W - step + 1, step), indexing="ij")
    d = g.uniform(2.0, 3.0, ys.shape)
    return np.stack([(xs - K4[2]) / K4[0] * d, (ys - K4[3]) / K4[1] * d, d], -1)


def to_world(c2w, pc):
    return pc @ c2w[:3, :3].T + c2w[:3, 3]


FWD_CASES = tuple([(B, 768, al, cz) for B in (64, 65, 130) for al in (False, True) for cz in (True, False)]
                  + [(65, n, True, True) for n in (1, 255, 513)])
FWD_SEED_SHIFT = {(65, 1): 4}                           # chosen on the CPU: camera 64, alone in its chunk, sees the single point


@functools.lru_cache(maxsize=None)
def fwd_case(B, N, has_align):
    """one 24 x 32 pointmap (its first N points) seen by B cameras scattered around the one that produced it"""
    H, W = 24, 32
    K4 = intrinsics(W, H)
    g = np.random.default_rng(100 * B + N + (7 if has_align else 0) + FWD_SEED_SHIFT.get((B, N), 0))
    world = camera_points(K4, H, W, g).reshape(-1, 3)
    world[5] = [0.0, 0.0, -5.0]                        # behind most cameras
    c2w = np.stack([pose(g.normal(0, 0.2, 3), g.normal(0, 0.7, 3)) for _ in range(B)])
    P12, s = None, 1.0
    if has_align:                                      # raw points such that P * (s * raw) is the world pointmap
        Pm, s = pose(g.normal(0, 0.3, 3), g.normal(0, 0.5, 3)), 1.37
        world = ((world - Pm[:3, 3]) @ Pm[:3, :3]) / s
        P12 = Pm[:3, :4].reshape(-1).astype(np.float32)
    return dict(pm=np.ascontiguousarray(world[:N], dtype=np.float32), w2c=G.w2c_rows(c2w), K4=K4, W=W, H=H, P12=P12, s=s)


def fwd_reference(case, clamp_z):
    pm = case["pm"]
    if case["P12"] is not None:                        # align_view takes an image: N x 1
        pm = G.align_view(pm.reshape(-1, 1, 3), np.ones((pm.shape[0], 1), np.float32), case["P12"], case["s"], 1)[0].reshape(-1, 3)
    return G.overlap_fwd(pm, case["w2c"], case["K4"], case["W"], case["H"], clamp_z=clamp_z)


def chunks_not_vacuous(counts, N, chunk=64):
    """every chunk of 64 cameras holds a count strictly between 0 and N (N = 1, where a chunk may be one camera: every chunk
    holds a camera that sees the point, and some camera does not)"""
    for c0 in range(0, len(counts), chunk):
        c = counts[c0:c0 + chunk]
        ok = c.max() == 1 if N == 1 else bool(((c > 0) & (c < N)).any())
        if not ok:
            return False
    return N > 1 or counts.min() == 0


def box_points(n, g):
    """points of which about half fall into a camera near the origin, whatever index range is looked at"""
    return np.stack([g.uniform(-2.5, 2.5, n), g.uniform(-2.0, 2.0, n), g.uniform(1.0, 4.0, n)], -1)


@functools.lru_cache(maxsize=None)
def bwd_case(name):
    """stride  66000 points (beyond the 64 x 256 x 4 a launch covers in one pass), 3 pointmaps
       slots   7 pointmaps in slots 0..4, 6, 7 of a [8,N,3] store (grp 5, stride 6); slot 5 holds points that would ALL count
       one     a single pointmap"""
    g = np.random.default_rng({"stride": 1, "slots": 2, "one": 3}[name])
    if name == "stride":
        W, H, B, N, grp, stride, nslot = 300, 220, 3, 66000, 0, 0, 3
    elif name == "slots":
        W, H, B, N, grp, stride, nslot = 16, 12, 7, 192, 5, 6, 8
    else:
        W, H, B, N, grp, stride, nslot = 16, 12, 1, 192, 0, 0, 1
    K4 = intrinsics(W, H)
    store = np.stack([box_points(N, g) for _ in range(nslot)])
    if name == "slots":
        store[5] = np.stack([g.uniform(-0.1, 0.1, N), g.uniform(-0.1, 0.1, N), g.uniform(2.0, 3.0, N)], -1)
    c2w = pose(g.normal(0, 0.05, 3), g.normal(0, 0.1, 3))
    return dict(store=store.astype(np.float32), w2c=G.w2c_rows(c2w[None])[0], K4=K4, W=W, H=H, B=B, N=N, grp=grp, grp_stride=stride)


# ------------------------------------------------------------------------------------------------ window update
#        name          t0 (absolute), V, first, ds, base keyframe of the views handed in, w2c_new given, lsum given
WINDOW_CASES = {
    "two_chunks":     (65, 6, 3, 2, 0, True, True),          # every view sweeps both camera chunks
    "chunk_boundary": (60, 6, 3, 2, 0, True, True),          # kfi <= 64: nothing from the second chunk; kfi = 65: one camera
    "warm_up":        (0, 6, 3, 2, 0, True, True),           # keyframes 0..2 are not counted
    "mid_submap_1":   (12, 1, 3, 2, 0, True, True),          # pm_ds = store[2, 2:3]
    "mid_submap_2":   (11, 2, 3, 2, 0, True, True),          # pm_ds = store[2, 1:3]
    "mid_submap_5":   (11, 5, 3, 2, 0, True, True),          # pm_ds = store[2, 1:6]
    "not_counting":   (10, 6, 1 << 30, 2, 0, True, True),    # align and store only
    "no_w2c_new":     (10, 6, 3, 2, 0, False, True),
    "no_lsum_reset":  (10, 6, 3, 2, 0, True, False),
    "ds_one":         (10, 6, 3, 1, 0, True, True),
    "offset_views":   (15, 6, 3, 2, 5, True, True),          # store[b0 // 5:], w2c[b0:], t0 - b0
}
WIN_H, WIN_W, WIN_S, WIN_LDC = 24, 32, 1.37, 80
BEHIND = (0.0, 0.0, -1.0)                                     # fills the slots nothing may read: such a point never counts


@functools.lru_cache(maxsize=None)
def window_case(name):
    """A trajectory of t0 + V keyframes drifting sideways (0.05 per keyframe, depth 2..3: neighbours overlap almost fully,
    keyframes 40 apart not at all), their stride-ds world pointmaps in the [submaps,6,h,w,3] store (keyframe b at slot
    (b/5)*6 + b%5; every sixth slot and the slots of the window hold points behind every camera), and the window's network
    outputs: camera-space points / s, so that P_v * (s * pts_v) is the view's world pointmap."""
    t0, V, first, ds, b0, has_w2c, has_lsum = WINDOW_CASES[name]
    H, W, s = WIN_H, WIN_W, WIN_S
    h, w = H // ds, W // ds
    K4 = intrinsics(W, H)
    g = np.random.default_rng(sum(map(ord, name)))
    nkf = t0 + V
    c2w = np.stack([pose([0.0, 0.004 * k, 0.0] + g.normal(0, 0.02, 3), [0.05 * k, 0.0, 0.0] + g.normal(0, 0.03, 3)) for k in range(nkf)])
    nsub = nkf // 5 + 2
    store = np.empty((nsub * 6, h, w, 3), np.float32)
    store[:] = BEHIND
    for b in range(t0):
        store[(b // 5) * 6 + b % 5] = to_world(c2w[b], camera_points(K4, H, W, g, ds))
    pts = np.stack([camera_points(K4, H, W, g) / s for _ in range(V)]).astype(np.float32)
    conf = (1.0 + 4.0 * g.random((V, H, W))).astype(np.float32)
    return dict(name=name, t0=t0, V=V, first=first, ds=ds, b0=b0, has_w2c=has_w2c, has_lsum=has_lsum, H=H, W=W, s=s, K4=K4, ldc=WIN_LDC,
                store=store.reshape(nsub, 6, h, w, 3), w2c=G.w2c_rows(c2w), P=np.ascontiguousarray(c2w[t0:, :3, :4].reshape(V, 12), dtype=np.float32),
                pts=pts, conf=conf, dst_slot=(t0 // 5) * 6 + t0 % 5)


def window_views(case):
    """what track_frontend hands to cut3r_window_update: the store from submap b0 / 5 on, the w2c table from row b0 on, t0
    relative to b0, and the destination slot inside that store view"""
    b0 = case["b0"]
    assert b0 % 5 == 0
    h, w = case["H"] // case["ds"], case["W"] // case["ds"]
    return dict(store=case["store"][b0 // 5:].reshape(-1, h, w, 3), w2c=case["w2c"][b0:], t0=case["t0"] - b0,
                dst_slot=case["dst_slot"] - (b0 // 5) * 6)


def counted_rows_not_vacuous(case, counts):
    """every counted row (keyframe >= first, >= 1) is neither all zero nor all full over its cameras / pointmaps"""
    t0, npts = window_views(case)["t0"], (case["H"] * case["W"], (case["H"] // case["ds"]) * (case["W"] // case["ds"]))
    for v in range(case["V"]):
        kfi = t0 + v
        if kfi < case["first"] or kfi < 1:
            continue
        for d in (0, 1):
            row = counts[v, d, :kfi]
            if not row.any() or (row == npts[d]).all():
                return False
    return True


# ------------------------------------------------------------------------------------------------ log depth
LOGDEPTH_N = 512 * 256 + 333                                  # the grid is capped at 512 blocks of 256: a second pass of 333 elements
LOGDEPTH_MARKS = (0, 131071, 131072, LOGDEPTH_N - 1)


def logdepth_marked():
    """prev = 1 and z = 1 everywhere (every term an exact 0) but z = 2 at the first and last element of both passes"""
    prev = np.ones(LOGDEPTH_N, np.float32)
    pts = np.ones((LOGDEPTH_N, 3), np.float32)
    pts[:, :2] = 7.0                                          # x, y are not read
    pts[list(LOGDEPTH_MARKS), 2] = 2.0
    return prev, pts


def logdepth_random(seed=5):
    g = np.random.default_rng(seed)
    prev = (np.abs(g.normal(2, 0.3, LOGDEPTH_N)) + 0.1).astype(np.float32)
    pts = g.normal(0, 1, (LOGDEPTH_N, 3)).astype(np.float32)
    pts[:, 2] = np.abs(pts[:, 2]) + 0.5
    return prev, pts
