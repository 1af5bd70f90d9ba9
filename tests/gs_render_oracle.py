"""fp64 evaluation, PER-ELEMENT error bounds and decision margins of the Gaussian rasteriser's binning and render passes (csrc/gs.hip:
cut3r_gs_bin, cut3r_gs_render_forward, cut3r_gs_render_backward).  CPU only (numpy); shared by tests/test_gs_render_cpu.py and
tests/test_gs_render_gpu.py.  Not collected by pytest.

The references work on the kernels' STORED inputs: the fp32 records (GS_REC floats each, layout below), `ranges`, `point_list` and, for
the backward pass, the stored forward products.  Constants of the kernels (0.99f, 1.f / 255.f, 0.0001f, 1e-12f) are the fp32 numbers they
are.  One tile is evaluated at a time as a [256 lanes, list length] array: everything local to a (pixel, entry) pair is elementwise, the
transmittance is a cumulative product and the sums are cumulative sums along the list -- in fp64 for the reference, and in fp32 with the
kernel's order of operations for the restatement (np.cumsum / np.cumprod / np.divide.accumulate run in sequence).

Error model.  Every value is carried with a first-order bound of its fp32 error (class EV): an operation adds u |result| (u = 2^-24) to
what its operands' errors propagate to, expf adds 2 u (one ulp), and an operation whose operands are exact and whose exact result is an
fp32 number adds nothing (this is what makes power = 0 at a Gaussian's own pixel, and the exactly cancelling normals of one case, exact on
both sides).  Along a list this gives the companion sums of absolute terms: the relative error of T grows by (err(1 - a) / (1 - a) + u) per
contributor, a sum S_n = sum p_j carries sum err(p_j) + u sum_j |S_j|, the back-walk T_i = T_{i+1} / (1 - a_i) the same per division,
and the suffix sum S of the backward pass u times the running sum of |v_j a_j T_j| (absolute, not signed).  A gradient slot is a sum over
pixels in a wave tree (6 levels) and one atomic per wave and entry: u (6 + waves) sum |contribution| on top of the contributions' own errors.

Decisions.  A pixel is `ambiguous` when, at any entry it visits before it is done, power lies within MARGIN x its error of 0, alpha of
1/255, test_T of 1e-4, T of 0.5 (contributing entries), or at the end nlen of 1e-12; `ambiguous_cap` when araw lies within MARGIN x its error
of 0.99 (the backward pass's sixth condition).  The comparisons are strict, so a quantity that is exact (error 0) is never ambiguous.

The constants K.  RATIO is the largest |fp32 restatement - reference| / (model bound) over the unambiguous elements of every case of
tests/gs_render_cases.py (the hand-built cases and the two scenes), measured by tests/test_gs_render_cpu.py, plus 0.05 (numpy's pairwise
sums may group differently on another host), rounded up to a decimal; K = max(1, 2 RATIO): twice what the restatement needs, since the
kernel contracts multiply-adds, uses another expf and sums gradients in a wave tree and by atomics where numpy sums pairwise.  The model is
a worst case (every rounding at its limit and in the same direction), so most ratios are below one half; there K = 1, because a bound
below the first-order worst case would no longer be a bound.

  output    measured (worst case of)      RATIO   K      dgeom slots            measured               RATIO   K
  color     0.727  (cap16)                0.8    1.6     xy (0, 1)              0.149  (scene900)      0.2    1.0
  coord     0.500  (cap16)                0.6    1.2     |d/dxy| sum (2)        0.197  (lists)         0.3    1.0
  mcoord    0.969  (cap16)                1.1    2.2     ts (3)                 0.405  (scene150)      0.5    1.0
  depth     0.224  (cap16)                0.3    1.0     conic (4..6)           0.163  (scene150)      0.3    1.0
  mdepth    0.750  (partial)              0.8    1.6     opacity (7)            0.114  (scene150)      0.2    1.0
  alpha     0.337  (lists)                0.4    1.0     rgb (8..10)            0.438  (scene150)      0.5    1.0
  normal    0.329  (scene150)             0.4    1.0     view point (11..13)    0.306  (scene150)      0.4    1.0
  aux       0.583  (scene150)             0.7    1.4     camera plane (14..19)  0.560  (tile16)        0.7    1.4
                                                         ray plane (20, 21)     0.399  (scene150)      0.5    1.0
                                                         normal (22..24)        0.502  (scene150)      0.6    1.2
  The kernels on an MI355X against K x bound (tests/test_gs_render_gpu.py): forward at most 0.47 (mdepth), backward at most 0.21.
  (mcoord and mdepth are one contributor's co / t, three or four roundings deep: a single value comes close to its worst case where a
  sum of many does not.)
"""
import numpy as np

U = 2.0 ** -24
F32, F64 = np.float32, np.float64

GS_REC, GS_TILE, GS_BATCH, GS_NGRAD = 32, 16, 256, 25
G_XY, G_DEPTH, G_TS, G_CONIC, G_OP, G_RGB, G_VP, G_CP, G_RP, G_NRM = 0, 2, 3, 4, 7, 8, 11, 14, 20, 22
G_RADIUS, G_TILES, G_RECT, G_CLAMP = 25, 26, 27, 31                    # G_RADIUS a float; G_TILES, G_RECT..G_RECT+3, G_CLAMP bit-cast ints

CAP = float(F32(0.99))
TH_ALPHA = float(F32(1.0) / F32(255.0))
TH_T = float(F32(0.0001))
TH_NLEN = float(F32(1e-12))
MARGIN = 4.0
NONE = 0xffffffff

IMAGES = (("color", 3), ("coord", 3), ("mcoord", 3), ("depth", 1), ("mdepth", 1), ("alpha", 1), ("normal", 3))
SLOT_GROUPS = (("xy", (0, 1)), ("dxy_stat", (2,)), ("ts", (3,)), ("conic", (4, 5, 6)), ("op", (7,)), ("rgb", (8, 9, 10)), ("vp", (11, 12, 13)),
               ("cp", tuple(range(14, 20))), ("rp", (20, 21)), ("nrm", (22, 23, 24)))
RATIO = {"color": 0.8, "coord": 0.6, "mcoord": 1.1, "depth": 0.3, "mdepth": 0.8, "alpha": 0.4, "normal": 0.4, "aux": 0.7,
         "xy": 0.2, "dxy_stat": 0.3, "ts": 0.5, "conic": 0.3, "op": 0.2, "rgb": 0.5, "vp": 0.4, "cp": 0.7, "rp": 0.5, "nrm": 0.6}
K = {name: max(1.0, 2.0 * r) for name, r in RATIO.items()}


def ints(col):
    """a column of bit-cast ints of the fp32 records"""
    return np.ascontiguousarray(col, dtype=F32).view(np.int32)


def host_focal(W, H, tanfovx, tanfovy):
    """fx, fy as the host wrapper hands them to the kernels: (float) W / (2.f * tanfovx) in fp32"""
    return F32(W) / (F32(2.0) * F32(tanfovx)), F32(H) / (F32(2.0) * F32(tanfovy))


def ratio(got, ref, bound, keep=None):
    """largest |got - ref| / bound over the elements of `keep`, and how many lie beyond the bound; a NaN or an error against a zero
    bound gives inf"""
    err = np.abs(np.asarray(got, dtype=F64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    r = np.where(np.isfinite(r), r, np.inf)
    if keep is not None:
        r = np.where(keep, r, 0.0)
    return (float(r.max()) if r.size else 0.0), int((r > 1.0).sum())


# ---------------------------------------------------------------------------------------------------------------- binning
def bin_reference(geom, offsets, W, H, n_inst, pad=False, mutant=None):
    """exact (point_list [n_inst] uint32, ranges [tiles, 2] uint32, overflow) of cut3r_gs_bin: keys (tile << 32) | bits(depth) written at
    each record's offset in Gaussian-id, then row-major tile order, stable sort, [start, end) per tile.  `pad`: capacity mode, unused
    entries carry tile id `tiles` and value 0 and sort behind every tile."""
    geom = np.ascontiguousarray(geom, dtype=F32)
    gx, gy = (W + GS_TILE - 1) // GS_TILE, (H + GS_TILE - 1) // GS_TILE
    tiles, rect = ints(geom[:, G_TILES]), ints(geom[:, G_RECT:G_RECT + 4])
    dbits = np.ascontiguousarray(geom[:, G_DEPTH]).view(np.uint32).astype(np.uint64)
    keys = np.full(n_inst, (gx * gy) << 32, dtype=np.uint64)
    vals = np.zeros(n_inst, dtype=np.uint32)
    written = np.zeros(n_inst, dtype=bool)
    overflow = 0
    offsets = np.asarray(offsets).astype(np.int64) & 0xffffffff
    for i in np.nonzero(tiles > 0)[0]:
        off = 0 if i == 0 else int(offsets[i - 1])
        x0, y0, x1, y1 = (int(v) for v in rect[i])
        ys, xs = np.meshgrid(np.arange(y0, y1), np.arange(x0, x1), indexing="ij")
        k = ((ys * gx + xs).reshape(-1).astype(np.uint64) << np.uint64(32)) | dbits[i]
        room = max(0, min(len(k), n_inst - off))
        overflow |= int(room < len(k))
        keys[off:off + room], vals[off:off + room], written[off:off + room] = k[:room], i, True
    assert pad or overflow or bool(written.all()), "offsets do not tile the instance buffer"
    order = np.argsort(keys, kind="stable")
    ks, point_list = keys[order], vals[order]
    ranges = np.zeros((gx * gy, 2), dtype=np.uint32)
    t = (ks >> np.uint64(32)).astype(np.int64)
    for tile in np.unique(t[t < gx * gy]):
        w = np.nonzero(t == tile)[0]
        ranges[tile] = (w[0], w[-1] + 1 - (mutant == "ranges_short"))
    return point_list, ranges, overflow


def tile_rect_reference(xy, radius, W, H):
    """gs_tile_clamp on the record's own fp32 xy and radius: fp32 sums, fp32 division by 16, truncation, clamp -> x0, y0, x1, y1"""
    gx, gy = (W + GS_TILE - 1) // GS_TILE, (H + GS_TILE - 1) // GS_TILE
    xy, rad = np.asarray(xy, dtype=F32), np.asarray(radius, dtype=F32).astype(np.int32).astype(F32)

    def tc(v, g):
        return np.clip(np.trunc(v.astype(F32) / F32(GS_TILE)).astype(np.int64), 0, g)
    hi = F32(GS_TILE - 1)
    return np.stack([tc(xy[:, 0] - rad, gx), tc(xy[:, 1] - rad, gy), tc(xy[:, 0] + rad + hi, gx), tc(xy[:, 1] + rad + hi, gy)], 1)


# ---------------------------------------------------------------------------------------- values with first-order fp32 error bounds
def _rep(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return x.astype(F32).astype(F64) == x


class EV:
    """value `v` (fp64 with an error bound `e`, or fp32 with e = None: the restatement) under the kernel's fp32 operations"""
    __slots__ = ("v", "e")
    __array_ufunc__ = None                                                 # ndarray * EV is EV.__rmul__, not an object array

    def __init__(self, v, e=None):
        self.v, self.e = v, e

    @staticmethod
    def mk(v, inh):
        if inh is None:
            return EV(v)
        exact = (inh == 0) & _rep(v)
        return EV(v, np.where(exact, 0.0, inh + U * np.abs(v)))

    @staticmethod
    def parts(o, like):
        if isinstance(o, EV):
            return o.v, o.e
        return o, (None if like.e is None else 0.0)

    def __add__(self, o):
        ov, oe = EV.parts(o, self)
        return EV.mk(self.v + ov, None if self.e is None else self.e + oe)
    __radd__ = __add__

    def __sub__(self, o):
        ov, oe = EV.parts(o, self)
        return EV.mk(self.v - ov, None if self.e is None else self.e + oe)

    def __rsub__(self, o):
        return EV.mk(o - self.v, None if self.e is None else self.e + 0.0)

    def __mul__(self, o):
        ov, oe = EV.parts(o, self)
        return EV.mk(self.v * ov, None if self.e is None else np.abs(self.v) * oe + np.abs(ov) * self.e)
    __rmul__ = __mul__

    def __truediv__(self, o):
        ov, oe = EV.parts(o, self)
        q = self.v / ov
        return EV.mk(q, None if self.e is None else (self.e + np.abs(q) * oe) / np.abs(ov))

    def __rtruediv__(self, o):
        q = o / self.v
        return EV.mk(q, None if self.e is None else np.abs(q) * self.e / np.abs(self.v))

    def __neg__(self):
        return EV(-self.v, self.e)

    def abs(self):
        return EV(np.abs(self.v), self.e)

    def exp(self):
        if self.e is None:                                                    # (the correctly rounded expf: the same bits on every host)
            return EV(np.exp(self.v.astype(F64)).astype(F32))
        v = np.exp(self.v)
        return EV(v, np.where((self.v == 0) & (self.e == 0), 0.0, v * (self.e + 2.0 * U)))

    def sqrt(self):
        v = np.sqrt(self.v)
        if self.e is None:
            return EV(v)
        with np.errstate(divide="ignore", invalid="ignore"):
            inh = np.where(v > 0, self.e / (2.0 * v), np.sqrt(self.e))
        return EV.mk(v, inh)

    def where(self, m, o):
        """self where m, else o"""
        ov, oe = EV.parts(o, self)
        return EV(np.where(m, self.v, ov), None if self.e is None else np.where(m, self.e, oe))

    def take(self, idx):
        """column idx[i] of row i (idx < 0: 0)"""
        if self.v.shape[1] == 0:
            return EV(np.zeros(len(idx), dtype=self.v.dtype), None if self.e is None else np.zeros(len(idx)))
        j = np.maximum(idx, 0)[:, None]
        g = lambda a: np.where(idx >= 0, np.take_along_axis(a, j, 1)[:, 0], 0)
        return EV(g(self.v), None if self.e is None else g(np.broadcast_to(self.e, self.v.shape)))


def _shift(a, first):
    """a along the list, one position later, `first` in front"""
    return np.concatenate([np.broadcast_to(np.asarray(first, dtype=a.dtype).reshape(-1, 1), (a.shape[0], 1)), a[:, :-1]], 1)[:, :a.shape[1]]


def _chain_sum(p, mask):
    """the running sums  p_0 + ... + p_j  over the masked entries, in sequence: EV [rows, L].  An addition is exact where everything
    before it was and the sum is an fp32 number."""
    S = np.cumsum(np.where(mask, p.v, 0).astype(p.v.dtype), axis=1, dtype=p.v.dtype)
    if p.e is None:
        return EV(S)
    pe = np.where(mask, p.e, 0.0)
    e1 = np.cumsum(pe + np.where(mask & ~_rep(S), U * np.abs(S), 0.0), axis=1)
    loc = np.where(mask & ~(_rep(S) & (_shift(e1, 0.0) == 0) & (pe == 0)), U * np.abs(S), 0.0)
    return EV(S, np.cumsum(pe + loc, axis=1))


def _last_col(a, rows):
    if a.v.shape[1] == 0:
        return EV(np.zeros(rows, dtype=a.v.dtype), None if a.e is None else np.zeros(rows))
    return EV(a.v[:, -1], None if a.e is None else a.e[:, -1])


class _Tile:
    """the lanes of one 16 x 16 tile and the records of its list, as the render kernels stage them"""

    def __init__(self, geom, ranges, point_list, W, H, tile, dt, reverse=False, shift=0):
        gx = (W + GS_TILE - 1) // GS_TILE
        lane = np.arange(GS_BATCH)
        self.px, self.py = (tile % gx) * GS_TILE + (lane & 15), (tile // gx) * GS_TILE + (lane >> 4)
        self.inside = (self.px < W) & (self.py < H)
        r0, r1 = int(ranges[tile, 0]), int(ranges[tile, 1])
        pos = np.arange(r0, r1)[::-1] if reverse else np.arange(r0, r1)
        self.ids = point_list[np.minimum(pos + shift, len(point_list) - 1)].astype(np.int64) if r1 > r0 else np.zeros(0, dtype=np.int64)
        self.L = r1 - r0
        self.G = geom[self.ids, :GS_NGRAD].astype(dt)
        self.dt, self.track = dt, dt == F64

    def f(self, k):
        return self.G[None, :, k]

    def local(self):
        """dx, dy, power, Gs = exp(power), araw = op Gs, alpha, the camera-space point co[3] and the ray distance t: EV [256, L]"""
        z = None if not self.track else 0.0
        dx = EV.mk(self.f(G_XY) - self.px[:, None].astype(self.dt), z)
        dy = EV.mk(self.f(G_XY + 1) - self.py[:, None].astype(self.dt), z)
        power = -0.5 * (self.f(G_CONIC) * dx * dx + self.f(G_CONIC + 2) * dy * dy) - self.f(G_CONIC + 1) * dx * dy
        Gs = power.exp()
        araw = self.f(G_OP) * Gs
        alpha = EV(CAP, z).where(araw.v > CAP, araw) if self.track else EV(np.minimum(F32(CAP), araw.v))
        co = [self.f(G_VP + ch) + self.f(G_CP + 2 * ch) * dx + self.f(G_CP + 2 * ch + 1) * dy for ch in range(3)]
        t = self.f(G_TS) + self.f(G_RP) * dx + self.f(G_RP + 1) * dy
        return dx, dy, power, Gs, araw, alpha, co, t


def _ray_len(px, py, W, H, fx, fy, dt, track):
    z = 0.0 if track else None
    nx = EV.mk((px.astype(dt) - dt(0.5) * dt(W)), z) / dt(fx)
    ny = EV.mk((py.astype(dt) - dt(0.5) * dt(H)), z) / dt(fy)
    return (nx * nx + ny * ny + dt(1.0)).sqrt()


# ---------------------------------------------------------------------------------------------------------------- forward pass
def _forward(geom, ranges, point_list, W, H, tanfovx, tanfovy, bg, dt, mutants=()):
    geom = np.ascontiguousarray(geom, dtype=F32)
    ranges = np.asarray(ranges).astype(np.int64).reshape(-1, 2) & 0xffffffff
    point_list = np.asarray(point_list).astype(np.int64).reshape(-1) & 0xffffffff
    track = dt == F64
    fx, fy = host_focal(W, H, tanfovx, tanfovy)
    bg = [dt(F32(b)) for b in bg]
    img = {k: np.zeros((c, H, W), dtype=dt) for k, c in IMAGES}
    img["aux"] = np.zeros((2, H, W), dtype=dt)
    bound = {k: np.zeros(v.shape) for k, v in img.items()}
    n_contrib = np.zeros((2, H, W), dtype=np.uint32)
    amb, amb_cap = np.zeros((H, W), dtype=bool), np.zeros((H, W), dtype=bool)
    for tile in range(ranges.shape[0]):
        tl = _Tile(geom, ranges, point_list, W, H, tile, dt)
        if not tl.inside.any():
            continue
        ins, L, rows = tl.inside, tl.L, GS_BATCH
        dx, dy, power, Gs, araw, alpha, co, t = tl.local()
        cand = ins[:, None] & ~(power.v > 0) & ~(alpha.v < dt(TH_ALPHA))     # contributes if the pixel gets this far
        if "skip256" in mutants and L > GS_BATCH:
            cand[:, GS_BATCH] = False
        om = 1.0 - alpha
        # T after each candidate, in sequence; its relative error grows by err(1 - a) / (1 - a) + u per contributor
        omv = np.where(cand, om.v, 1).astype(dt)
        testT = np.cumprod(omv, axis=1, dtype=dt)
        Tprev = _shift(testT, 1.0)
        stop = cand & (testT < dt(TH_T))
        nstop = np.cumsum(stop, axis=1)
        visited = ins[:, None] & (nstop - stop == 0)
        contrib = cand & (nstop == 0)
        if track:
            a_rel = np.where(cand, om.e / om.v, 0.0)
            loc0 = np.where(cand & ~_rep(testT), U, 0.0)
            e1 = np.cumsum(a_rel + loc0, axis=1)
            loc = np.where(cand & ~(_rep(testT) & (_shift(e1, 0.0) == 0) & (a_rel == 0)), U, 0.0)
            tT = EV(testT, testT * np.cumsum(a_rel + loc, axis=1))
            T = EV(Tprev, _shift(tT.e, 0.0))
        else:
            tT, T = EV(testT), EV(Tprev)
        before = contrib & ((tT.v if "before_test_T" in mutants else T.v) > dt(0.5))
        pos1 = np.arange(1, L + 1)[None, :]
        last = (pos1 * contrib).max(axis=1, initial=0)
        maxc = (pos1 * before).max(axis=1, initial=0)
        aT = alpha * T
        one = lambda p: _last_col(_chain_sum(p, contrib), rows)
        C = [one(tl.f(G_RGB + ch) * aT) for ch in range(3)]
        Nr = [one(tl.f(G_NRM + ch) * aT) for ch in range(3)]
        Co = [one(co[ch] * aT) for ch in range(3)]
        D = one(t * aT)
        weight = one(aT)
        mC = [co[ch].take(maxc - 1) for ch in range(3)]
        mD = t.take(maxc - 1)
        Tfin = tT.take(last - 1).where(last > 0, 1.0)
        ln = _ray_len(tl.px, tl.py, W, H, fx, fy, dt, track)
        has = last > 0
        z = EV(np.zeros(rows, dtype=dt), np.zeros(rows) if track else None)
        with np.errstate(divide="ignore", invalid="ignore"):
            iw = (1.0 / weight).where(has, z)
            out = {"color": [C[ch] + Tfin * bg[ch] for ch in range(3)], "alpha": [weight], "coord": [Co[ch] * iw for ch in range(3)],
                   "mcoord": mC, "depth": [D / ln * iw], "mdepth": [mD / ln]}
            nlen = (Nr[0] * Nr[0] + Nr[1] * Nr[1] + Nr[2] * Nr[2]).sqrt()
            il = 1.0 / EV(np.maximum(nlen.v, dt(TH_NLEN)), nlen.e)
            out["normal"] = [(Nr[ch] * il).where(has, z) for ch in range(3)]
            out["aux"] = [Tfin, nlen.where(has, 1.0)]
        yy, xx = tl.py[ins], tl.px[ins]
        for k, vals in out.items():
            for ch, ev in enumerate(vals):
                img[k][ch, yy, xx] = ev.v[ins]
                if track:
                    bound[k][ch, yy, xx] = np.broadcast_to(ev.e, (rows,))[ins]
        maxc_out = np.where(maxc > 0, maxc + ("maxc_plus_one" in mutants), NONE)
        n_contrib[0, yy, xx], n_contrib[1, yy, xx] = last[ins], maxc_out[ins]
        if track:
            m = MARGIN
            d_pow = np.abs(power.v) < m * power.e
            d_alpha = ~(power.v > 0) & (np.abs(alpha.v - TH_ALPHA) < m * alpha.e)
            d_T = cand & (np.abs(tT.v - TH_T) < m * tT.e)
            d_half = cand & ~stop & (np.abs(T.v - 0.5) < m * T.e)
            d_cap = cand & ~stop & (np.abs(araw.v - CAP) < m * araw.e)
            a = (visited & (d_pow | d_alpha | d_T | d_half)).any(axis=1) | (has & (np.abs(nlen.v - TH_NLEN) < m * nlen.e))
            amb[yy, xx], amb_cap[yy, xx] = a[ins], (visited & d_cap).any(axis=1)[ins]
    res = dict(img)
    res.update(n_contrib=n_contrib, bound=bound, ambiguous=amb, ambiguous_cap=amb_cap)
    return res


def render_forward_reference(geom, ranges, point_list, W, H, tanfovx, tanfovy, bg):
    """fp64: the seven images and `aux` (T_final, nlen) [C,H,W], `n_contrib` (last, maxc; 0xffffffff: no median contributor) uint32,
    `bound` (the same keys: first-order fp32 error bound per element, to be scaled by K) and the masks `ambiguous`, `ambiguous_cap` [H,W]"""
    return _forward(geom, ranges, point_list, W, H, tanfovx, tanfovy, bg, F64)


def render_forward_f32(geom, ranges, point_list, W, H, tanfovx, tanfovy, bg, mutants=()):
    """the kernel's own operation order in fp32 numpy (no bounds, no masks); `mutants`: skip256, before_test_T, maxc_plus_one"""
    return _forward(geom, ranges, point_list, W, H, tanfovx, tanfovy, bg, F32, mutants)


def products_f32(fwd):
    """what the backward pass reads of a forward result, as the fp32 / uint32 arrays the kernel stores"""
    p = {k: np.ascontiguousarray(fwd[k], dtype=F32) for k in ("aux", "alpha", "coord", "depth", "normal")}
    p["n_contrib"] = np.ascontiguousarray(fwd["n_contrib"], dtype=np.uint32)
    return p


# ---------------------------------------------------------------------------------------------------------------- backward pass
def _backward(geom, ranges, point_list, W, H, tanfovx, tanfovy, bg, products, cot, dt, mutants=()):
    geom = np.ascontiguousarray(geom, dtype=F32)
    P = geom.shape[0]
    ranges = np.asarray(ranges).astype(np.int64).reshape(-1, 2) & 0xffffffff
    point_list = np.asarray(point_list).astype(np.int64).reshape(-1) & 0xffffffff
    track = dt == F64
    fx, fy = host_focal(W, H, tanfovx, tanfovy)
    bg = [dt(F32(b)) for b in bg]
    prod = {k: np.asarray(v, dtype=F32).astype(dt) for k, v in products.items() if k != "n_contrib"}
    ncon = np.asarray(products["n_contrib"]).astype(np.int64) & 0xffffffff
    g = {k: np.asarray(c, dtype=F32).astype(dt).reshape(ch, H, W) for (k, ch), c in zip(IMAGES, cot)}
    dgeom = np.zeros((P, GS_REC), dtype=dt)
    err = np.zeros((P, GS_REC))
    mag = np.zeros((P, GS_REC))
    waves = np.zeros(P)
    zt = 0.0 if track else None
    for tile in range(ranges.shape[0]):
        tl = _Tile(geom, ranges, point_list, W, H, tile, dt, reverse=True, shift=1 if "stage_off_by_one" in mutants else 0)
        L, rows = tl.L, GS_BATCH
        if L == 0 or not tl.inside.any():
            continue
        leak = "outside_lane" in mutants
        ins = tl.inside | leak
        yy, xx = np.minimum(tl.py, H - 1), np.minimum(tl.px, W - 1)           # (lanes outside the image: read nothing, masked below)
        col = lambda a, ch=0: EV(np.where(ins, a[ch, yy, xx], 0).astype(dt).reshape(-1, 1), zt)
        last = np.where(ins, ncon[0, yy, xx], 0)[:, None]
        maxc = np.where(ins, ncon[1, yy, xx], NONE)[:, None]
        has = last > 0
        Tf, nlen = col(prod["aux"], 0), col(prod["aux"], 1)
        ln = _ray_len(tl.px, tl.py, W, H, fx, fy, dt, track)
        ln = EV(ln.v.reshape(-1, 1), None if ln.e is None else ln.e.reshape(-1, 1))
        GC = [col(g["color"], ch) for ch in range(3)]
        S0 = (GC[0] * bg[0] + GC[1] * bg[1] + GC[2] * bg[2]) * Tf
        if "no_bg_in_S" in mutants:
            S0 = S0 * 0.0
        GW = col(g["alpha"])
        GmD = col(g["mdepth"]) / ln
        GmC = [col(g["mcoord"], ch) for ch in range(3)]
        zc = EV(np.zeros((rows, 1), dtype=dt), np.zeros((rows, 1)) if track else None)
        with np.errstate(divide="ignore", invalid="ignore"):
            iw = 1.0 / col(prod["alpha"])
            GCo, dotn = [], zc
            for ch in range(3):
                gc = col(g["coord"], ch)
                GCo.append((gc * iw).where(has, zc))
                GW = (GW - gc * col(prod["coord"], ch) * iw).where(has, GW)
                dotn = dotn + col(g["normal"], ch) * col(prod["normal"], ch)
            GD = (col(g["depth"]) * iw / ln).where(has, zc)
            GW = (GW - col(g["depth"]) * col(prod["depth"]) * iw).where(has, GW)
            unit = nlen.v > dt(TH_NLEN)
            il = 1.0 / EV(np.maximum(nlen.v, dt(TH_NLEN)), nlen.e)
            GN = [((col(g["normal"], ch) - (col(prod["normal"], ch) * dotn).where(unit, zc)) * il).where(has, zc) for ch in range(3)]
        dx, dy, power, Gs, araw, alpha, co, t = tl.local()
        pos1 = (L - np.arange(L))[None, :]
        act = ins[:, None] & (pos1 <= last) & ~(power.v > 0) & ~(alpha.v < dt(TH_ALPHA))
        om = 1.0 - alpha
        # the back-walk T_i = T_{i+1} / (1 - a_i), in sequence from the stored T_final
        omv = np.where(act, om.v, 1).astype(dt)
        Tv = np.divide.accumulate(np.concatenate([np.broadcast_to(Tf.v, (rows, 1)).astype(dt), omv], 1), axis=1, dtype=dt)[:, 1:]
        T = EV(Tv, Tv * np.cumsum(np.where(act, om.e / om.v + U, 0.0), axis=1)) if track else EV(Tv)
        aT = alpha * T
        v = GW + GD * t
        for ch in range(3):
            v = v + (GC[ch] * tl.f(G_RGB + ch) + GCo[ch] * co[ch] + GN[ch] * tl.f(G_NRM + ch))
        vaT = v * aT
        # S before each entry: S0 + the terms of the entries behind it; its error uses the running sum of |terms|, not of the terms
        Sv = np.cumsum(np.concatenate([np.broadcast_to(S0.v, (rows, 1)).astype(dt), np.where(act, vaT.v, 0).astype(dt)], 1), axis=1, dtype=dt)[:, :-1]
        if track:
            absrun = np.abs(S0.v) + np.cumsum(np.where(act, np.abs(vaT.v), 0.0), axis=1)
            Se = np.broadcast_to(S0.e, (rows, 1)) + np.cumsum(np.where(act, vaT.e + U * absrun, 0.0), axis=1)
            S = EV(Sv, _shift(Se, np.broadcast_to(S0.e, (rows, 1))[:, 0]))
        else:
            S = EV(Sv)
        dalpha = v * T - S / om
        d = [None] * GS_NGRAD
        GDaT = GD * aT
        d[G_TS], d[G_RP], d[G_RP + 1] = GDaT, GDaT * dx, GDaT * dy
        ddx, ddy = GD * tl.f(G_RP) * aT, GD * tl.f(G_RP + 1) * aT
        for ch in range(3):
            d[G_RGB + ch], d[G_NRM + ch] = GC[ch] * aT, GN[ch] * aT
            ca = GCo[ch] * aT
            d[G_VP + ch], d[G_CP + 2 * ch], d[G_CP + 2 * ch + 1] = ca, ca * dx, ca * dy
            ddx, ddy = ddx + ca * tl.f(G_CP + 2 * ch), ddy + ca * tl.f(G_CP + 2 * ch + 1)
        med = pos1 == maxc
        d[G_TS], d[G_RP], d[G_RP + 1] = (d[G_TS] + GmD).where(med, d[G_TS]), (d[G_RP] + GmD * dx).where(med, d[G_RP]), \
            (d[G_RP + 1] + GmD * dy).where(med, d[G_RP + 1])
        ddx, ddy = (ddx + GmD * tl.f(G_RP)).where(med, ddx), (ddy + GmD * tl.f(G_RP + 1)).where(med, ddy)
        for ch in range(3):
            a, b, c = G_VP + ch, G_CP + 2 * ch, G_CP + 2 * ch + 1
            d[a], d[b], d[c] = (d[a] + GmC[ch]).where(med, d[a]), (d[b] + GmC[ch] * dx).where(med, d[b]), (d[c] + GmC[ch] * dy).where(med, d[c])
            ddx, ddy = (ddx + GmC[ch] * tl.f(b)).where(med, ddx), (ddy + GmC[ch] * tl.f(c)).where(med, ddy)
        free = (araw.v <= dt(CAP)) | ("cap_gradient" in mutants)              # d min(0.99, .) = 0 beyond the cap
        zl = EV(np.zeros((rows, L), dtype=dt), np.zeros((rows, L)) if track else None)
        dpow = araw * dalpha
        d[G_OP] = (Gs * dalpha).where(free, zl)
        d[G_CONIC], d[G_CONIC + 1], d[G_CONIC + 2] = (-0.5 * dx * dx * dpow).where(free, zl), (-dx * dy * dpow).where(free, zl), \
            (-0.5 * dy * dy * dpow).where(free, zl)
        ax = (-tl.f(G_CONIC) * dx - tl.f(G_CONIC + 1) * dy) * dpow
        ay = (-tl.f(G_CONIC + 2) * dy - tl.f(G_CONIC + 1) * dx) * dpow
        wx = dt(1.0) if "no_half_W" in mutants else dt(0.5) * dt(W)
        d[G_DEPTH] = (ax.abs() * wx + ay.abs() * (dt(0.5) * dt(H))).where(free, zl)
        d[G_XY], d[G_XY + 1] = (ddx + ax).where(free, ddx), (ddy + ay).where(free, ddy)
        nw = act.reshape(4, 64, L).any(axis=1).sum(axis=0)
        np.add.at(waves, tl.ids, nw)
        for k in range(GS_NGRAD):
            cv = np.where(act, d[k].v, 0).astype(dt)
            tot = cv.sum(axis=0, dtype=dt)
            np.add.at(dgeom[:, k], tl.ids, tot)                               # (fp32: one addition per tile and entry, as the atomics)
            if track:
                np.add.at(err[:, k], tl.ids, np.where(act, d[k].e, 0.0).sum(axis=0))
                np.add.at(mag[:, k], tl.ids, np.abs(cv).sum(axis=0))
    if "swap_slots" in mutants:
        dgeom[:, [G_CP + 1, G_CP + 2]] = dgeom[:, [G_CP + 2, G_CP + 1]]
    return dgeom, err + U * (6.0 + waves[:, None]) * mag


def render_backward_reference(geom, ranges, point_list, W, H, tanfovx, tanfovy, bg, products, cot):
    """fp64 dgeom [P, 32] (slots 0..24; 25..31 zero) of the stored forward `products` (n_contrib, aux, alpha, coord, depth, normal) and the
    seven cotangents `cot` (the order of IMAGES), and its first-order error bound per (Gaussian, slot), to be scaled by K"""
    return _backward(geom, ranges, point_list, W, H, tanfovx, tanfovy, bg, products, cot, F64)


def render_backward_f32(geom, ranges, point_list, W, H, tanfovx, tanfovy, bg, products, cot, mutants=()):
    """the kernel's operation order in fp32 numpy; `mutants`: stage_off_by_one, swap_slots, no_bg_in_S, cap_gradient, outside_lane, no_half_W"""
    return _backward(geom, ranges, point_list, W, H, tanfovx, tanfovy, bg, products, cot, F32, mutants)[0]




# ---------------------------------------------------------------------------------------------------------------- comparisons
def compare_forward(got, ref):
    """`got` (the seven images, aux, n_contrib) against a forward reference on its unambiguous pixels -> ({output: (largest error / (K
    bound), elements beyond)}, n_contrib entries that differ)"""
    keep = ~ref["ambiguous"]
    res = {k: ratio(got[k], ref[k], K[k] * ref["bound"][k], keep[None]) for k in [k for k, _ in IMAGES] + ["aux"]}
    return res, int(((np.asarray(got["n_contrib"]).astype(np.int64) & 0xffffffff) != ref["n_contrib"])[:, keep].sum())


def compare_backward(got, dgeom, bound):
    """`got` [P, 32] against a backward reference -> {slot group: (largest error / (K bound), elements beyond)}; "rest": slots 25..31"""
    got = np.asarray(got, dtype=F64)
    res = {name: ratio(got[:, list(s)], dgeom[:, list(s)], K[name] * bound[:, list(s)]) for name, s in SLOT_GROUPS}
    res["rest"] = (float(np.abs(got[:, GS_NGRAD:]).max()), int((got[:, GS_NGRAD:] != 0).sum()))
    return res


def rejected(res):
    return any(r[1] > 0 for r in (res[0] if isinstance(res, tuple) else res).values()) or (isinstance(res, tuple) and res[1] > 0)
