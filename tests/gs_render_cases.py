"""The cases of tests/test_gs_render_cpu.py and tests/test_gs_render_gpu.py: hand-built fp32 records (written directly in the layout of
tests/gs_render_oracle.py; isotropic or axis-aligned conics) and the inputs of two small scenes.  Not collected by pytest.

Every hand-built case scatters its records over a larger, otherwise empty record array (G_TILES = 0: never referenced) in an order
unrelated to depth, so ids are not in list order.  `about` marks the pixels a case exists for: none of them may be ambiguous.

  tile16   16 x 16, one full tile, 40 Gaussians of mixed size and opacity
  one      1 x 1
  cap16    16 x 16: a Gaussian with G_OP = 1.5 on pixel (4, 4) (araw 1.5 there, 1.17 one pixel away, 0.91 on the diagonal, 0.55 two
           away: the min(0.99, .) cap and its edge), and two entries on pixel (11, 11) whose weighted normals cancel exactly.  Two
           successive entries cannot have EQUAL fp32 weights a T below the cap (a_2 = a_1 / (1 - a_1) is never a dyadic number < 1 for a
           dyadic a_1), so the weights are 1/2 and 1/4 and the normals n and -2 n: n a T cancels exactly in fp32 and in fp64, nlen = 0
  partial  17 x 33 (H x W): 2 x 3 tiles with a column of 1-pixel-wide and a row of 1-pixel-high partial tiles; one Gaussian spans all six
           tiles, several are centred beyond the image edge so that lanes outside the image see large alphas
  lists    48 x 64, 12 tiles (4 bits of tile id with the pad id), by tile:
             0  empty                               6  513 entries, alpha 0.8: every pixel done at entry 6, inside the first round
             1  1 entry                             7  300 entries: 20 row Gaussians end rows 0-3 (one wave) early, rows 4-15 run on
             2  255 entries, alpha ~ 0.006 (*)      8  alpha 0.6 first: T crosses 0.5 at contributor 1
             3  256                                 9  256 entries below 1/255, then alpha 0.6: T crosses 0.5 at contributor 257
             4  257                                10  2 entries
             5  513                                11  5 entries below 1/255: nothing contributes, maxc stays 0xffffffff
           in tiles 3, 4, 5 entries 256 and 257 are pure red and pure green.  (*) Entry 100 of tiles 2..5 (entry 60 of tile 7) has alpha 0.3
           (0.4): T steps from 0.55 to 0.39 there instead of creeping through 0.5 in steps of 0.3 %, which would leave the median
           contributor of one pixel in a hundred within the rounding error of T."""
import math

import numpy as np

from tests import gs_render_oracle as RO
from tests.gs_render_oracle import F32, G_CONIC, G_CP, G_DEPTH, G_NRM, G_OP, G_RADIUS, G_RECT, G_RGB, G_RP, G_TILES, G_TS, G_VP, G_XY, GS_REC


class _Builder:
    def __init__(self, name, H, W, P, seed, tan=(0.5, 0.4), bg=(0.1, 0.2, 0.3)):
        self.name, self.H, self.W, self.P = name, H, W, P
        self.tanx, self.tany, self.bg = tan[0], tan[1], bg
        self.rng = np.random.default_rng(seed)
        self.geom = np.zeros((P, GS_REC), dtype=F32)
        self.free = list(self.rng.permutation(P))
        self.about = np.zeros((H, W), dtype=bool)
        self.gx, self.gy = (W + 15) // 16, (H + 15) // 16

    def add(self, xy, depth, conic, op, rect, rgb=None, nrm=None):
        r, i = self.rng, int(self.free.pop())
        g = self.geom[i]
        conic = (conic, 0.0, conic) if np.isscalar(conic) else conic
        g[G_XY:G_XY + 2], g[G_DEPTH], g[G_CONIC:G_CONIC + 3], g[G_OP] = xy, depth, conic, op
        g[G_TS] = depth * (1.0 + 0.1 * r.random())
        g[G_RGB:G_RGB + 3] = r.random(3) * 0.4 + 0.2 if rgb is None else rgb
        g[G_VP:G_VP + 3] = (r.normal() * 0.5, r.normal() * 0.5, depth)
        g[G_CP:G_CP + 6] = r.normal(size=6) * 0.03
        g[G_RP:G_RP + 2] = r.normal(size=2) * 0.02
        n = r.normal(size=3)
        g[G_NRM:G_NRM + 3] = n / np.linalg.norm(n) if nrm is None else nrm
        g[G_RADIUS] = math.ceil(3.0 / math.sqrt(max(max(conic[0], conic[2]), 1e-4)))
        x0, y0, x1, y1 = rect
        assert 0 <= x0 < x1 <= self.gx and 0 <= y0 < y1 <= self.gy
        g[G_TILES:G_TILES + 5] = np.array([(x1 - x0) * (y1 - y0), x0, y0, x1, y1], dtype=np.int32).view(F32)
        return i

    def own_rect(self, xy, conic):
        """the tiles within three standard deviations, as gs_tile_clamp gives them"""
        rad = math.ceil(3.0 / math.sqrt(conic))
        rect = RO.tile_rect_reference(np.array([xy], dtype=F32), np.array([rad], dtype=F32), self.W, self.H)[0]
        return tuple(int(v) for v in rect)

    def fill(self, tile, n, op, conic, depth0, mark=(), jump=()):
        """n entries of one tile, centred at random inside it, depth rising with the entry; `mark`: {entry (1-based): rgb}, `jump`:
        {entry: opacity}"""
        tx, ty = tile % self.gx, tile // self.gx
        for k in range(n):
            xy = (16 * tx + self.rng.random() * 15.0, 16 * ty + self.rng.random() * 15.0)
            o = op if np.isscalar(op) else op[0] + (op[1] - op[0]) * self.rng.random()
            o = dict(jump).get(k + 1, o)
            self.add(xy, depth0 + 1e-3 * k, conic, o, (tx, ty, tx + 1, ty + 1), rgb=dict(mark).get(k + 1))

    def mark(self, tile, local):
        tx, ty = tile % self.gx, tile // self.gx
        for (y, x) in local:
            if 16 * ty + y < self.H and 16 * tx + x < self.W:
                self.about[16 * ty + y, 16 * tx + x] = True

    def done(self):
        tiles = RO.ints(self.geom[:, G_TILES]).astype(np.int64)
        offsets = np.cumsum(tiles).astype(np.uint32)
        return dict(name=self.name, H=self.H, W=self.W, P=self.P, tanx=self.tanx, tany=self.tany, bg=self.bg, geom=self.geom, offsets=offsets,
                    n_inst=int(offsets[-1]), about=self.about)


def case_tile16():
    b = _Builder("tile16", 16, 16, 64, 1)
    for k in range(40):
        c = 0.02 + 0.28 * b.rng.random()
        b.add((b.rng.random() * 20 - 2, b.rng.random() * 20 - 2), 1.0 + b.rng.random(), c, 0.1 + 0.8 * b.rng.random(), (0, 0, 1, 1))
    return b.done()


def case_one():
    b = _Builder("one", 1, 1, 16, 2)
    for xy, op in (((0.25, -0.5), 0.3), ((-0.75, 0.5), 0.5), ((0.0, 0.0), 0.4)):
        b.add(xy, 1.0 + b.rng.random(), 0.3, op, (0, 0, 1, 1))
    b.about[0, 0] = True
    return b.done()


CAP_PIXEL, CANCEL_PIXEL = (4, 4), (11, 11)


def case_cap16():
    b = _Builder("cap16", 16, 16, 32, 3)
    b.add((4.0, 4.0), 1.0, 0.5, 1.5, (0, 0, 1, 1))
    n = np.array([0.5, -0.25, 0.75])
    b.add((11.0, 11.0), 1.5, 0.5, 0.5, (0, 0, 1, 1), nrm=n)
    b.add((11.0, 11.0), 2.0, 0.5, 0.5, (0, 0, 1, 1), nrm=-2.0 * n)
    b.mark(0, [(4, 4), (4, 5), (5, 5), (4, 6), (6, 4), (11, 11), (11, 12), (10, 10)])
    return b.done()


def case_partial():
    b = _Builder("partial", 17, 33, 96, 4)
    b.add((16.0, 8.0), 1.0, 0.004, 0.5, (0, 0, 3, 2))                         # spans all six tiles
    for k in range(36):
        c = 0.03 + 0.2 * b.rng.random()
        if k < 12:                                                            # centred beyond the right / lower edge: the partial tiles' dead lanes
            xy = (33.0 + 6 * b.rng.random(), 17 * b.rng.random()) if k % 2 else (33 * b.rng.random(), 17.0 + 6 * b.rng.random())
        else:
            xy = (b.rng.random() * 33, b.rng.random() * 17)
        b.add(xy, 1.1 + b.rng.random(), c, 0.15 + 0.7 * b.rng.random(), b.own_rect(xy, c))
    for y, x in ((16, 32), (0, 32), (16, 0), (8, 16)):
        b.about[y, x] = True
    return b.done()


LISTS_LEN = {0: 0, 1: 1, 2: 255, 3: 256, 4: 257, 5: 513, 6: 513, 7: 300, 8: 6, 9: 267, 10: 2, 11: 5}
_PROBE = [(0, 0), (15, 15), (7, 8), (3, 12)]


def case_lists():
    b = _Builder("lists", 48, 64, 4000, 5)
    red_green = {256: (1.0, 0.0, 0.0), 257: (0.0, 1.0, 0.0)}
    b.fill(1, 1, 0.3, 0.01, 1.0)
    for tile in (2, 3, 4, 5):
        b.fill(tile, LISTS_LEN[tile], (0.005, 0.007), 2e-4, 1.0, mark=red_green, jump={100: 0.3})
    b.fill(6, 513, 0.8, 1e-5, 1.0)
    for k in range(20):                                                       # rows: constant along x, alpha 0.79 / 0.29 / 0.04 / below 1/255 by row
        b.add((48.0 + 8.0, 16.0 + (0.5 if k % 2 == 0 else 2.5)), 1.0 + 1e-3 * k, (0.0, 0.0, 1.0), 0.9, (3, 1, 4, 2))
    b.fill(7, 280, (0.005, 0.007), 2e-4, 2.0, jump={40: 0.4})
    b.fill(8, 1, 0.6, 1e-4, 1.0)
    b.fill(8, 5, 0.05, 1e-3, 2.0)
    b.fill(9, 256, 0.001, 1e-4, 1.0)
    b.fill(9, 1, 0.6, 1e-4, 2.0)
    b.fill(9, 10, 0.05, 1e-3, 3.0)
    b.fill(10, 2, 0.4, 0.01, 1.0)
    b.fill(11, 5, 0.001, 1e-4, 1.0)
    for tile in range(1, 12):
        b.mark(tile, _PROBE)
    b.mark(7, [(0, 5), (3, 9), (4, 9), (15, 2)])
    return b.done()


HAND_BUILT = {"tile16": case_tile16, "one": case_one, "cap16": case_cap16, "partial": case_partial, "lists": case_lists}
SCENES = {"scene150": (33, 47, 150, (-0.1, 0.1, (0.0, 0.1, 0.0))), "scene900": (40, 56, 900, (0.05, 0.05, (0.0, 0.0, 0.5)))}
_CACHE = {}


def hand_built(name):
    if name not in _CACHE:
        _CACHE[name] = HAND_BUILT[name]()
    return _CACHE[name]


def scene_inputs(name):
    """fp64 torch inputs of a scene in the style of tests/test_gs_gpu.py (_scene, _w2c): means, scales, quaternions, opacities, colours and
    the oracle's settings dict"""
    import torch
    from oracle import gs_oracle as GO
    H, W, P, (rx, ry, t) = SCENES[name]
    g = torch.Generator().manual_seed(P)
    f64 = torch.float64
    means = torch.randn(P, 3, generator=g, dtype=f64) * 0.8 + torch.tensor([0.0, 0.0, 3.0], dtype=f64)
    means[:4, 2] = -1.0                                                       # behind the camera: culled
    scales = torch.rand(P, 3, generator=g, dtype=f64) * 0.22 + 0.03
    scales[4:7, 2] = 1e-5                                                     # flat Gaussians
    q = torch.randn(P, 4, generator=g, dtype=f64)
    q = q / q.norm(dim=-1, keepdim=True)
    op = torch.rand(P, 1, generator=g, dtype=f64) * 0.85 + 0.1
    colors = torch.rand(P, 3, generator=g, dtype=f64)
    cx, sx, cy, sy = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry)
    M = torch.eye(4, dtype=f64)
    M[:3, :3] = torch.tensor([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], dtype=f64) @ torch.tensor([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=f64)
    M[:3, 3] = torch.tensor(t, dtype=f64)
    st = GO.camera_settings(H, W, 1.0, 1.0 * H / W, M, bg=(0.1, 0.2, 0.3), sh_degree=0, kernel_size=0.0)
    return means, scales, q, op, colors, st


def scene_stand_in(name):
    """the scene as a case without a GPU: records from the fp64 projection of oracle/gs_oracle.py rounded to fp32 (the kernels' own records
    differ in the last bits; the GPU test takes theirs)"""
    if name in _CACHE:
        return _CACHE[name]
    from oracle import gs_oracle as GO
    means, scales, q, op, colors, st = scene_inputs(name)
    H, W, P = SCENES[name][:3]
    g = GO.preprocess(means, op, scales, q, None, colors, st)
    vis = g["visible"].numpy()
    geom = np.zeros((P, GS_REC), dtype=F32)
    n = lambda k: g[k].numpy()
    geom[:, G_XY:G_XY + 2], geom[:, G_DEPTH], geom[:, G_TS], geom[:, G_CONIC:G_CONIC + 3], geom[:, G_OP] = n("xy"), n("depth"), n("ts"), n("conic"), n("opacity")
    geom[:, G_RGB:G_RGB + 3], geom[:, G_VP:G_VP + 3], geom[:, G_CP:G_CP + 6] = n("colour"), n("view_point"), n("camera_plane")
    geom[:, G_RP:G_RP + 2], geom[:, G_NRM:G_NRM + 3], geom[:, G_RADIUS] = n("ray_plane"), n("normal"), n("radii")
    rect = n("rect").astype(np.int32)
    tiles = ((rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1])).astype(np.int32)
    geom[:, G_TILES] = tiles.view(F32)
    geom[:, G_RECT:G_RECT + 4] = rect.view(F32)
    geom[~vis] = 0
    offsets = np.cumsum(RO.ints(geom[:, G_TILES]).astype(np.int64)).astype(np.uint32)
    _CACHE[name] = dict(name=name, H=H, W=W, P=P, tanx=float(st["tanfovx"]), tany=float(st["tanfovy"]), bg=(0.1, 0.2, 0.3), geom=geom, offsets=offsets,
                        n_inst=int(offsets[-1]), about=np.zeros((H, W), dtype=bool))
    return _CACHE[name]


def cotangents(case, zero_at, seed=7):
    """random cotangents on all seven images (fp32), zero on the pixels of `zero_at`"""
    r = np.random.default_rng(seed)
    return [np.where(zero_at[None], 0, r.normal(size=(c, case["H"], case["W"]))).astype(F32) for _, c in RO.IMAGES]


_REF = {}


def reference(case):
    """the binning, forward and backward references of a case, computed once and left unchanged: point_list, ranges, the argument tuple
    `args` of the render references, `fwd`, the pixels `amb` whose cotangents are zero (ambiguous | ambiguous_cap), the fp32 `products`
    the backward pass is fed, the cotangents `cot`, `dgeom` and its bound `dbound`"""
    if case["name"] not in _REF:
        pl, rg, overflow = RO.bin_reference(case["geom"], case["offsets"], case["W"], case["H"], case["n_inst"])
        assert overflow == 0
        args = (case["geom"], rg, pl, case["W"], case["H"], case["tanx"], case["tany"], case["bg"])
        fwd = RO.render_forward_reference(*args)
        amb = fwd["ambiguous"] | fwd["ambiguous_cap"]
        products, cot = RO.products_f32(fwd), cotangents(case, amb)
        dgeom, dbound = RO.render_backward_reference(*args, products, cot)
        _REF[case["name"]] = dict(point_list=pl, ranges=rg, args=args, fwd=fwd, amb=amb, products=products, cot=cot, dgeom=dgeom, dbound=dbound)
    return _REF[case["name"]]
