"""cut3r_gs_bin, cut3r_gs_render_forward and cut3r_gs_render_backward (csrc/gs.hip), each called on its own through the C ABI and compared
PER ELEMENT with the fp64 references of tests/gs_render_oracle.py on the cases of tests/gs_render_cases.py: five sets of hand-built fp32
records and the records the kernels themselves project for two small scenes.

Binning is exact.  The render passes take hard decisions per pixel and entry; the reference knows how far each deciding quantity lies
from its threshold, pixels with a decision inside 4 x its fp32 error are `ambiguous` and left out (at most 2 % per case, none of the pixels a
hand-built case is about), and EVERY other element must lie within its own first-order bound -- no percentile, no share beyond a
tolerance.  The backward pass is fed the reference's forward products rounded to fp32 and cotangents that are zero on the ambiguous
pixels, so it is judged independently of the forward kernel.  Every output lies inside a larger allocation whose margins must stay intact.

Measured on an MI355X, largest error / bound (with K applied) over the seven cases; no pixel of any case was ambiguous there:
  forward   color 0.455, coord 0.417, mcoord 0.441, depth 0.224, alpha 0.265, aux 0.262 (all cap16), mdepth 0.469 (partial), normal 0.173 (lists)
  backward  xy 0.152, |d/dxy| sum 0.148, ts 0.201, conic 0.177, opacity 0.160, rgb 0.201, view point 0.191, camera plane 0.14, ray plane 0.201,
            normal 0.194 (scene900 but for the camera plane; the hand-built cases stay below 0.15; the atomics' order moves these a little)
Each test prints its own figures as `[gs stage] ...`."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pytestmark = pytest.mark.gpu

from cut3r_slam_amd import _lib  # noqa: E402
from cut3r_slam_amd import gaussian_rasterizer as GR  # noqa: E402
from tests import gs_render_cases as GC  # noqa: E402
from tests import gs_render_oracle as RO  # noqa: E402

DEV = "cuda:0"
CASES = tuple(GC.HAND_BUILT) + tuple(GC.SCENES)
MARGIN = 64                                                                 # guard elements on either side of every output
MAX_AMBIGUOUS = 0.02


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _arr(vals):
    return (C.c_float * len(vals))(*[float(v) for v in vals])


class Guarded:
    """a tensor inside a larger allocation filled with a sentinel (the tensor itself included: whatever survives was not written)"""

    def __init__(self, shape, dtype):
        n = max(1, int(np.prod(shape)))
        fill = -3.0e38 if dtype == torch.float32 else 0x5a5a5a5a
        self.whole = torch.full((n + 2 * MARGIN,), fill, dtype=dtype, device=DEV)
        self.t = self.whole[MARGIN:MARGIN + n].view(*shape) if int(np.prod(shape)) else self.whole[MARGIN:MARGIN + n]
        self.fill, self.ref = fill, self.whole[:MARGIN].clone()

    def intact(self):
        return torch.equal(self.whole[:MARGIN], self.ref) and torch.equal(self.whole[-MARGIN:], self.ref)

    def written(self):
        return bool((self.t != self.fill).all())

    def np(self):
        return self.t.cpu().numpy()


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a).astype(dtype)).to(DEV).contiguous()


_SCENE = {}


def _scene(name):
    """the scene through cut3r_gs_preprocess (for tiles_touched and offsets) and through GR._forward (the buffers the rasteriser keeps)"""
    if name in _SCENE:
        return _SCENE[name]
    lib = _lib.load()
    means, scales, q, op, colors, st = GC.scene_inputs(name)
    H, W, P = GC.SCENES[name][:3]
    f = lambda t: t.float().to(DEV).contiguous()
    settings = GR.GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=st["tanfovx"], tanfovy=st["tanfovy"], kernel_size=0.0,
                                                bg=f(st["bg"]), scale_modifier=1.0, viewmatrix=f(st["viewmatrix"]), projmatrix=f(st["projmatrix"]),
                                                sh_degree=0, campos=f(st["campos"]), prefiltered=False, require_depth=True, require_coord=True,
                                                debug=False)
    t = dict(means=f(means), scales=f(scales), rots=f(q), opac=f(op), colors=f(colors))
    out, radii, buf = GR._forward(t["means"], None, t["colors"], t["opac"], t["scales"], t["rots"], settings)
    geom = Guarded((P, RO.GS_REC), torch.float32)
    radii2, tiles, offsets = (Guarded((P,), torch.int32) for _ in range(3))
    ws = torch.empty(GR.workspace_bytes(P, 0), dtype=torch.uint8, device=DEV)
    rc = lib.cut3r_gs_preprocess(P, _p(t["means"]), _p(t["scales"]), _p(t["rots"]), _p(t["opac"]), None, 0, 0, _p(t["colors"]),
                                 GR._host16(settings.viewmatrix, 16), GR._host16(settings.projmatrix, 16), GR._host16(settings.campos, 3), W, H,
                                 float(st["tanfovx"]), float(st["tanfovy"]), 0.0, 1.0, _p(geom.t), _p(radii2.t), _p(tiles.t), _p(offsets.t), _p(ws),
                                 ws.numel(), None)
    torch.cuda.synchronize()
    assert rc == 0 and all(g.intact() and g.written() for g in (geom, radii2, tiles, offsets))
    g = geom.np()
    off = offsets.np().view(np.uint32)
    case = dict(name=name + "@kernels", H=H, W=W, P=P, tanx=float(st["tanfovx"]), tany=float(st["tanfovy"]), bg=(0.1, 0.2, 0.3), geom=g, offsets=off,
                n_inst=int(off[-1]), about=np.zeros((H, W), dtype=bool))
    _SCENE[name] = dict(case=case, out=out, radii=radii, buf=buf, radii2=radii2.np(), tiles=tiles.np(), settings=settings)
    return _SCENE[name]


def _case(name):
    return GC.hand_built(name) if name in GC.HAND_BUILT else _scene(name)["case"]


def _bin(c, n_inst, capacity_mode):
    """cut3r_gs_bin on the case's records -> (rc, point_list, ranges, overflow flag or None), margins checked"""
    lib = _lib.load()
    n, tiles = max(1, n_inst), ((c["W"] + 15) // 16) * ((c["H"] + 15) // 16)
    geom, offsets = _dev(c["geom"], np.float32), _dev(c["offsets"].view(np.int32), np.int32)
    keys_tmp, keys_sorted = Guarded((n,), torch.int64), Guarded((n,), torch.int64)
    vals_tmp, point_list, ranges = Guarded((n,), torch.int32), Guarded((n,), torch.int32), Guarded((tiles, 2), torch.int32)
    overflow = Guarded((1,), torch.int32) if capacity_mode else None
    if overflow is not None:
        overflow.t.zero_()
    ws = torch.empty(GR.workspace_bytes(c["P"], n_inst), dtype=torch.uint8, device=DEV)
    rc = lib.cut3r_gs_bin(c["P"], _p(geom), _p(offsets), n_inst, c["W"], c["H"], _p(keys_tmp.t), _p(vals_tmp.t), _p(keys_sorted.t), _p(point_list.t),
                          _p(ranges.t), _p(ws), ws.numel(), _p(overflow.t) if overflow is not None else None, None)
    torch.cuda.synchronize()
    assert all(g.intact() for g in (keys_tmp, keys_sorted, vals_tmp, point_list, ranges) + ((overflow,) if overflow is not None else ()))
    return rc, point_list.np().view(np.uint32), ranges.np().view(np.uint32), (int(overflow.np()[0]) if overflow is not None else None)


@pytest.mark.parametrize("name", CASES)
def test_binning_is_exact_also_in_capacity_mode(name):
    c = _case(name)
    r = GC.reference(c)
    n = c["n_inst"]
    rc, pl, rg, _ = _bin(c, n, False)
    assert rc == 0 and np.array_equal(rg, r["ranges"]) and np.array_equal(pl[:n], r["point_list"])
    rc, pl, rg, flag = _bin(c, n + 300, True)                               # a capacity above the count: padded behind every tile
    assert rc == 0 and flag == 0 and np.array_equal(rg, r["ranges"]) and np.array_equal(pl[:n], r["point_list"]) and (pl[n:] == 0).all()
    rc, pl, rg, flag = _bin(c, n - 1, True)                                 # one short: flagged
    assert rc == 0 and flag == 1
    tiles = rg.shape[0]
    print(f"[gs stage] {name}: binning exact, {n} instances over {tiles} tiles ({32 + tiles.bit_length()} key bits), longest list "
          f"{int((rg[:, 1] - rg[:, 0]).max()) if n > 1 else 0}")


def test_binning_without_instances_needs_no_buffers_and_clears_the_ranges():
    c = GC.hand_built("lists")
    geom, offsets = _dev(np.zeros_like(c["geom"]), np.float32), _dev(np.zeros(c["P"], dtype=np.int32), np.int32)
    ranges = Guarded((12, 2), torch.int32)
    rc = _lib.load().cut3r_gs_bin(c["P"], _p(geom), _p(offsets), 0, c["W"], c["H"], None, None, None, None, _p(ranges.t), None, 0, None, None)
    torch.cuda.synchronize()
    assert rc == 0 and ranges.intact() and (ranges.np() == 0).all()


def _forward(c, r):
    """cut3r_gs_render_forward on the reference's lists -> dict of numpy outputs (the seven images, aux, n_contrib), margins checked"""
    lib = _lib.load()
    H, W = c["H"], c["W"]
    geom, ranges = _dev(c["geom"], np.float32), _dev(r["ranges"].view(np.int32), np.int32)
    point_list = _dev(r["point_list"].view(np.int32), np.int32)
    out = {k: Guarded((ch, H, W), torch.float32) for k, ch in RO.IMAGES}
    out["aux"], out["n_contrib"] = Guarded((2, H, W), torch.float32), Guarded((2, H, W), torch.int32)
    rc = lib.cut3r_gs_render_forward(_p(ranges), _p(point_list), _p(geom), W, H, c["tanx"], c["tany"], _arr(c["bg"]),
                                     *[_p(out[k].t) for k in ("color", "coord", "mcoord", "depth", "mdepth", "alpha", "normal", "n_contrib", "aux")], None)
    torch.cuda.synchronize()
    assert rc == 0 and all(g.intact() for g in out.values()) and all(g.written() for g in out.values())
    res = {k: g.np() for k, g in out.items()}
    res["n_contrib"] = res["n_contrib"].view(np.uint32)
    return res


def _backward(c, r, products, cot):
    """cut3r_gs_render_backward into a pre-filled dgeom -> [P, 32] numpy, margins checked"""
    lib = _lib.load()
    geom, ranges = _dev(c["geom"], np.float32), _dev(r["ranges"].view(np.int32), np.int32)
    point_list = _dev(r["point_list"].view(np.int32), np.int32)
    p = {k: _dev(v, np.float32) for k, v in products.items() if k != "n_contrib"}
    p["n_contrib"] = _dev(np.ascontiguousarray(products["n_contrib"]).view(np.int32), np.int32)
    g = [_dev(t, np.float32) for t in cot]
    dgeom = Guarded((c["P"], RO.GS_REC), torch.float32)                     # pre-filled: the pass must overwrite, not accumulate
    rc = lib.cut3r_gs_render_backward(_p(ranges), _p(point_list), _p(geom), c["P"], c["W"], c["H"], c["tanx"], c["tany"], _arr(c["bg"]),
                                      _p(p["n_contrib"]), _p(p["aux"]), _p(p["alpha"]), _p(p["coord"]), _p(p["depth"]), _p(p["normal"]),
                                      *[_p(t) for t in g], _p(dgeom.t), None)
    torch.cuda.synchronize()
    assert rc == 0 and dgeom.intact() and dgeom.written()
    return dgeom.np()


_FWD = {}


def _forward_once(name):
    if name not in _FWD:
        c = _case(name)
        _FWD[name] = _forward(c, GC.reference(c))
    return _FWD[name]


@pytest.mark.parametrize("name", CASES)
def test_forward_is_within_its_bound_on_every_unambiguous_pixel(name):
    c = _case(name)
    r = GC.reference(c)
    got = _forward_once(name)
    amb = r["amb"]
    assert amb.mean() <= MAX_AMBIGUOUS and not (amb & c["about"]).any()
    res, n_diff = RO.compare_forward(got, r["fwd"])
    print(f"[gs stage] {name} forward: ambiguous {100 * r['fwd']['ambiguous'].mean():.2f} % of {amb.size} pixels, n_contrib exact on the rest: "
          f"{n_diff == 0}; error / bound " + ", ".join(f"{k} {v[0]:.3f}" for k, v in res.items()))
    assert n_diff == 0
    for k, v in res.items():
        assert v[1] == 0, (k, v)
    again = _forward(c, r)                                                   # a second launch: the same bits
    for k in got:
        assert np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)), k


def _check_backward(name, tag, c, r, dgeom, dbound, got):
    res = RO.compare_backward(got, dgeom, dbound)
    print(f"[gs stage] {name} backward{tag}: error / bound " + ", ".join(f"{k} {v[0]:.3f}" for k, v in res.items() if k != "rest"))
    assert res["rest"] == (0.0, 0)                                           # slots 25..31
    used = RO.ints(c["geom"][:, RO.G_TILES]) > 0
    assert used.sum() < c["P"] and (got[~used] == 0).all()                  # unreferenced rows: exactly 0 (the pre-fill is gone)
    for k, v in res.items():
        assert v[1] == 0, (k, v)


@pytest.mark.parametrize("name", CASES)
def test_backward_is_within_its_bound_for_every_gaussian_and_slot(name):
    """fed the reference's forward products (fp32) and cotangents that are zero on ambiguous pixels"""
    c = _case(name)
    r = GC.reference(c)
    got = _backward(c, r, r["products"], r["cot"])
    assert np.abs(r["dgeom"]).max() > 0
    _check_backward(name, "", c, r, r["dgeom"], r["dbound"], got)


def test_backward_of_the_kernels_own_forward_products_on_a_scene():
    name = "scene900"
    c = _case(name)
    r = GC.reference(c)
    fwd = _forward_once(name)
    products = RO.products_f32(fwd)
    dgeom, dbound = RO.render_backward_reference(*r["args"], products, r["cot"])
    _check_backward(name, " (own forward products)", c, r, dgeom, dbound, _backward(c, r, products, r["cot"]))


@pytest.mark.parametrize("name", tuple(GC.SCENES))
def test_scene_records_lists_and_offsets_are_what_the_records_themselves_imply(name):
    s = _scene(name)
    c, buf = s["case"], s["buf"]
    g, P, W, H = c["geom"], c["P"], c["W"], c["H"]
    assert np.array_equal(buf.geom.cpu().numpy().view(np.uint32), g.view(np.uint32))          # the rasteriser's records are these records
    radii, tiles = s["radii"].cpu().numpy(), s["tiles"].view(np.uint32).astype(np.int64)
    assert np.array_equal(radii, s["radii2"]) and np.array_equal(radii, g[:, RO.G_RADIUS].astype(np.int32))
    vis = radii > 0
    assert 0 < vis.sum() < P and not vis[:4].any() and (g[~vis] == 0).all() and (tiles[~vis] == 0).all()        # culled records are all zero
    rect = RO.tile_rect_reference(g[:, RO.G_XY:RO.G_XY + 2], g[:, RO.G_RADIUS], W, H)
    assert np.array_equal(RO.ints(g[:, RO.G_RECT:RO.G_RECT + 4])[vis], rect[vis])
    area = (rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1])
    assert np.array_equal(RO.ints(g[:, RO.G_TILES])[vis], area[vis]) and np.array_equal(tiles[vis], area[vis]) and (area[vis] > 0).all()
    assert np.array_equal(c["offsets"].astype(np.int64), np.cumsum(tiles))                   # inclusive scan
    pl, rg, overflow = RO.bin_reference(g, c["offsets"], W, H, c["n_inst"])
    assert overflow == 0 and buf.n_inst == c["n_inst"]
    assert np.array_equal(buf.ranges.cpu().numpy().view(np.uint32), rg) and np.array_equal(buf.point_list.cpu().numpy().view(np.uint32)[:c["n_inst"]], pl)
    print(f"[gs stage] {name}: {int(vis.sum())} of {P} records visible, {c['n_inst']} instances, longest list {int((rg[:, 1] - rg[:, 0]).max())}")
