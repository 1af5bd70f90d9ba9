"""cut3r_gs_preprocess and cut3r_gs_preprocess_backward (csrc/gs.hip), each called on its own through the C ABI and compared PER GAUSSIAN
and per field with the fp64 reference of tests/gs_project_oracle.py on the cases of tests/gs_project_cases.py.

The projection takes a dozen hard decisions per Gaussian; the reference knows how far each deciding quantity lies from its threshold,
Gaussians with a decision inside 4 x its fp32 error are `ambiguous` and left out (at most 2 % per case, none of the hand-built ones), and
EVERY field of every other record must lie within K x its own first-order bound -- no percentile, no share beyond a tolerance; radii,
tiles, rectangles, clamp bits and offsets are exact, culled records all-zero.  The backward pass is fed the reference's records rounded to
fp32 and a random dgeom that is zero for ambiguous Gaussians, so it is judged independently of the forward kernel.  Every output lies
inside a larger sentinel-filled allocation whose margins must stay intact.

Contract stated here: cut3r_gs_preprocess_backward writes the gradient rows of VISIBLE Gaussians only (and of d_shs only the
(deg + 1)^2 active coefficients); rows of culled Gaussians and inactive coefficients keep what the caller put there -- the caller zeroes them.

Measured on an MI355X, largest error / (K x bound) over the five cases (each test prints its own figures as `[gs project] ...`):
  forward   xy 0.324 (hand257), depth 0.413, vp 0.413, conic 0.338 (hand257), ts 0.458, op 0.048 (sh65), rgb 0.457 (one), cp 0.340 (scene300),
            rp 0.102, nrm 0.088 (hand257); no Gaussian of any case was ambiguous
  backward  d_means 0.146 (scene300), d_scales 0.055, d_rots 0.037 (one), d_opacities 0.060 (sh65), d_shs 0.436 (scene300)"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pytestmark = pytest.mark.gpu

from cut3r_slam_amd import _lib  # noqa: E402
from cut3r_slam_amd import gaussian_rasterizer as GR  # noqa: E402
from tests import gs_project_cases as PC  # noqa: E402
from tests import gs_project_oracle as PO  # noqa: E402
from tests.test_gs_render_gpu import DEV, Guarded, _arr, _dev, _p  # noqa: E402

CASES = tuple(PC.CASES)
MAX_AMBIGUOUS = 0.02
F32 = np.float32


def _inputs(c):
    t = dict(means=_dev(c["means"], F32), scales=_dev(c["scales"], F32), rots=_dev(c["rots"], F32), opac=_dev(c["opac"].reshape(-1), F32))
    t["shs"] = _dev(c["shs"], F32) if c["shs"] is not None else None
    t["colors"] = _dev(c["colors"], F32) if c["colors"] is not None else None
    return t


def _preprocess_args(c, t, out, scan, **change):
    """the argument list of cut3r_gs_preprocess for a case; `change` replaces arguments by name"""
    a = dict(P=c["P"], means=_p(t["means"]), scales=_p(t["scales"]), rots=_p(t["rots"]), opac=_p(t["opac"]), shs=_p(t["shs"]), deg=c["deg"], K=c["K"],
             colors=_p(t["colors"]), view=_arr(c["view"]), proj=_arr(c["proj"]), campos=_arr(c["campos"]), W=c["W"], H=c["H"], tanx=c["tanx"],
             tany=c["tany"], ks=c["ks"], mod=c["mod"], geom=_p(out["geom"].t), radii=_p(out["radii"].t), tiles=_p(out["tiles"].t),
             offsets=_p(out["offsets"].t), ws=_p(scan), ws_bytes=scan.numel(), stream=None)
    a.update(change)
    return list(a.values())


def _forward_outputs(P):
    out = {"geom": Guarded((P, 32), torch.float32)}
    out.update({k: Guarded((P,), torch.int32) for k in ("radii", "tiles", "offsets")})
    return out


_FWD = {}


def _forward(name):
    """cut3r_gs_preprocess on a case, once -> numpy outputs, margins and full writes checked"""
    if name not in _FWD:
        c = PC.case(name)
        t, out = _inputs(c), _forward_outputs(c["P"])
        ws = torch.empty(GR.workspace_bytes(c["P"], 0), dtype=torch.uint8, device=DEV)
        rc = _lib.load().cut3r_gs_preprocess(*_preprocess_args(c, t, out, ws))
        torch.cuda.synchronize()
        assert rc == 0 and all(g.intact() and g.written() for g in out.values())
        _FWD[name] = dict(geom=out["geom"].np(), radii=out["radii"].np(), tiles=out["tiles"].np().view(np.uint32),
                          offsets=out["offsets"].np().view(np.uint32))
    return _FWD[name]


@pytest.mark.parametrize("name", CASES)
def test_every_record_field_is_within_its_bound_and_the_integers_are_exact(name):
    c, r = PC.case(name), PC.reference(name)
    ref = r["fwd"]
    assert ref["ambiguous"].mean() <= MAX_AMBIGUOUS and not (ref["ambiguous"] & c["about"]).any()
    got = _forward(name)
    res, bad = PO.compare_forward(got, ref)
    print(f"[gs project] {name} forward: {int(ref['visible'].sum())} of {c['P']} visible, {int(ref['ambiguous'].sum())} ambiguous, exact quantities "
          f"that differ {bad}; error / bound " + ", ".join(f"{k} {v[0]:.3f}" for k, v in res.items()))
    assert bad == 0
    for k, v in res.items():
        assert v[1] == 0, (k, v, _worst(got["geom"], ref, k, c))
    culled = ~ref["ambiguous"] & ~ref["visible"]
    assert (got["geom"][culled].view(np.uint32) == 0).all() and (got["radii"][culled] == 0).all() and (got["tiles"][culled] == 0).all()
    assert np.array_equal(got["offsets"].astype(np.int64), np.cumsum(got["tiles"].astype(np.int64)))


def _worst(geom, ref, group, c):
    """the Gaussian that shows a ratio above 1, for the report"""
    s = list(dict(PO.FIELDS)[group])
    err = np.abs(geom[:, s].astype(np.float64) - ref["geom"][:, s]) / np.maximum(PO.K[group] * ref["bound"][:, s], 1e-300)
    err[ref["ambiguous"]] = 0
    i = int(np.argmax(err.max(axis=1)))
    inv = {v: k for k, v in c["labels"].items()}
    return dict(gaussian=i, label=inv.get(i), got=geom[i, s].tolist(), ref=ref["geom"][i, s].tolist(), bound=ref["bound"][i, s].tolist())


def _backward_outputs(c):
    P = c["P"]
    out = {"d_means": Guarded((P, 3), torch.float32), "d_scales": Guarded((P, 3), torch.float32), "d_rots": Guarded((P, 4), torch.float32),
           "d_opacities": Guarded((P,), torch.float32), "d_means2D": Guarded((P, 3), torch.float32)}
    if c["shs"] is not None:
        out["d_shs"] = Guarded((P, c["K"], 3), torch.float32)
    else:
        out["d_colors"] = Guarded((P, 3), torch.float32)
    return out


def _backward_args(c, t, records, grads, out, **change):
    a = dict(P=c["P"], means=_p(t["means"]), scales=_p(t["scales"]), rots=_p(t["rots"]), opac=_p(t["opac"]), shs=_p(t["shs"]), deg=c["deg"], K=c["K"],
             view=_arr(c["view"]), proj=_arr(c["proj"]), campos=_arr(c["campos"]), W=c["W"], H=c["H"], tanx=c["tanx"], tany=c["tany"], ks=c["ks"],
             mod=c["mod"], geom=_p(records), dgeom=_p(grads), d_means=_p(out["d_means"].t), d_scales=_p(out["d_scales"].t), d_rots=_p(out["d_rots"].t),
             d_opac=_p(out["d_opacities"].t), d_shs=_p(out["d_shs"].t) if "d_shs" in out else None,
             d_colors=_p(out["d_colors"].t) if "d_colors" in out else None, d_means2D=_p(out["d_means2D"].t), stream=None)
    a.update(change)
    return list(a.values())


@pytest.mark.parametrize("name", CASES)
def test_every_gradient_is_within_its_bound_for_every_gaussian_and_component(name):
    """fed the reference's records (fp32) and a dgeom that is zero for ambiguous Gaussians; the outputs are pre-filled with a sentinel"""
    c, r = PC.case(name), PC.reference(name)
    ref = r["bwd"]
    t, out = _inputs(c), _backward_outputs(c)
    geom, dgeom = _dev(r["geom"], F32), _dev(r["dgeom"], F32)
    rc = _lib.load().cut3r_gs_preprocess_backward(*_backward_args(c, t, geom, dgeom, out))
    torch.cuda.synchronize()
    assert rc == 0 and all(g.intact() for g in out.values())
    got = {k: g.np() for k, g in out.items()}
    vis = ref["visible"]
    assert np.array_equal(vis, r["fwd"]["visible"]) and 0 < vis.sum()
    for k, g in out.items():                                                # culled rows keep the sentinel (the caller zeroes them) ...
        assert (got[k][~vis] == F32(g.fill)).all(), k
        if k != "d_shs":                                                    # ... visible rows are fully written
            assert (got[k][vis] != F32(g.fill)).all(), k
    if "d_shs" in out:                                                      # of d_shs the active coefficients, the others are the caller's
        nb = (c["deg"] + 1) ** 2
        assert (got["d_shs"][vis][:, :nb] != F32(out["d_shs"].fill)).all() and (got["d_shs"][vis][:, nb:] == F32(out["d_shs"].fill)).all()
    res, bad = PO.compare_backward(got, ref)
    print(f"[gs project] {name} backward: exact quantities that differ {bad}; error / bound " + ", ".join(f"{k} {v[0]:.3f}" for k, v in res.items()))
    assert bad == 0
    for k, v in res.items():
        assert v[1] == 0, (k, v)
    assert all(np.abs(ref[k]).max() > 0 for k in res)


def test_pose_mode_and_gradient_mode_give_the_same_per_gaussian_bits():
    """cut3r_gs_pose_backward launches the same kernel; with ONE Gaussian, an identity pose and the unit quaternion (1, 0, 0, 0) in theta
    its sums 9..11 are that Gaussian's d_mean and its sums 12..15 its d_rot (x, y, z, r), each summed with exact zeros only"""
    lib, name = _lib.load(), "hand65"
    c, r = PC.case(name), PC.reference(name)
    t, out = _inputs(c), _backward_outputs(c)
    geom, dgeom = _dev(r["geom"], F32), _dev(r["dgeom"], F32)
    assert lib.cut3r_gs_preprocess_backward(*_backward_args(c, t, geom, dgeom, out)) == 0
    d_means, d_rots = out["d_means"].np(), out["d_rots"].np()
    picked = [c["labels"][k] for k in ("x1.4", "thin5e-5", "pair12", "q0.7", "whole_grid", "corner0", "z0.21")] + [0, 1]
    theta = torch.zeros(1, 14, device=DEV)
    theta[0, 10] = 1.0
    ps = torch.zeros(32, device=DEV)
    ps[6] = 1.0
    for i in picked:
        assert r["bwd"]["visible"][i]
        one = lambda a: a[i:i + 1].contiguous()
        partials, sums = Guarded((1, 16), torch.float32), Guarded((16,), torch.float32)
        rc = lib.cut3r_gs_pose_backward(1, _p(one(t["means"])), _p(one(t["scales"])), _p(one(t["rots"])), _p(one(t["opac"])), _arr(c["view"]),
                                        _arr(c["proj"]), c["W"], c["H"], c["tanx"], c["tany"], c["ks"], c["mod"], _p(one(geom)), _p(one(dgeom)),
                                        _p(theta), _p(ps), _p(partials.t), _p(sums.t), None)
        torch.cuda.synchronize()
        assert rc == 0 and partials.intact() and sums.intact() and sums.written()
        s = sums.np()
        assert np.array_equal(s[9:12], d_means[i]) and np.array_equal(s[[15, 12, 13, 14]], d_rots[i]), (i, s[9:16], d_means[i], d_rots[i])


def _untouched(out):
    return all(g.intact() and bool((g.t == g.fill).all()) for g in out.values())


def test_refused_preprocess_calls_write_nothing():
    lib = _lib.load()
    c = PC.case("sh65")
    t, out = _inputs(c), _forward_outputs(c["P"])
    ws = torch.empty(GR.workspace_bytes(c["P"], 0), dtype=torch.uint8, device=DEV)
    bad = [dict(P=0), dict(P=-3), dict(deg=-1), dict(deg=4), dict(deg=2, K=8), dict(W=0), dict(H=-1), dict(tanx=0.0), dict(tany=-0.5),
           dict(shs=None, colors=None), dict(ws=None), dict(ws_bytes=0)]
    bad += [{k: None} for k in ("means", "scales", "rots", "opac", "view", "proj", "geom", "radii", "tiles", "offsets")]
    for change in bad:
        assert lib.cut3r_gs_preprocess(*_preprocess_args(c, t, out, ws, **change)) == 1, change
        torch.cuda.synchronize()
        assert _untouched(out), change
    assert lib.cut3r_gs_preprocess(*_preprocess_args(c, t, out, ws, campos=None)) == 0          # (optional: the origin)
    torch.cuda.synchronize()
    assert all(g.intact() and g.written() for g in out.values())


def test_refused_preprocess_backward_calls_write_nothing():
    lib = _lib.load()
    c, r = PC.case("sh65"), PC.reference("sh65")
    t, out = _inputs(c), _backward_outputs(c)
    geom, dgeom = _dev(r["geom"], F32), _dev(r["dgeom"], F32)
    bad = [dict(P=0), dict(P=-3), dict(deg=-1), dict(deg=4), dict(deg=2, K=8), dict(W=0), dict(H=-1), dict(tanx=0.0), dict(tany=-0.5), dict(d_shs=None)]
    bad += [{k: None} for k in ("means", "scales", "rots", "opac", "view", "proj", "geom", "dgeom", "d_means", "d_scales", "d_rots", "d_opac",
                                "d_means2D")]
    bad += [dict(shs=None)]                                                 # the colour mode without d_colors
    for change in bad:
        assert lib.cut3r_gs_preprocess_backward(*_backward_args(c, t, geom, dgeom, out, **change)) == 1, change
        torch.cuda.synchronize()
        assert _untouched(out), change


def test_refused_binning_leaves_the_ranges_alone():
    """with instances to sort, a missing key / value / workspace buffer is refused before `ranges` is cleared"""
    lib = _lib.load()
    c = PC.case("hand65")
    f = _forward("hand65")
    n = int(f["offsets"][-1])
    assert n > 0
    geom, offsets = _dev(f["geom"], F32), _dev(f["offsets"].view(np.int32), np.int32)
    tiles = ((c["W"] + 15) // 16) * ((c["H"] + 15) // 16)
    bufs = dict(keys_tmp=Guarded((n,), torch.int64), vals_tmp=Guarded((n,), torch.int32), keys_sorted=Guarded((n,), torch.int64),
                point_list=Guarded((n,), torch.int32), ranges=Guarded((tiles, 2), torch.int32))
    ws = torch.empty(GR.workspace_bytes(c["P"], n), dtype=torch.uint8, device=DEV)
    for missing in ("keys_tmp", "vals_tmp", "keys_sorted", "point_list", "ws", "ws_bytes", "ranges", "geom", "offsets"):
        a = dict(P=c["P"], geom=_p(geom), offsets=_p(offsets), n=n, W=c["W"], H=c["H"], keys_tmp=_p(bufs["keys_tmp"].t), vals_tmp=_p(bufs["vals_tmp"].t),
                 keys_sorted=_p(bufs["keys_sorted"].t), point_list=_p(bufs["point_list"].t), ranges=_p(bufs["ranges"].t), ws=_p(ws), ws_bytes=ws.numel(),
                 overflow=None, stream=None)
        a[missing] = 0 if missing == "ws_bytes" else None
        assert lib.cut3r_gs_bin(*a.values()) == 1, missing
        torch.cuda.synchronize()
        assert _untouched(bufs), missing
