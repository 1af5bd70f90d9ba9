"""CPU: the reference-alone checks behind tests/gs_project_oracle.py, on the cases of tests/gs_project_cases.py.

  * the fp64 reference (constants taken as doubles) equals oracle/gs_oracle.py::preprocess, an independent restatement, and its torch
    autograd for the derivative, at the fp64 level: found 3.9e-12 of the scale for values and 1.6e-11 for gradients (the 1e11-sized planes
    of the two `vbn` Gaussians; 6e-15 and 1.2e-14 without them), asserted at 2e-11 and 1e-10;
  * the fp32 restatement stays inside RATIO x the model bound, i.e. under half of what the GPU test allows with K = max(1, 2 RATIO): the
    table in the oracle's docstring comes from here;
  * every case leaves at least 98 % of its Gaussians unambiguous, none of the hand-built ones is ambiguous and each of them is on the
    side of its branch it was built for;
  * eleven mutants of the restatement are each REJECTED by the comparison the GPU test makes, on a named case."""
import numpy as np
import pytest
import torch

from oracle import gs_oracle as GO
from tests import gs_project_cases as PC
from tests import gs_project_oracle as PO
from tests.gs_render_oracle import F32, F64, G_DEPTH, G_OP, G_RADIUS, G_RGB

CASES = tuple(PC.CASES)
MAX_AMBIGUOUS = 0.02


def _settings(c):
    t = lambda a, n: torch.from_numpy(np.asarray(a, dtype=F64).reshape(n, n) if n > 1 else np.asarray(a, dtype=F64))
    return {"image_height": c["H"], "image_width": c["W"], "tanfovx": c["tanx"], "tanfovy": c["tany"], "kernel_size": float(F32(c["ks"])),
            "scale_modifier": float(F32(c["mod"])), "viewmatrix": t(c["view"], 4), "projmatrix": t(c["proj"], 4), "sh_degree": c["deg"],
            "campos": t(c["campos"], 1)}


@pytest.mark.parametrize("name", CASES)
def test_reference_is_the_independent_fp64_restatement_and_its_autograd(name):
    c, r = PC.case(name), PC.reference(name)
    fwd = PO.forward_reference(c, exact_constants=True)
    leaf = lambda a: torch.from_numpy(np.asarray(a, dtype=F64)).requires_grad_(True)
    means, scales, rots, opac = leaf(c["means"]), leaf(c["scales"]), leaf(c["rots"]), leaf(c["opac"])
    shs = leaf(c["shs"]) if c["shs"] is not None else None
    colors = torch.from_numpy(c["colors"].astype(F64)) if c["colors"] is not None else None
    g = GO.preprocess(means, opac, scales, rots, shs, colors, _settings(c))
    keep = ~r["fwd"]["ambiguous"]
    vis = fwd["visible"]
    assert np.array_equal(g["visible"].numpy()[keep], vis[keep]) and np.array_equal(g["radii"].numpy()[keep], fwd["radii"][keep])
    assert np.array_equal(g["rect"].numpy()[keep & vis], fwd["rect"][keep & vis])
    cols = torch.cat([g["xy"], g["depth"][:, None], g["ts"][:, None], g["conic"], g["opacity"][:, None], g["colour"], g["view_point"],
                      g["camera_plane"], g["ray_plane"], g["normal"]], 1)
    ok = keep & vis
    scale = np.maximum(1.0, np.abs(fwd["geom"][:, :25]))
    worst = float((np.abs(cols.detach().numpy() - fwd["geom"][:, :25]) / scale)[ok].max()) if ok.any() else 0.0
    # the derivative: the same contraction with dgeom, on the Gaussians without the (NaN-producing, in autograd) mlen exit
    fine = ok & ~fwd["side"]["bad"]
    dg = r["dgeom"].astype(F64)
    dg_rgb0 = dg.copy()
    dg_rgb0[:, G_DEPTH] = 0                                                  # (the |d/dxy| statistic of the render pass: handed on, no gradient)
    if c["shs"] is None:
        dg_rgb0[:, G_RGB:G_RGB + 3] = 0
    loss = (cols * torch.from_numpy(np.where(fine[:, None], dg_rgb0[:, :25], 0.0))).sum()
    leaves = [means, scales, rots, opac] + ([shs] if shs is not None else [])
    grads = [t.numpy() for t in torch.autograd.grad(loss, leaves, allow_unused=True)]
    geom = PO.records_f32(fwd)
    bwd = PO.backward_reference(c, geom, r["dgeom"], exact_constants=True)
    ours = [bwd["d_means"], bwd["d_scales"], bwd["d_rots"], bwd["d_opacities"].reshape(-1, 1)] + ([bwd["d_shs"]] if shs is not None else [])
    gworst = 0.0
    for a, b in zip(grads, ours):
        m = fine.reshape((-1,) + (1,) * (a.ndim - 1))
        sc = np.maximum(1.0, np.abs(a).max(axis=tuple(range(1, a.ndim)), keepdims=True))
        gworst = max(gworst, float(np.where(m, np.abs(a - b) / sc, 0.0).max()))
    print(f"[gs project cpu] {name}: reference against oracle/gs_oracle.py: values {worst:.2e}, autograd {gworst:.2e} of the scale "
          f"({int(ok.sum())} visible, {int(fine.sum())} differentiated)")
    assert worst <= 2e-11 and gworst <= 1e-10


@pytest.mark.parametrize("name", CASES)
def test_reference_alone_leaves_the_case_unambiguous_and_the_hand_built_on_their_side(name):
    c, r = PC.case(name), PC.reference(name)
    f = r["fwd"]
    amb, side = f["ambiguous"], f["side"]
    print(f"[gs project cpu] {name}: ambiguous {int(amb.sum())} of {c['P']} ({', '.join(k for k, v in f['why'].items() if v.any()) or 'none'}), "
          f"visible {int(f['visible'].sum())}, hand-built {int(c['about'].sum())}")
    assert amb.mean() <= MAX_AMBIGUOUS and not (amb & c["about"]).any()
    assert np.isfinite(f["geom"]).all() and np.isfinite(f["bound"]).all()
    assert all(np.isfinite(r["bwd"][k]).all() for k in PO.GRADS if k in r["bwd"])
    gx, gy = (c["W"] + 15) // 16, (c["H"] + 15) // 16
    for label, i in c["labels"].items():
        for key, want in c["expect"][label].items():
            if key == "visible":
                assert bool(f["visible"][i]) == want, (label, key)
            elif key == "rect0":
                assert tuple(f["rect"][i, :2]) == want, (label, key)
            elif key == "full":
                assert tuple(f["rect"][i]) == (0, 0, gx, gy), (label, key)
            elif key == "clampbits":
                assert int(f["clampbits"][i]) == want and f["geom"][i, G_RGB + 1] == 0 and (f["geom"][i, [G_RGB, G_RGB + 2]] > 0).all(), (label, key)
            elif key == "edge":
                continue
            else:
                assert side[key][i] == want, (label, key, side[key][i])
    lab = c["labels"]
    if "all0" in lab and c["ks"] > 0:                                        # kept with coef = 0: opacity 0, and no derivative through coef
        assert f["geom"][lab["all0"], G_OP] == 0 and f["bound"][lab["all0"], G_OP] == 0
    if "x1.4" in lab:                                                        # the clamped terms carry no derivative: see the mutant below
        assert side["clamped"][lab["x1.4"]] and not side["clamped"][lab["x1.2"]]
    if "mlen0" in lab:
        assert (f["geom"][lab["mlen0"], 14:25] == 0).all() and (f["bound"][lab["mlen0"], 14:25] == 0).all()
    if "edge_in" in lab:
        assert f["tiles"][lab["edge_in"]] >= 1 and f["tiles"][lab["edge_out"]] == 0 and f["radii"][lab["edge_out"]] == 0


_MEASURED = {}


def _measure(name):
    """error / model bound (K = 1 units) of the fp32 restatement per group, and the exact quantities that differ"""
    if name not in _MEASURED:
        c, r = PC.case(name), PC.reference(name)
        res, bad = PO.compare_forward(PO.forward_f32(c), r["fwd"])
        back, bad2 = PO.compare_backward(PO.backward_f32(c, r["geom"], r["dgeom"]), r["bwd"])
        res.update(back)
        _MEASURED[name] = ({k: v[0] * PO.K[k] for k, v in res.items()}, bad + bad2)
    return _MEASURED[name]


@pytest.mark.parametrize("name", CASES)
def test_fp32_restatement_stays_under_the_measured_ratios(name):
    units, bad = _measure(name)
    print(f"[gs project cpu] {name}: error / model bound " + ", ".join(f"{k} {v:.3f}" for k, v in units.items()))
    assert bad == 0
    for k, v in units.items():
        assert v <= PO.RATIO[k], (k, v)
        assert v / PO.K[k] <= 0.5, (k, v)                                     # half of what the GPU test allows


def test_ratio_table_is_the_measured_worst_plus_a_twentieth_rounded_up():
    wrong = []
    for k, ratio in PO.RATIO.items():
        worst, where = max((_measure(n)[0][k], n) for n in CASES if k in _measure(n)[0])
        rule = np.ceil((worst + 0.05) * 10 - 1e-9) / 10
        print(f"[gs project cpu] RATIO {k:12s} measured {worst:.3f} ({where}) -> {rule:.1f}, K {max(1.0, 2 * rule):.1f}")
        if abs(ratio - rule) > 1e-9 or PO.K[k] != max(1.0, 2.0 * ratio):
            wrong.append(k)
    assert not wrong, wrong


MUTANTS = (("near_ge", "sh65", "forward"), ("clamp_1", "hand65", "forward"), ("clamp_value_only", "hand65", "backward"),
           ("kmin_largest", "hand65", "forward"), ("keep_g", "hand257", "forward"), ("coef_not_zeroed", "hand257", "forward"),
           ("no_radius_floor", "hand65", "forward"), ("sh_stride", "sh65", "forward"), ("clampbit_ignored", "sh65", "backward"),
           ("mod_once", "hand257", "forward"), ("means2d_W", "hand65", "backward"))


@pytest.mark.parametrize("mutant,name,stage", MUTANTS)
def test_mutant_is_rejected(mutant, name, stage):
    c, r = PC.case(name), PC.reference(name)
    if stage == "forward":
        res = PO.compare_forward(PO.forward_f32(c, mutants=(mutant,)), r["fwd"])
    else:
        res = PO.compare_backward(PO.backward_f32(c, r["geom"], r["dgeom"], mutants=(mutant,)), r["bwd"])
    worst = max(v[0] for v in res[0].values())
    print(f"[gs project cpu] mutant {mutant} on {name} ({stage}): worst error / bound {worst:.3g}, exact quantities that differ {res[1]}")
    assert PO.rejected(res)
    assert mutant in PO.MUTANTS


def test_decisions_on_a_threshold_are_flagged_and_exact_ones_are_not():
    c = PC.case("sh65")
    f = PC.reference("sh65")["fwd"]
    i = c["labels"]["z=0.2f"]
    assert c["means"][i, 2] == F32(0.2) and not f["ambiguous"][i] and not f["visible"][i]        # exact: decided, and culled by `>`
    moved = dict(c, means=c["means"].copy(), name="moved")
    moved["means"][i, 0] = 0.013                                            # no longer on the axis: nothing changes for z
    assert not PO.forward_reference(moved)["ambiguous"][i]
    h = PC.case("hand65")
    j = h["labels"]["z0.21"]
    for dz, want in ((0.0, False), (-0.00999998, True)):                    # through the rotated view z carries roundings: 0.2 + 2e-8 is open
        m = dict(h, means=h["means"].copy(), name="moved")
        w2c = PC.camera_of("hand65")["w2c"]
        m["means"][j] = (np.linalg.inv(w2c) @ np.array([0.01, 0.01, 0.21 + dz, 1.0]))[:3].astype(F32)
        assert bool(PO.forward_reference(m)["why"]["z"][j]) == want
    assert G_RADIUS == 25
