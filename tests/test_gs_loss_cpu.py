"""CPU: the reference-alone checks behind tests/gs_loss_oracle.py.

  * the references equal plain fp64 formulations written another way, at the fp64 level: gs_mapper.ssim_torch and torch autograd for
    the SSIM maps and gradient (with the window ssim_torch itself builds for fp64 inputs -- it takes no window -- handed to the oracle),
    the tensor formulations of tests/test_gs_gpu.py for the pixel and refine losses, an exhaustive fp64 search for the 3-NN.
    Tolerance: FP64_LEVEL x the element's own fp32 bound -- the two unit roundoffs are 2^-29 apart, and the other formulation has at
    most 121 summands (an 11 x 11 convolution) where the oracle has 22, far fewer than the 64 allowed -- plus 1e-14 of the value for the
    handful of roundings of the value itself.
  * the fp32 restatements stay inside RATIO x the model bound (the table of the oracle's docstring is printed here), and no case leaves
    more than 1 % of its elements ambiguous;
  * the kernel's window table is the normalised Gaussian;
  * mutants of the restatements are each REJECTED by the comparison the GPU test makes."""
import numpy as np
import pytest
import torch

from tests import gs_loss_oracle as LO
from tests.gs_render_oracle import F32, F64, ratio

_WORST = {}
FP64_LEVEL = 64.0 * 2.0 ** -29


def _note(group, name, got, ref, keep=None):
    r, _ = ratio(got, ref.v, ref.e, keep)
    if r > _WORST.get(group, (0.0, ""))[0]:
        _WORST[group] = (r, name)
    return r


def _same64(got, ref, what):
    """an independent fp64 formulation against the reference, at the fp64 level"""
    got = np.asarray(got, dtype=F64).reshape(ref.v.shape)
    tol = FP64_LEVEL * np.broadcast_to(ref.e, ref.v.shape) + 1e-14 * np.abs(ref.v)
    bad = np.abs(got - ref.v) > tol
    assert not bad.any(), (what, int(bad.sum()), float(np.abs(got - ref.v).max()))


# ------------------------------------------------------------------------------------------------------------------ SSIM
def test_kernel_window_is_the_normalised_gaussian():
    x = np.arange(11, dtype=F64) - 5
    g = np.exp(-x * x / (2 * 1.5 * 1.5))
    g /= g.sum()
    err, total = np.abs(LO.SS_G.astype(F64) - g).max(), LO.SS_G.astype(F64).sum()
    print(f"[gs loss cpu] SS_G: max |entry - Gaussian| {err:.3g}, sum 1 - {1 - total:.3g}")
    assert err < 1e-8 and abs(total - 1) < 4e-8
    assert np.array_equal(LO.SS_G, LO.SS_G[::-1])                            # symmetric: the backward pass filters with the same table


def _torch_window():
    """the window gs_mapper.ssim_torch builds for fp64 inputs"""
    g = torch.exp(-((torch.arange(11).to(torch.float64) - 5) ** 2) / (2 * 1.5 * 1.5))
    return g / g.sum()


def _ssim_maps_torch(a, b):
    """ssim_torch's own expressions per pixel (fp64), and the three partial maps by autograd of the per-pixel S"""
    g = _torch_window()[:, None]
    C = a.shape[0]
    w = (g @ g.T)[None, None].expand(C, 1, 11, 11).contiguous()
    f = lambda t: torch.nn.functional.conv2d(t[None], w, padding=5, groups=C)[0]
    mu1, x11, x12 = (f(t).detach().requires_grad_(True) for t in (a, a * a, a * b))
    mu2, x22 = f(b), f(b * b)
    s11, s22, s12 = x11 - mu1 * mu1, x22 - mu2 * mu2, x12 - mu1 * mu2
    c1, c2 = float(F32(0.0001)), float(F32(0.0009))
    S = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s11 + s22 + c2))
    return [S.detach().numpy()] + [t.numpy() for t in torch.autograd.grad(S.sum(), [mu1, x11, x12])]


@pytest.mark.parametrize("C,H,W", ((1, 1, 1), (1, 5, 5), (2, 11, 11), (1, 17, 33), (3, 37, 50)))
def test_ssim_reference_is_ssim_torch_and_its_autograd(C, H, W):
    from cut3r_slam_amd.gs_mapper import ssim_torch
    win = _torch_window().numpy()
    for content in ("random", "flat_bright", "exposure"):
        a, b = LO.ssim_case(content, C, H, W)
        ref = LO.ssim_forward(a, b, C, H, W, window=win)
        ta, tb = torch.tensor(a.astype(F64), requires_grad=True), torch.tensor(b.astype(F64))
        # (ssim_torch squares 0.01 and 0.03 in fp64; the kernel's constants are the fp32 numbers: a relative 3e-8 of C1, C2)
        value = ssim_torch(ta, tb)
        maps = _ssim_maps_torch(ta.detach(), tb)
        assert abs(float(value.detach()) - maps[0].mean()) < 1e-7
        for got, r, name in zip(maps, ref, ("smap", "d_mu1", "d_x11", "d_x12")):
            _same64(got, r, (C, H, W, content, name))
        # the gradient of the mean: the backward pass on the reference's own fp64 maps, against autograd through the whole expression
        S = _ssim_mean_torch(ta, tb)
        grad = torch.autograd.grad(S, ta)[0].numpy()
        back = LO.ssim_backward(a, b, ref[1].v, ref[2].v, ref[3].v, np.array([1.0 / (C * H * W)]), C, H, W, window=win)
        # the maps handed in are exact inputs there: their own fp32 bounds, pushed through the filter, are what the comparison may use
        tol = LO.ssim_backward(np.abs(a), np.abs(b), ref[1].e, ref[2].e, ref[3].e, np.array([1.0 / (C * H * W)]), C, H, W, window=win).v
        assert (np.abs(grad - back.v) <= FP64_LEVEL * (back.e + tol) + 1e-14 * np.abs(back.v)).all(), (C, H, W, content)


def _ssim_mean_torch(a, b):
    g = _torch_window()[:, None]
    C = a.shape[0]
    w = (g @ g.T)[None, None].expand(C, 1, 11, 11).contiguous()
    f = lambda t: torch.nn.functional.conv2d(t[None], w, padding=5, groups=C)[0]
    mu1, mu2 = f(a), f(b)
    s11, s22, s12 = f(a * a) - mu1 * mu1, f(b * b) - mu2 * mu2, f(a * b) - mu1 * mu2
    c1, c2 = float(F32(0.0001)), float(F32(0.0009))
    return (((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s11 + s22 + c2))).mean()


_SSIM_GROUPS = ("ssim_map", "d_mu1", "d_x11", "d_x12")


def test_ssim_restatement_within_the_model_bound():
    for name, C, H, W, a, b in LO.ssim_cases():
        ref, f32 = LO.ssim_forward(a, b, C, H, W), LO.ssim_forward(a, b, C, H, W, f32=True)
        r = [_note(g, name, x.v, y) for g, x, y in zip(_SSIM_GROUPS, f32, ref)]
        if name.endswith("black"):                                           # every pass runs over zeros: exact
            assert (f32[0].v == 1).all() and (f32[1].v == 0).all() and (ref[1].v == 0).all() and (ref[1].e == 0).all()
            assert (np.abs(ref[0].v - 1) <= ref[0].e).all()
        gs = LO.ssim_cotangent(C, H, W)
        maps = [m.v for m in f32[1:]]                                        # the backward pass is judged on stored fp32 maps
        back, back32 = LO.ssim_backward(a, b, *maps, gs, C, H, W), LO.ssim_backward(a, b, *maps, gs, C, H, W, f32=True)
        r.append(_note("ssim_grad", name, back32.v, back))
        assert np.isfinite(ref[0].v).all() and np.isfinite(back.v).all()
        assert all(x <= LO.RATIO[g] for x, g in zip(r, _SSIM_GROUPS + ("ssim_grad",))), (name, r)
    print("[gs loss cpu] ssim: restatement error / model bound " + ", ".join(f"{g} {_WORST[g][0]:.3f}" for g in _SSIM_GROUPS + ("ssim_grad",)))


# ------------------------------------------------------------------------------------------------------------------ pixel loss
def _pixel_tensor64(c, H, W, coef):
    """the tensor formulation of tests/test_gs_gpu.py (colour L1, masked inverse-depth L1, masked depth-normal term) in fp64 with the
    kernel's floor: sums [4] and the autograd gradient w.r.t. the rendered depth"""
    fx, fy, cx, cy = (float(F32(v)) for v in c["cam"])
    th = float(LO.TH_D)
    t = lambda a: torch.tensor(np.asarray(a, dtype=F32).astype(F64))
    d, gd, gn, img, gt = t(c["depth"]).requires_grad_(True), t(c["gt_depth"]), t(c["gn"]), t(c["img"]), t(c["gt"])
    mask = (gd > th) & (d > th)
    one = torch.ones_like(d)
    inv = torch.abs(1 / torch.where(mask, d, one) - 1 / torch.where(mask, gd, one)) * mask
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    pts = torch.stack([(xs - cx) / fx * d, (ys - cy) / fy * d, d], 0)
    dx, dy = pts[:, 1:-1, 2:] - pts[:, 1:-1, :-2], pts[:, 2:, 1:-1] - pts[:, :-2, 1:-1]
    cr = torch.cross(dx, dy, dim=0)
    ln = cr.norm(dim=0, keepdim=True)
    big = ln > LO.FLOOR                                                      # below the floor: c / 1e-12, and no gradient
    n = torch.nn.functional.pad(torch.where(big, cr / torch.where(big, ln, torch.ones_like(ln)), (cr / LO.FLOOR).detach()), (1, 1, 1, 1))
    nrm = (1 - (n * gn).sum(0)) * mask
    sums = [torch.abs(gt - img).sum(), inv.sum(), nrm.sum(), mask.sum()]
    c_dep, c_nrm = float(F32(coef[1])), float(F32(coef[2]))
    g = torch.autograd.grad(c_dep * sums[1] + c_nrm * sums[2], d, allow_unused=True)[0]
    return np.array([float(s.detach()) for s in sums]), (g.numpy() if g is not None else np.zeros((H, W)))


def _pixel_args(c, H, W):
    return c["img"], c["gt"], c["depth"], c["gt_depth"], c["gn"], H, W, c["cam"]


def test_pixel_loss_reference_and_restatement():
    for name, H, W, c in LO.pixel_cases():
        args = _pixel_args(c, H, W)
        s, s32 = LO.pixel_loss_forward(*args), LO.pixel_loss_forward(*args, f32=True)
        gi, gd, amb = LO.pixel_loss_backward(*args, LO.PIXEL_COEF)
        gi32, gd32, _ = LO.pixel_loss_backward(*args, LO.PIXEL_COEF, f32=True)
        assert amb.mean() <= LO.MAX_AMBIGUOUS, (name, int(amb.sum()))
        sums64, g64 = _pixel_tensor64(c, H, W, LO.PIXEL_COEF)
        _same64(sums64, s, (name, "sums"))
        _same64(g64, gd, (name, "g_d"))
        mask = LO._valid(c["depth"], c["gt_depth"])
        assert s.v[3] == s32.v[3] == mask.sum() and s.e[3] == 0 and np.array_equal(gi, gi32)
        assert (gi[:, 0, 0] == 0).all() and set(np.unique(np.abs(gi))) <= {F32(0), F32(LO.PIXEL_COEF[0])}
        same = mask & (c["depth"] == c["gt_depth"])                          # d == gt_d: the inverse-depth term has gradient exactly 0
        if name.endswith("mixed"):
            assert same.any() and not amb[same].any()
            g0 = LO.pixel_loss_backward(*args, LO.PIXEL_COEF[:2] + (0.0,))[1]  # without the normal term the whole gradient is 0 there
            assert (g0.v[same] == 0).all() and (g0.e[same] == 0).all() and (g0.v[mask & ~same] != 0).all()
            th, succ = LO.TH_D, np.nextafter(LO.TH_D, F32(1))
            assert (c["depth"] == th).any() and (c["depth"] == succ).any() and not mask[c["depth"] == th].any()
            if H > 3:
                assert mask[c["depth"] == succ].all() and mask[1, 1] and mask[H - 2, W - 2] and mask[1, W - 2] and mask[H - 2, 1]
        else:                                                                # |c| clearly below the floor on one half, clearly above on the other
            ln = LO._normal_parts(c["depth"], H, W, c["cam"], False)["len"].v
            inner = np.zeros((H, W), bool)
            inner[1:-1, 1:-1] = True
            assert (ln[inner & mask] < 0.9 * LO.FLOOR).mean() > 0.3 and (ln[inner & mask] > 1.1 * LO.FLOOR).mean() > 0.3
        r = (_note("pix_sums", name, s32.v, s), _note("pix_g_d", name, gd32.v, gd, ~amb))
        print(f"[gs loss cpu] pixel loss {name}: sums {r[0]:.3f}, g_d {r[1]:.3f}, ambiguous {int(amb.sum())} of {H * W}")
        assert r[0] <= LO.RATIO["pix_sums"] and r[1] <= LO.RATIO["pix_g_d"]


# ------------------------------------------------------------------------------------------------------------------ refine loss
def _refine_tensor64(c, H, W, coef):
    """the tensor formulation of tests/test_gs_gpu.py (pose refinement) in fp64: sums [5] and d/d depth of c_var (sum diff^2 - 2 mean sum diff)"""
    th = float(LO.TH_D)
    t = lambda a: torch.tensor(np.asarray(a, dtype=F32).astype(F64))
    d, gd, img, gt, alpha = t(c["depth"]).requires_grad_(True), t(c["gt_depth"]), t(c["img"]), t(c["gt"]), t(c["alpha"])
    a = alpha > float(F32(LO.REFINE_TH))
    m = a & (gd > th) & (d > th)
    diff = torch.log(d[m]) - torch.log(gd[m])
    sums = [torch.abs(gt - img)[:, a].sum(), a.sum(), diff.sum(), (diff ** 2).sum(), m.sum()]
    g = torch.autograd.grad(float(F32(coef[1])) * (sums[3] - 2 * float(F32(coef[2])) * sums[2]), d, allow_unused=True)[0]
    return np.array([float(s.detach()) for s in sums]), (g.numpy() if g is not None else np.zeros((H, W)))


def _refine_args(c, H, W):
    return c["img"], c["gt"], c["depth"], c["gt_depth"], c["alpha"], LO.REFINE_TH, H, W


def test_refine_loss_reference_and_restatement():
    for name, H, W, c in LO.refine_cases():
        args = _refine_args(c, H, W)
        s, s32 = LO.refine_loss_forward(*args), LO.refine_loss_forward(*args, f32=True)
        gi, gd = LO.refine_loss_backward(*args, LO.REFINE_COEF)
        gi32, gd32 = LO.refine_loss_backward(*args, LO.REFINE_COEF, f32=True)
        sums64, g64 = _refine_tensor64(c, H, W, LO.REFINE_COEF)
        _same64(sums64, s, (name, "sums"))
        _same64(g64, gd, (name, "g_d"))
        assert np.array_equal(gi, gi32) and s.e[1] == 0 and s.e[4] == 0 and s.v[1] == s32.v[1] and s.v[4] == s32.v[4]
        if name.endswith("below"):
            assert (s.v == 0).all() and (s.e == 0).all() and (gi == 0).all() and (gd.v == 0).all() and (gd.e == 0).all()
        elif name.endswith("no_depth"):
            assert s.v[1] == H * W and s.v[0] > 0 and (s.v[2:] == 0).all() and (s.e[2:] == 0).all() and (gd.v == 0).all() and (gi != 0).any()
        else:
            assert s.v[1] >= 1 and (H * W == 1 or 0 < s.v[4] < s.v[1] < H * W)
        r = (_note("ref_sums", name, s32.v, s), _note("ref_g_d", name, gd32.v, gd))
        assert r[0] <= LO.RATIO["ref_sums"] and r[1] <= LO.RATIO["ref_g_d"], (name, r)
    print(f"[gs loss cpu] refine loss: restatement error / model bound sums {_WORST['ref_sums'][0]:.3f}, g_d {_WORST['ref_g_d'][0]:.3f}")


# ------------------------------------------------------------------------------------------------------------------ 3-NN
def test_knn_chunk_counts_of_the_chosen_sizes():
    assert [LO.knn3_chunks(P) for P in (3, 4, 257, 2048, 2049, 5000)] == [0, 1, 1, 1, 2, 3]
    assert LO.knn3_chunks(16385) == 9 and LO.knn3_chunk_size(16385) == 2048 and 16385 - 8 * 2048 == 1          # one candidate in the last
    assert LO.knn3_chunks(32769) == 16 and LO.knn3_chunk_size(32769) == 2304 and 15 * 2304 > 32769 > 14 * 2304  # the last starts beyond P


@pytest.mark.parametrize("P", LO.KNN_SIZES)
def test_knn_exhaustive_reference_and_restatement(P):
    p = LO.knn_surface(P)
    ref = LO.knn3_mean_dist2(p)
    if P <= 5000:
        assert np.allclose(ref.v, LO.knn3_dense64(p), rtol=1e-13, atol=0)
    assert np.array_equal(ref.v[0], ref.v[P - 1]) and (ref.v > 0).all()     # (the duplicate is ONE neighbour at 0, not three)
    r = _note("knn", f"exhaustive P={P}", LO.knn3_exhaustive_f32(p), ref)
    print(f"[gs loss cpu] knn exhaustive P {P}: {LO.knn3_chunks(P)} chunks of {LO.knn3_chunk_size(P)}, restatement error / model bound {r:.3f}")
    assert r <= LO.RATIO["knn"]


@pytest.mark.parametrize("name", LO.KNN_GRID)
def test_knn_grid_reference_and_restatement(name):
    p = LO.knn_grid_case(name)
    ref = LO.knn3_mean_dist2(p)
    assert np.allclose(ref.v, LO.knn3_dense64(p), rtol=1e-13, atol=0)
    got, outside = LO.knn3_grid_f32(p)
    lo, cs, inv, g = LO.knn_grid_header(p)
    r = _note("knn", f"grid: {name}", got, ref)
    print(f"[gs loss cpu] knn grid {name}: P {len(p)}, grid {tuple(int(v) for v in g)}, cell {float(cs):.3g}, {int(outside.sum())} queries outside, "
          f"restatement error / model bound {r:.3f}")
    assert r <= LO.RATIO["knn"]
    if name.startswith("identical"):
        assert cs == 1 and tuple(g) == (1, 1, 1) and (ref.v == 0).all()
    if name == "two_sites":
        assert (ref.v == 0).all()
    if name == "collinear":
        assert g[1] == 1 and g[2] == 1 and g[0] > 1
    if name == "plane":
        assert g[2] == 1
    if name == "cauchy":
        assert outside.sum() >= 100
    if name == "outliers":
        assert outside.sum() == 5
    if name in LO.KNN_SHARED:
        assert LO.within(LO.knn3_exhaustive_f32(p), ref, "knn")[1] == 0


# ------------------------------------------------------------------------------------------------------------------ mutants
SSIM_MUTANTS = ("window_shift", "replicate_pad", "drop_halo", "c2_is_c1", "no_2a")
PIXEL_MUTANTS = ("border_normal", "q_gate_dropped", "ex_sign_flipped", "ge_threshold")
REFINE_MUTANTS = ("mean_not_subtracted", "alpha_ignored")
KNN_MUTANTS = ("self_included", "dup_by_distance", "last_chunk_dropped", "shell_early")


@pytest.mark.parametrize("mutant", SSIM_MUTANTS + PIXEL_MUTANTS + REFINE_MUTANTS + KNN_MUTANTS)
def test_mutant_is_rejected(mutant):
    """beyond K x bound on at least one element of at least one case"""
    beyond, worst = 0, 0.0

    def see(got, ref, group, keep=None):
        nonlocal beyond, worst
        r, n = LO.within(got, ref, group, keep)
        beyond, worst = beyond + n, max(worst, r)
    if mutant in SSIM_MUTANTS:
        for name, C, H, W, a, b in LO.ssim_cases():
            ref = LO.ssim_forward(a, b, C, H, W)
            if mutant != "no_2a":
                for g, x, y in zip(_SSIM_GROUPS, LO.ssim_forward(a, b, C, H, W, f32=True, mutants=(mutant,)), ref):
                    see(x.v, y, g)
            maps = [m.v for m in LO.ssim_forward(a, b, C, H, W, f32=True)[1:]]
            gs = LO.ssim_cotangent(C, H, W)
            if mutant != "c2_is_c1":
                see(LO.ssim_backward(a, b, *maps, gs, C, H, W, f32=True, mutants=(mutant,)).v, LO.ssim_backward(a, b, *maps, gs, C, H, W), "ssim_grad")
    elif mutant in PIXEL_MUTANTS:
        for name, H, W, c in LO.pixel_cases():
            args = _pixel_args(c, H, W)
            see(LO.pixel_loss_forward(*args, f32=True, mutants=(mutant,)).v, LO.pixel_loss_forward(*args), "pix_sums")
            gi, gd, amb = LO.pixel_loss_backward(*args, LO.PIXEL_COEF)
            see(LO.pixel_loss_backward(*args, LO.PIXEL_COEF, f32=True, mutants=(mutant,))[1].v, gd, "pix_g_d", ~amb)
    elif mutant in REFINE_MUTANTS:
        for name, H, W, c in LO.refine_cases():
            args = _refine_args(c, H, W)
            see(LO.refine_loss_backward(*args, LO.REFINE_COEF, f32=True, mutants=(mutant,))[1].v, LO.refine_loss_backward(*args, LO.REFINE_COEF)[1], "ref_g_d")
    elif mutant == "shell_early":
        for name in ("random9", "collinear", "outliers"):
            p = LO.knn_grid_case(name)
            see(LO.knn3_grid_f32(p, (mutant,))[0], LO.knn3_mean_dist2(p), "knn")
    else:
        for P in (5, 257, 2049):
            p = LO.knn_surface(P)
            see(LO.knn3_exhaustive_f32(p, (mutant,)), LO.knn3_mean_dist2(p), "knn")
    print(f"[gs loss cpu] mutant {mutant}: worst error / bound {worst:.3g}, elements beyond {beyond}")
    assert beyond > 0


@pytest.mark.parametrize("mutant,case", (("window_shift", "1x17x33 impulse (0,0)"), ("drop_halo", "1x17x33 impulse (16,32)"),
                                         ("replicate_pad", "1x1x1 random")))
def test_the_edge_cases_alone_reject_their_mutant(mutant, case):
    """what the impulses and the smallest image are there for"""
    name, C, H, W, a, b = next(c for c in LO.ssim_cases() if c[0] == case)
    ref, got = LO.ssim_forward(a, b, C, H, W), LO.ssim_forward(a, b, C, H, W, f32=True, mutants=(mutant,))
    assert sum(LO.within(x.v, y, g)[1] for g, x, y in zip(_SSIM_GROUPS, got, ref)) > 0


def test_ratio_table_is_the_measured_worst_plus_a_twentieth_rounded_up():
    """runs after the measuring tests of this module (pytest keeps file order)"""
    wrong = []
    for k, value in LO.RATIO.items():
        worst, where = _WORST.get(k, (0.0, "not measured"))
        rule = np.ceil((worst + 0.05) * 10 - 1e-9) / 10
        print(f"[gs loss cpu] RATIO {k:10s} measured {worst:.3f} ({where}) -> {rule:.1f}, K {max(1.0, 2 * rule):.1f}")
        if abs(value - rule) > 1e-9 or where == "not measured":
            wrong.append(k)
    assert not wrong, wrong
