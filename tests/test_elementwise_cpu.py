"""CPU: the reference-alone checks behind tests/elementwise_oracle.py.

  * every fp32 numpy restatement stays inside its bound with the measured RATIO (k = 1 units), i.e. with a factor 2 to spare under the k the
    GPU tests use -- this is where the table in the oracle's docstring comes from (each test prints its figures);
  * one named mutant per operation is REJECTED by the same check at the full k, so the GPU comparison is known to have teeth;
  * the fp64 references agree with torch where torch has the operation.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import elementwise_oracle as E

F32 = np.float32


def measured(got, fn):
    """largest (error - the part of the bound that does not scale with k) / (the part that does, at k = 1); fn(k) -> (ref, bound)"""
    ref, b1 = fn(1.0)
    _, b0 = fn(0.0)
    err = np.abs(E.f64(got) - ref)
    unit = b1 - b0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err <= b0, 0.0, (err - b0) / unit)
    return float(np.where(np.isfinite(r), r, np.inf).max())


def rejected(got, ref, bound):
    return E.ratio(got, ref, bound)[0] > 1.0


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("kind", E.LN_KINDS)
def test_layernorm_two_pass_inside_the_bound_one_pass_rejected(kind):
    worst, mut = 0.0, []
    for C in E.LN_GENERIC_C + E.LN_FAST_C + (192,):
        for eps in (1e-6, 1e-5):
            for adaln in (False, True):
                x = E.ln_rows(kind, 257, C, C)               # the GPU test's rows: 257 draws of the per-row mean reach |mu| ~ 9 sigma
                g, b, sc, sh = E.ln_params(C, C, adaln)
                fn = lambda k: E.layernorm64(x, g, b, eps, sc, sh, k=k)
                r = measured(E.layernorm_f32(x, g, b, eps, sc, sh), fn)
                worst = max(worst, r)
                ref, bound = fn(E.K["layernorm"])
                mut.append((C, E.ratio(E.layernorm_f32(x, g, b, eps, sc, sh, one_pass=True), ref, bound)[0]))
                if kind == "constant" and not adaln:
                    assert np.array_equal(E.layernorm_f32(x, g, b, eps), np.broadcast_to(b, x.shape)), "a constant row must give beta exactly"
    lo, hi = min(m for _, m in mut), max(m for _, m in mut)
    print(f"[layernorm {kind}] two-pass restatement {worst:.2f} of the k = 1 bound; one-pass mutant {lo:.2f} .. {hi:.2f} of the k = {E.K['layernorm']} bound")
    assert worst <= E.RATIO["layernorm"], worst
    if kind in ("massive", "near_constant"):
        assert all(m > 1.0 for C, m in mut), [(C, round(m, 2)) for C, m in mut]          # outside the FULL bound at every width


def test_layernorm_fp16_output_bound_adds_one_fp16_rounding():
    x = E.ln_rows("massive", 24, 260, 1)
    g, b, _, _ = E.ln_params(260, 1, False)
    y32 = E.layernorm_f32(x, g, b, 1e-6)
    ref, bound = E.layernorm64(x, g, b, 1e-6, fp16=True)
    assert not rejected(y32.astype(np.float16), ref, bound)
    assert rejected(y32.astype(np.float16).astype(np.float64) * (1 + 3 * E.H16), ref, bound)


def test_layernorm_reference_is_torch_layer_norm():
    x = E.ln_rows("massive", 7, 516, 2)
    g, b, sc, sh = E.ln_params(516, 2, True)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    ref = F.layer_norm(t(x), (516,), t(g), t(b), float(F32(1e-6)))
    assert np.abs(E.layernorm64(x, g, b, 1e-6)[0] - ref.numpy()).max() < 1e-12
    assert np.abs(E.layernorm64(x, g, b, 1e-6, sc, sh)[0] - (ref * (1 + t(sc)) + t(sh)).numpy()).max() < 1e-12


# ------------------------------------------------------------------------------------------------ im2col
@pytest.mark.parametrize("P,C,B", [(8, 1, 1), (16, 3, 2), (24, 3, 1)])
def test_im2col_reference_is_unfold_and_the_swap_is_seen(P, C, B):
    g = np.random.default_rng(P)
    img = g.standard_normal((B, C, 2 * P, 3 * P)).astype(F32)
    ref = F.unfold(torch.from_numpy(img).double(), P, stride=P).transpose(1, 2).reshape(-1, C * P * P).numpy()
    assert np.array_equal(E.im2col64(img, P), ref)
    assert not np.array_equal(E.im2col64(img, P, swap=True), ref)


def test_im2col_u8_restatement_is_within_one_fp16_ulp_and_monotone():
    img = np.arange(256, dtype=np.uint8).reshape(1, 1, 16, 16)
    got = E.im2col_u8_f32(img, 16).astype(np.float64)
    ref = E.im2col64(img, 16)
    assert np.abs(ref.reshape(-1) - (2.0 * np.arange(256) / 255.0 - 1.0)).max() < 1e-15
    assert (np.abs(got - ref) <= E.fp16_ulp(ref)).all()
    assert (np.diff(got.reshape(-1)) >= 0).all()


# ------------------------------------------------------------------------------------------------ column mean


def test_colmean_restatement_inside_the_bound_dropped_tail_rejected():
    worst = 0.0
    for M in E.COLMEAN_M:
        for C in (1, 63, 64, 65, 200):
            x = E.colmean_inputs(M, C, M * 1000 + C)
            r = measured(E.colmean_f32(x), lambda k: E.colmean64(x, k=k))
            worst = max(worst, r)
            if M % 16:                                                             # the tail loop has rows to add
                assert rejected(E.colmean_f32(x, drop_tail=True), *E.colmean64(x)), (M, C)
    print(f"[colmean] restatement {worst:.2f} of the k = 1 bound")
    assert worst <= E.RATIO["colmean"], worst


# ------------------------------------------------------------------------------------------------ upsample


def test_upsample_restatement_inside_the_bound_and_half_pixel_rejected():
    worst = 0.0
    for Hh, W in E.UPSAMPLE_HW:
        x = E.upsample_input(2, Hh, W, 16, Hh * 10 + W)
        r = measured(E.upsample_f32(x), lambda k: E.upsample64(x, k=k))
        worst = max(worst, r)
        assert r <= E.RATIO["upsample"], (Hh, W, r)
        ref, bound = E.upsample64(x)
        t = torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2)
        ac = F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1).numpy()
        assert np.abs(ac - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
        if Hh * W > 1:
            hp = F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1).numpy()
            assert rejected(hp.astype(np.float16), ref, bound), (Hh, W)
    print(f"[upsample] restatement {worst:.2f} of the k = 1 bound")


# ------------------------------------------------------------------------------------------------ DPT output stage
def test_dpt_final_restatement_inside_the_bound_and_bias_per_lane_rejected():
    worst = {"pts": 0.0, "conf": 0.0, "rgb": 0.0}
    for Cin in (8, 16, 24, 40, 64, 128, 512, 1024, 2048):
        for zb in (False, True):
            P = 131
            x, w, b = E.dpt_problem(P, Cin, 4, Cin + zb, zb)
            pts, conf = E.dpt_final_f32(x, w, b, 0)
            worst["pts"] = max(worst["pts"], measured(pts, lambda k: E.dpt_final64(x, w, b, 0, k=k)[:2]))
            worst["conf"] = max(worst["conf"], measured(conf, lambda k: E.dpt_final64(x, w, b, 0, k=k)[2:]))
            rgb, _ = E.dpt_final_f32(x, w[:3], b[:3], 1)
            worst["rgb"] = max(worst["rgb"], measured(rgb, lambda k: E.dpt_final64(x, w[:3], b[:3], 1, k=k)[:2]))
            ref = E.dpt_final64(x, w, b, 0)
            d = np.log1p(np.sqrt((ref[0] ** 2).sum(1)))
            if zb:
                assert d.min() == 0.0 and 0 < d[d > 0].min() < 1e-8 and d.max() > 1.5, (Cin, d[d > 0].min(), d.max())
            lpp = Cin // 8
            if not zb and lpp > 1:
                mut = E.dpt_final64(x, w, b, 0, bias_per_lane=lpp)
                assert rejected(mut[0], ref[0], ref[1]) and rejected(mut[2], ref[2], ref[3]), Cin
    for Cin in (24, 40, 1024):                 # the per-lane kernel's chain from the bias: inside the constant-free chain bound
        x, w, b = E.dpt_problem(131, Cin, 4, Cin, False)
        pts, conf = E.dpt_final_f32(x, w, b, 0, chain=True)
        ref = E.dpt_final64(x, w, b, 0, chain=True)
        rp, rc = E.ratio(pts, ref[0], ref[1])[0], E.ratio(conf, ref[2], ref[3])[0]
        tree = E.dpt_final64(x, w, b, 0)
        print(f"[dpt_final per-lane chain Cin={Cin}] restatement {rp:.2f} / {rc:.2f} of the chain bound, {E.ratio(pts, tree[0], tree[1])[0]:.2f} of the tree bound")
        assert rp <= 1.0 and rc <= 1.0
    print(f"[dpt_final] restatement, of the k = 1 bound: {worst}")
    assert all(worst[o] <= E.RATIO[o] for o in worst), worst


@pytest.mark.parametrize("nch", [3, 4])
def test_postprocess_pts_restatement_inside_the_bound_and_ignored_sign_rejected(nch):
    raw = E.pts_raw(nch, nch)
    assert (raw[:, 2] > 0).any() and (raw[:, 2] < 0).any()
    for pos_z in (False, True):
        pts, conf = E.postprocess_pts_f32(raw, pos_z)
        r = measured(pts, lambda k: E.postprocess_pts64(raw, pos_z, k=k)[:2])
        rc = measured(conf, lambda k: E.postprocess_pts64(raw, pos_z, k=k)[2:]) if nch == 4 else 0.0
        print(f"[postprocess_pts nch={nch} pos_z={pos_z}] restatement: points {r:.2f}, confidence {rc:.2f} of the k = 1 bound")
        assert r <= E.RATIO["pts"] and rc <= E.RATIO["conf"]
    ref = E.postprocess_pts64(raw, True)
    assert (ref[0][:, 2] >= 0).all() and np.all(ref[0][1:3] == 0)
    assert rejected(E.postprocess_pts64(raw, True, ignore_sign=True)[0], ref[0], ref[1])


def test_postprocess_pose_restatement_inside_the_bound():
    raw = E.pose_raw()
    r = measured(E.postprocess_pose_f32(raw), lambda k: E.postprocess_pose64(raw, k=k))
    print(f"[postprocess_pose] restatement {r:.2f} of the k = 1 bound")
    assert r <= E.RATIO["pts"]
    ref, _ = E.postprocess_pose64(raw)
    assert (ref[:, 3] >= 0).all() and np.all(ref[0::4, 3:] == 0) and np.all(ref[:4, :3] == 0)
    n = np.sqrt((ref[:, 3:] ** 2).sum(1))
    assert np.allclose(n[n > 0], 1.0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ GEMV


def test_gemv_restatement_inside_the_interval_and_unrounded_activation_rejected():
    worst, amb_total = 0.0, 0
    for Kd in (8, 504, 512, 520, 768):
        for silu in (False, True):
            for act in (0, 1):
                X, W, b, res = E.gemv_problem(8, 5, Kd, Kd + act, bias=bool(act), res=not act)
                got = E.gemv_f32(X, W, b, act, res, silu)

                def fn(k):
                    lo, hi, _ = E.gemv_interval(X, W, b, act, res, silu, k=k)
                    return 0.5 * (lo + hi), 0.5 * (hi - lo)
                r = measured(got, fn)
                worst = max(worst, r)
                assert r <= E.RATIO["gemv"], (Kd, silu, act, r)
                lo, hi, amb = E.gemv_interval(X, W, b, act, res, silu)
                amb_total += amb
                assert (amb == 0) or silu
                if Kd >= 504:
                    mlo, _, _ = E.gemv_interval(X, W, b, act, res, silu, round_act=False, k=0.0)
                    assert E.interval_ratio(mlo, lo, hi)[0] > 1.0, (Kd, silu, act)
    print(f"[gemv] restatement {worst:.2f} of the k = 1 widening; {amb_total} activations within a few ulp of an fp16 tie")


def test_gemv_interval_holds_both_roundings_of_a_tie():
    """silu(x) made to sit within tau of the midpoint of two fp16 numbers: both roundings of that activation must be inside [lo, hi]"""
    X, W, b, _ = E.gemv_problem(1, 3, 8, 1)
    a, a2 = np.float16(0.5), np.nextafter(np.float16(0.5), np.float16(1))
    target = 0.5 * (float(a) + float(a2))
    lo_, hi_ = 0.0, 4.0
    for _ in range(200):                                  # invert silu by bisection in fp64, then take the nearest fp32
        mid = 0.5 * (lo_ + hi_)
        lo_, hi_ = (mid, hi_) if mid / (1 + np.exp(-mid)) < target else (lo_, mid)
    X[0, 3] = F32(lo_)
    lo, hi, amb = E.gemv_interval(X, W, b, 0, None, True)
    assert amb == 1
    for cand in (a, a2):
        act = (E.f64(X) / (1 + np.exp(-E.f64(X)))).astype(np.float16).astype(np.float64)
        act[0, 3] = float(cand)
        y = act @ E.f64(W).T + E.f64(b)
        assert ((y >= lo) & (y <= hi)).all()


# ------------------------------------------------------------------------------------------------ ConvTranspose


@pytest.mark.parametrize("s,Cin,Cout,Hh,W,B", E.CONVT)
def test_conv_transpose_restatement_inside_the_bound_and_swapped_scatter_rejected(s, Cin, Cout, Hh, W, B):
    x, w, wt, b = E.convt_problem(s, Cin, Cout, Hh, W, B)
    r = measured(E.conv_transpose_f32(x, wt, b, s), lambda k: E.conv_transpose64(x, wt, b, s, k=k))
    print(f"[convT s={s} Cin={Cin}] restatement {r:.2f} of the k = 1 bound")
    assert r <= E.RATIO["convt"]
    ref, bound = E.conv_transpose64(x, wt, b, s)
    t = F.conv_transpose2d(torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2), torch.from_numpy(w.astype(np.float64)),
                           torch.from_numpy(b.astype(np.float64)), stride=s).permute(0, 2, 3, 1).numpy()
    assert np.abs(t - ref).max() < 1e-11
    assert rejected(E.conv_transpose64(x, wt, b, s, swap=True)[0].astype(np.float16), ref, bound)
