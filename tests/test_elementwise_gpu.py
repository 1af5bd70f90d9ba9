"""GPU: the small kernels every window runs through (csrc/elementwise.hip, gemv_kernel and the ConvTranspose pixel-shuffle epilogue of
csrc/gemm.hip), PER ELEMENT against the fp64 references and rounding-model bounds of tests/elementwise_oracle.py (whose constants are
measured by tests/test_elementwise_cpu.py), at the smallest shapes that reach every branch: trip counts of the strided loops, ragged tails,
leading dimensions other than the width, the second grid-stride trip of the coalesced DPT kernel.

Every output is a view inside a sentinel-filled buffer with its payload pre-filled with NaN (Guard of tests/gemm_forms_child.py): afterwards
the payload is finite and no guard element has changed.  A failure names the worst element, both values and the number of violations.
The last tests make the calls the entry points must REFUSE (C ABI: CUT3R_ERR_ARG before any launch, outputs untouched; ops: ValueError).
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cut3r_slam_amd import _lib, ops  # noqa: E402
from tests import elementwise_oracle as E  # noqa: E402
from tests.gemm_forms_child import SENT, Guard, rows_in  # noqa: E402

DEV = "cuda:0"
F16, F32 = torch.float16, torch.float32
WORST = {}                                  # kernel -> largest error / bound seen by this file (printed by the last test)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def flat_guard(shape, dtype, nan=True):
    """a contiguous tensor of `shape` with 64 guard elements in front of it and behind it (entry points that want contiguous outputs)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 128,), SENT, dtype=dtype, device=DEV)
    return Guard(buf, [buf[64:64 + n].view(*shape)], nan)


def inside(t, top=1, left=0, right=8, bottom=1):
    """t [M, N] (numpy) on the GPU as a view of a zero buffer: `top` rows above, `left` / `right` columns beside, `bottom` rows below"""
    M, N = t.shape
    buf = torch.zeros(top + M + bottom, left + N + right, dtype=torch.from_numpy(t[:0]).dtype, device=DEV)
    buf[top:top + M, left:left + N] = dev(t)
    return buf[top:top + M, left:left + N]


def holds(kernel, name, got, ref, bound):
    r, msg = E.describe(name, got.detach().cpu().numpy(), ref, bound)
    WORST[kernel] = max(WORST.get(kernel, 0.0), r)
    assert r <= 1.0, msg


# ------------------------------------------------------------------------------------------------ LayerNorm
def _ln_launch(xv, prm, eps, M, C, mode, ada):
    g, b, sc, sh = prm
    g16 = rows_in([M], C, F16, pad=8) if mode in ("f16", "both") else None
    g32 = rows_in([M], C, F32, pad=12) if mode in ("f32", "both") else None
    ops.layernorm(xv[:M], dev(g), dev(b), eps, g16.views[0] if g16 else None, g32.views[0] if g32 else None,
                  dev(sc) if ada else None, dev(sh) if ada else None)
    return g16, g32


@pytest.mark.parametrize("C", E.LN_GENERIC_C + E.LN_FAST_C)
def test_layernorm_per_element(C):
    """generic kernel: C = 4 (one lane), 48, 252 (63 lanes), 256 (one whole trip), 260 (second trip, one lane), 516, 1280, 2048 (all 8
    trips); fast kernels 768 / 1024 / 1536.  x = big[1:, 64:64+C] (ldx = C + 128), outputs with ld16 = C + 8, ld32 = C + 12."""
    kernel = "layernorm_fast" if C in E.LN_FAST_C else "layernorm"
    for ki, kind in enumerate(E.LN_KINDS):
        x = E.ln_rows(kind, 257, C, C)
        xv = inside(x, top=1, left=64, right=64)
        assert xv.stride(0) == C + 128
        prm = E.ln_params(C, C, True)
        ref = {(eps, ada): (E.layernorm64(x, *prm[:2], eps, *(prm[2:] if ada else (None, None))),
                            E.layernorm64(x, *prm[:2], eps, *(prm[2:] if ada else (None, None)), fp16=True))
               for eps in (1e-6, 1e-5) for ada in (False, True)}
        cases = [(257, "both", eps, ada) for eps in (1e-6, 1e-5) for ada in (False, True)]
        cases += [(M, ("f16", "f32", "both")[(i + ki) % 3], (1e-6, 1e-5)[(i + ki) % 2], bool(((i + ki) // 2) % 2)) for i, M in enumerate((1, 3, 4, 5))]
        for M, mode, eps, ada in cases:
            name = f"layernorm C={C} {kind} M={M} {mode} eps={eps} adaLN={ada}"
            g16, g32 = _ln_launch(xv, prm, eps, M, C, mode, ada)
            (y, b32), (_, b16) = ref[(eps, ada)]
            if g32:
                g32.check(name)
                holds(kernel, name + " fp32", g32.views[0], y[:M], b32[:M])
            if g16:
                g16.check(name)
                holds(kernel + "_f16", name + " fp16", g16.views[0], y[:M], b16[:M])
            if kind == "constant" and not ada:                # x - mean is exactly 0: the output is beta, bit for bit
                beta = dev(prm[1])
                assert g32 is None or torch.equal(g32.views[0], beta.expand(M, C)), name
                assert g16 is None or torch.equal(g16.views[0], beta.half().expand(M, C)), name


@pytest.mark.parametrize("C", E.LN_FAST_C)
def test_layernorm_dual_gives_the_bits_of_two_layernorms(C):
    for kind in E.LN_KINDS:
        x = E.ln_rows(kind, 257, C, C + 1)
        xv = inside(x, top=1, left=64, right=64)
        p1, p2 = E.ln_params(C, C, False), E.ln_params(C, C + 7, False)
        for M in (1, 5, 257):
            name = f"layernorm_dual C={C} {kind} M={M}"
            r1, r2 = torch.empty(M, C, dtype=F16, device=DEV), torch.empty(M, C, dtype=F16, device=DEV)
            ops.layernorm(xv[:M], dev(p1[0]), dev(p1[1]), 1e-6, r1, None)
            ops.layernorm(xv[:M], dev(p2[0]), dev(p2[1]), 1e-6, r2, None)
            ga, gb = rows_in([M], C, F16, pad=8), rows_in([M], C, F16, pad=24)
            assert ga.views[0].stride(0) != gb.views[0].stride(0)
            ops.layernorm_dual(xv[:M], dev(p1[0]), dev(p1[1]), ga.views[0], dev(p2[0]), dev(p2[1]), gb.views[0], 1e-6)
            ga.check(name)
            gb.check(name)
            assert torch.equal(ga.views[0], r1) and torch.equal(gb.views[0], r2), name


# ------------------------------------------------------------------------------------------------ im2col, cast
@pytest.mark.parametrize("P", [8, 16, 24])
def test_im2col_per_element(P):
    for Cc in (1, 3):
        for B in (1, 2):
            for Hh, W in ((P, P), (2 * P, 3 * P)):
                g = np.random.default_rng(P * 100 + Cc * 10 + B)
                name = f"im2col P={P} C={Cc} B={B} {Hh}x{W}"
                shape = (B * (Hh // P) * (W // P), Cc * P * P)
                img = g.standard_normal((B, Cc, Hh, W)).astype(np.float32)
                gd = flat_guard(shape, F16)
                ops.im2col_patch(dev(img), P, gd.views[0])
                gd.check(name)
                ref = torch.nn.functional.unfold(torch.from_numpy(img), P, stride=P).transpose(1, 2).reshape(shape).half()
                assert np.array_equal(ref.double().numpy(), E.im2col64(img, P).astype(np.float16).astype(np.float64))
                assert torch.equal(gd.views[0].cpu(), ref), name
                u8 = g.integers(0, 256, (B, Cc, Hh, W), dtype=np.uint8)
                gd = flat_guard(shape, F16)
                ops.im2col_patch(dev(u8), P, gd.views[0])
                gd.check(name + " u8")
                ref8 = E.im2col64(u8, P)
                err = np.abs(gd.views[0].cpu().double().numpy() - ref8)
                assert (err <= E.fp16_ulp(ref8)).all(), (name, float((err / E.fp16_ulp(ref8)).max()))


@pytest.mark.parametrize("P", [8, 16])
def test_im2col_u8_every_byte_value_within_one_ulp_and_monotone(P):
    img = np.arange(256, dtype=np.uint8).reshape(1, 1, 16, 16)
    gd = flat_guard(((16 // P) ** 2, P * P), F16)
    ops.im2col_patch(dev(img), P, gd.views[0])
    gd.check("im2col u8 ramp")
    got = gd.views[0].cpu().double().numpy()
    by_byte = np.empty(256)
    by_byte[img.reshape(-1)[E.im2col_index(1, 1, 16, 16, P)].reshape(-1)] = got.reshape(-1)
    ref = 2.0 * np.arange(256) / 255.0 - 1.0
    assert (np.abs(by_byte - ref) <= E.fp16_ulp(ref)).all()
    assert (np.diff(by_byte) >= 0).all()


def test_cast_gives_the_bits_of_torch_half():
    special = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -23, 65504.0, -65504.0, 65519.99, 65520.0, -65520.0, 1e5, -1e38,
                        0.0, -0.0, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20), -2.0 ** -25, 3 * 2.0 ** -25, 1e-10, -1e-10, 2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -12)], np.float32)
    for M in (1, 5):
        for Cc in (4, 260):
            g = np.random.default_rng(M + Cc)
            x = g.standard_normal((M, Cc)).astype(np.float32)
            sub = (10.0 ** g.uniform(np.log10(6e-8), np.log10(6e-5), M * Cc) * np.sign(g.standard_normal(M * Cc))).astype(np.float32).reshape(M, Cc)
            x[:, ::2] = sub[:, ::2]                                              # fp16 subnormals on every other element
            flat = x.reshape(-1)
            n = min(len(special), flat.size)
            flat[:n] = special[:n]
            xv = inside(x, top=1, left=4, right=4)
            gd = rows_in([M], Cc, F16, pad=12)
            ops.cast_f16(xv, gd.views[0])
            torch.cuda.synchronize()
            got = gd.views[0].cpu()
            ref = torch.from_numpy(x).half()
            assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), (M, Cc, int((got.view(torch.int16) != ref.view(torch.int16)).sum()))
            gd.views[0].nan_to_num_(0.0, 0.0, 0.0)                               # (inf is a correct result here; the guard check wants finite payloads)
            gd.check(f"cast M={M} C={Cc}")


# ------------------------------------------------------------------------------------------------ column mean
@pytest.mark.parametrize("Cc", [1, 63, 64, 65, 200])
def test_colmean_per_element(Cc):
    for M in E.COLMEAN_M:
        name = f"colmean M={M} C={Cc}"
        x = E.colmean_inputs(M, Cc, M * 1000 + Cc)
        gd = rows_in([1], Cc, F32, pad=8)
        ops.colmean(inside(x, top=1, left=3, right=4), gd.views[0][0])
        gd.check(name)
        ref, bound = E.colmean64(x)
        holds("colmean", name, gd.views[0][0], ref, bound)


@pytest.mark.parametrize("Cc", [1, 63, 64, 65, 200])
def test_colmean_batched_per_element(Cc):
    for M in E.COLMEAN_M:
        name = f"colmean_batched M={M} C={Cc}"
        x = np.stack([E.colmean_inputs(M, Cc, M * 1000 + Cc + 7 * z) for z in range(3)])
        buf = torch.zeros(4, M + 2, Cc + 5, device=DEV)
        buf[:3, 1:1 + M, 2:2 + Cc] = dev(x)
        xv = buf[:3, 1:1 + M, 2:2 + Cc]
        assert not xv.is_contiguous() and xv.stride(0) != M * xv.stride(1)
        gd = rows_in([3], Cc, F32, pad=8)
        ops.colmean_batched(xv, gd.views[0])
        gd.check(name)
        ref, bound = E.colmean64(x)
        holds("colmean_batched", name, gd.views[0], ref, bound)


# ------------------------------------------------------------------------------------------------ upsample
@pytest.mark.parametrize("Cc", [8, 16, 256])
def test_upsample2x_per_element(Cc):
    for Hh, W in E.UPSAMPLE_HW:
        for B in (1, 2):
            name = f"upsample2x {B}x{Hh}x{W}x{Cc}"
            x = E.upsample_input(B, Hh, W, Cc, Hh * 10 + W + Cc)
            gd = flat_guard((B, 2 * Hh, 2 * W, Cc), F16)
            ops.upsample2x(dev(x), gd.views[0])
            gd.check(name)
            holds("upsample2x", name, gd.views[0], *E.upsample64(x))


# ------------------------------------------------------------------------------------------------ DPT output stage
def _dpt_case(kernel, P, Cin, seed, zero_bias):
    for mode in (0, 1):
        name = f"dpt_final mode={mode} P={P} Cin={Cin} zero_bias={zero_bias}"
        nout = 4 if mode == 0 else 3
        x, w, b = E.dpt_problem(P, Cin, nout, seed, zero_bias)
        gp, gc = flat_guard((P, 3), F32), (flat_guard((P,), F32) if mode == 0 else None)
        ops.dpt_final(dev(x), dev(w), dev(b), mode, gp.views[0], gc.views[0] if gc else None)
        gp.check(name)
        pts, pb, conf, cb = E.dpt_final64(x, w, b, mode, chain=kernel.endswith("per_lane"))
        holds(kernel + ("_pts" if mode == 0 else "_rgb"), name, gp.views[0], pts, pb)
        if gc:
            gc.check(name)
            holds(kernel + "_conf", name + " conf", gc.views[0], conf, cb)


@pytest.mark.parametrize("Cin", [8, 16, 64, 128, 512])
def test_dpt_final_coalesced_per_element(Cin):
    ppw = 64 // (Cin // 8)
    for i, P in enumerate(sorted({1, 3, ppw - 1, ppw + 1, 4099} - {0})):
        _dpt_case("dpt_final_coalesced", P, Cin, Cin + P, zero_bias=bool(i % 2) or P == 4099)


@pytest.mark.parametrize("Cin", [24, 40, 1024, 2048])
def test_dpt_final_per_lane_per_element(Cin):
    for i, P in enumerate((1, 3, 63, 65, 4099)):
        _dpt_case("dpt_final_per_lane", P, Cin, Cin + P, zero_bias=bool(i % 2) or P == 4099)


def test_dpt_final_coalesced_second_grid_stride_trip():
    """8192 blocks x 4 waves x 1 pixel per wave at Cin = 512: pixels from 32768 on are a wave's second trip (production: 384 x 512 images at
    Cin = 128 exceed one trip as well)"""
    _dpt_case("dpt_final_coalesced", 32768 + 5, 512, 1, zero_bias=True)


@pytest.mark.parametrize("nch", [3, 4])
def test_postprocess_pts_per_element(nch):
    raw = E.pts_raw(nch, nch)
    P = raw.shape[0]
    for pos_z in (False, True):
        name = f"postprocess_pts nch={nch} pos_z={pos_z}"
        gp, gc = flat_guard((P, 3), F32), (flat_guard((P,), F32) if nch == 4 else None)
        ops.postprocess_pts(dev(raw), pos_z, gp.views[0], gc.views[0] if gc else None)
        gp.check(name)
        pts, pb, conf, cb = E.postprocess_pts64(raw, pos_z)
        holds("postprocess_pts", name, gp.views[0], pts, pb)
        if gc:
            gc.check(name)
            holds("postprocess_pts_conf", name + " conf", gc.views[0], conf, cb)


def test_postprocess_pose_per_element():
    raw = E.pose_raw()
    gd = flat_guard(raw.shape, F32)
    ops.postprocess_pose(dev(raw), gd.views[0])
    gd.check("postprocess_pose")
    holds("postprocess_pose", "postprocess_pose", gd.views[0], *E.postprocess_pose64(raw))


# ------------------------------------------------------------------------------------------------ GEMV
@pytest.mark.parametrize("Kd", [8, 504, 512, 520, 768])
def test_gemv_inside_the_interval(Kd):
    """K = 8 (one lane), 504 (a 512-wide trip short by one lane), 512, 520 and 768 (ragged second trips); N around the 4 columns of a
    workgroup; X, W, the output and the residual all strided; bias / GELU / residual / SiLU rotate through their 16 combinations"""
    ki = [8, 504, 512, 520, 768].index(Kd)
    i = 0
    for M in (1, 8, 64):
        for N in (1, 3, 4, 5, 1536):
            f = (3 * i + 5 * ki) % 16
            i += 1
            bias, act, res, silu = bool(f & 1), (f >> 1) & 1, bool(f & 4), bool(f & 8)
            name = f"gemv M={M} N={N} K={Kd} bias={bias} act={act} res={res} silu_in={silu}"
            X, W, b, r = E.gemv_problem(M, N, Kd, M * 7 + N + Kd, bias, res)
            gd = rows_in([M], N, F32, pad=8)
            ops.gemv(inside(X, top=1, left=1, right=3), inside(W, top=1, left=8, right=8), gd.views[0], dev(b) if bias else None, act,
                     inside(r, top=2, left=1, right=2) if res else None, silu)
            gd.check(name)
            lo, hi, _ = E.gemv_interval(X, W, b, act, r, silu)
            holds("gemv", name, gd.views[0], 0.5 * (lo + hi), 0.5 * (hi - lo))


# ------------------------------------------------------------------------------------------------ ConvTranspose pixel shuffle
@pytest.mark.parametrize("s,Cin,Cout,Hh,W,B", E.CONVT)
def test_conv_transpose_per_element(s, Cin, Cout, Hh, W, B):
    name = f"convT s={s} {Cin}->{Cout} {B}x{Hh}x{W}"
    x, _, wt, b = E.convt_problem(s, Cin, Cout, Hh, W, B)
    gd = flat_guard((B, Hh * s, W * s, Cout), F16)
    ops.conv_transpose_nhwc(dev(x), dev(wt), gd.views[0], dev(b), s)
    gd.check(name)
    holds("conv_transpose", name, gd.views[0], *E.conv_transpose64(x, wt, b, s))


# ------------------------------------------------------------------------------------------------ refusals
def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + off) if t is not None else C.c_void_p(0)


def test_entry_points_refuse_and_leave_the_outputs_alone():
    """Only calls the entry point rejects BEFORE any launch: each returns CUT3R_ERR_ARG (1), the NaN payloads and the guards are as they
    were.  The same calls without the offending argument return 0, so the refusals are the rules'."""
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    M, Cc = 5, 768
    x = torch.randn(M, Cc + 8, device=DEV)
    g1, b1, g2, b2, sc, sh = (torch.randn(Cc + 8, device=DEV) for _ in range(6))
    o16, o16b, o32 = rows_in([M], Cc, F16, pad=8), rows_in([M], Cc, F16, pad=8), rows_in([M], Cc, F32, pad=8)
    y16, y16b, y32 = o16.views[0], o16b.views[0], o32.views[0]

    def ln(xo=0, go=0, bo=0, o16o=0, o32o=0, sco=0, sho=0, eps=1e-6, mod=True):
        return lib.cut3r_layernorm(_p(x, xo), Cc + 8, _p(g1, go), _p(b1, bo), eps, M, Cc, _p(y16, o16o), y16.stride(0), _p(y32, o32o), y32.stride(0),
                                   _p(sc if mod else None, sco), _p(sh if mod else None, sho), st)

    def dual(xo=0, g1o=0, b1o=0, y1o=0, g2o=0, b2o=0, y2o=0, eps=1e-6, width=Cc):
        return lib.cut3r_layernorm_dual(_p(x, xo), Cc + 8, _p(g1, g1o), _p(b1, b1o), _p(y16, y1o), y16.stride(0), _p(g2, g2o), _p(b2, b2o),
                                        _p(y16b, y2o), y16b.stride(0), eps, M, width, st)

    cases = {"ln x + 4 B": lambda: ln(xo=4), "ln x + 8 B": lambda: ln(xo=8), "ln gamma + 4 B": lambda: ln(go=4), "ln beta + 8 B": lambda: ln(bo=8),
             "ln y16 + 4 B": lambda: ln(o16o=4), "ln y16 + 2 B": lambda: ln(o16o=2), "ln y32 + 8 B": lambda: ln(o32o=8),
             "ln scale + 4 B": lambda: ln(sco=4), "ln shift + 8 B": lambda: ln(sho=8),
             "dual eps = 0": lambda: dual(eps=0.0), "dual eps < 0": lambda: dual(eps=-1e-6), "dual eps NaN": lambda: dual(eps=float("nan")),
             "dual C = 512": lambda: dual(width=512), "dual C = 0": lambda: dual(width=0), "dual C = 772": lambda: dual(width=772),
             "dual x + 8 B": lambda: dual(xo=8), "dual g1 + 4 B": lambda: dual(g1o=4), "dual b1 + 8 B": lambda: dual(b1o=8),
             "dual g2 + 8 B": lambda: dual(g2o=8), "dual b2 + 4 B": lambda: dual(b2o=4), "dual y1 + 4 B": lambda: dual(y1o=4),
             "dual y2 + 2 B": lambda: dual(y2o=2)}
    # cast
    cx = torch.randn(M, 264, device=DEV)
    cast = lambda xo=0, yo=0: lib.cut3r_cast_f32_f16(_p(cx, xo), 264, _p(y16, yo), y16.stride(0), M, 260, st)
    cases.update({"cast x + 4 B": lambda: cast(xo=4), "cast x + 8 B": lambda: cast(xo=8), "cast y + 4 B": lambda: cast(yo=4), "cast y + 2 B": lambda: cast(yo=2)})
    # upsample (B, H, W, C) = (1, 2, 3, 16): 192 input and 768 output elements, the buffers leave room for the offsets
    ux = torch.randn(256, device=DEV).half()
    up = flat_guard((1, 4, 6, 16 + 1), F16)                   # (room for a shifted start inside the payload)
    ups = lambda io=0, oo=0: lib.cut3r_upsample2x_nhwc(_p(ux, io), _p(up.views[0], oo), 1, 2, 3, 16, st)
    cases.update({"upsample in + 8 B": lambda: ups(io=8), "upsample in + 2 B": lambda: ups(io=2), "upsample out + 8 B": lambda: ups(oo=8)})
    # dpt_final
    P, Cin = 9, 64
    dx, dw, db = torch.randn(P + 1, Cin, device=DEV).half(), torch.randn(4, Cin, device=DEV) * 0.1, torch.zeros(4, device=DEV)
    dp, dc = flat_guard((P, 3), F32), flat_guard((P,), F32)
    dpt = lambda io=0, mode=0: lib.cut3r_dpt_final(_p(dx, io), P, Cin, _p(dw), _p(db), mode, _p(dp.views[0]), _p(dc.views[0]), st)
    cases.update({"dpt_final in + 8 B": lambda: dpt(io=8), "dpt_final in + 2 B": lambda: dpt(io=2)})
    # gemv
    gX, gW, gb = torch.randn(3, 64, device=DEV), torch.randn(6, 72, device=DEV).half(), torch.randn(5, device=DEV)
    gy = rows_in([3], 5, F32, pad=8)
    gemv = lambda act=0, wo=0: lib.cut3r_gemv_f16w(_p(gX), 64, _p(gW, wo), 72, _p(gb), _p(gy.views[0]), gy.views[0].stride(0), 3, 5, 64, act, _p(None), 0, 0, st)
    cases.update({"gemv act = 2 (ReLU)": lambda: gemv(act=2), "gemv act = -1": lambda: gemv(act=-1), "gemv act = 3": lambda: gemv(act=3),
                  "gemv W + 8 B": lambda: gemv(wo=8), "gemv W + 2 B": lambda: gemv(wo=2)})
    # LayerNorm fold wider than the 16 slabs the epilogue reads: the descriptor ops would build, with ops' own limit lifted
    Kw, Nw, Mw = 1088, 64, 70
    A, Wf = torch.randn(Mw, Kw, device=DEV).half(), torch.randn(Nw, Kw, device=DEV).half()
    stats, cs, fb = torch.ones(Kw // 64, Mw, 2, device=DEV), torch.zeros(Nw, device=DEV), torch.zeros(Nw, device=DEV)
    fo = rows_in([Mw], Nw, F16, pad=8)
    keep = ops.LN_FOLD_MAX_K
    try:
        ops.LN_FOLD_MAX_K = 1 << 20
        desc = ops._linear_desc(A, Wf, fo.views[0], fb, 0, None, 0, ln=(stats, cs, 1e-6))
        stats16 = stats[:16].contiguous()
        ok_desc = ops._linear_desc(A[:, :1024], Wf[:, :1024], fo.views[0], fb, 0, None, 0, ln=(stats16, cs, 1e-6))
    finally:
        ops.LN_FOLD_MAX_K = keep
    cases["gemm ln fold K = 1088"] = lambda: lib.cut3r_gemm_f16(C.byref(desc), st)
    guards = (o16, o16b, o32, up, dp, dc, gy, fo)
    for name, fn in cases.items():
        rc = fn()
        assert rc == 1, (name, rc)
        for gd in guards:
            gd.untouched(name)
    # the rules' refusals: the same calls with nothing wrong are accepted
    for name, fn in {"ln": ln, "dual": dual, "cast": cast, "upsample": ups, "dpt_final": dpt, "gemv": gemv,
                     "gemm ln fold K = 1024": lambda: lib.cut3r_gemm_f16(C.byref(ok_desc), st)}.items():
        assert fn() == 0, name
    torch.cuda.synchronize()
    fo.check("gemm ln fold K = 1024")
    assert bool(torch.isfinite(y32).all()) and bool(torch.isfinite(gy.views[0]).all()) and bool(torch.isfinite(dp.views[0]).all())


def test_ops_refuse_with_a_readable_message():
    M, Cc = 5, 768
    big = torch.randn(M, Cc + 8, device=DEV)
    g, b = torch.randn(Cc, device=DEV), torch.randn(Cc, device=DEV)
    o16, o32 = rows_in([M], Cc, F16, pad=8), rows_in([M], Cc, F32, pad=8)
    gX, gW = torch.randn(3, 64, device=DEV), torch.randn(6, 72, device=DEV).half()
    gy = rows_in([3], 5, F32, pad=8)
    calls = {
        "layernorm x at a column offset": (lambda: ops.layernorm(big[:, 2:2 + Cc], g, b, 1e-6, o16.views[0], o32.views[0]), "boundary"),
        "layernorm out16 at a column offset": (lambda: ops.layernorm(big[:, :Cc], g, b, 1e-6, o16.buf[1:1 + M, 2:2 + Cc], None), "boundary"),
        "layernorm_dual eps = 0": (lambda: ops.layernorm_dual(big[:, :Cc], g, b, o16.views[0], g, b, o16.views[0], 0.0), "eps"),
        "layernorm_dual x at a column offset": (lambda: ops.layernorm_dual(big[:, 1:1 + Cc], g, b, o16.views[0], g, b, o16.views[0]), "boundary"),
        "cast x at a column offset": (lambda: ops.cast_f16(big[:, 1:1 + Cc], o16.views[0]), "boundary"),
        "gemv ReLU": (lambda: ops.gemv(gX, gW[:5, :64], gy.views[0], None, 2), "act"),
        "gemv W at a column offset": (lambda: ops.gemv(gX, gW[:5, 4:68], gy.views[0]), "boundary"),
        "upsample2x input off the 16-byte grid": (lambda: ops.upsample2x(torch.zeros(200, dtype=F16, device=DEV)[4:196].view(1, 2, 3, 32),
                                                                        torch.empty(1, 4, 6, 32, dtype=F16, device=DEV)), "boundary"),
        "dpt_final input off the 16-byte grid": (lambda: ops.dpt_final(torch.zeros(9 * 64 + 8, dtype=F16, device=DEV)[4:4 + 9 * 64].view(9, 64),
                                                                       torch.zeros(3, 64, device=DEV), torch.zeros(3, device=DEV), 1,
                                                                       torch.empty(9, 3, device=DEV)), "boundary"),
    }
    for name, (fn, word) in calls.items():
        with pytest.raises(ValueError, match=word):
            fn()
        for gd in (o16, o32, gy):
            gd.untouched(name)
    # a LayerNorm fold wider than ops.LN_FOLD_MAX_K
    assert ops.LN_FOLD_MAX_K == 1024
    A, Wf = torch.zeros(70, 1088, dtype=F16, device=DEV), torch.zeros(64, 1088, dtype=F16, device=DEV)
    fo = rows_in([70], 64, F16, pad=8)
    with pytest.raises(ValueError, match="1024"):
        ops.linear(A, Wf, fo.views[0], torch.zeros(64, device=DEV), ln=(torch.ones(17, 70, 2, device=DEV), torch.zeros(64, device=DEV), 1e-6))
    fo.untouched("ln fold K = 1088")


def test_zz_worst_ratios_of_this_file():
    """not a check of its own: prints the largest error / bound every kernel reached above (all <= 1 or their tests failed)"""
    for kname in sorted(WORST):
        print(f"[elementwise] {kname}: worst error/bound {WORST[kname]:.3f}")
    assert all(v <= 1.0 for v in WORST.values())
