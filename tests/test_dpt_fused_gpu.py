"""GPU: the DPT output stage in the epilogue of head.2 (cut3r_conv3x3_dpt_final / ops.conv3x3_dpt_final).

The fused launch must give the BITS of conv3x3_nhwc(act = ReLU) followed by dpt_final(mode 0).  That is derived, not measured: a row of the
convolution is the same bits in every tile kernel (one MFMA, one K order), both paths round bias + ReLU to fp16 in the same way, and the
final 1x1 convolution with the activations is one device function (csrc/dpt_tail.h) whose rounding does not depend on the translation
unit that inlines it.  So every comparison of the two paths here is torch.equal.
"""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cut3r_slam_amd import _lib, ops  # noqa: E402
from oracle import cut3r_oracle as O  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")
F16, F32 = torch.float16, torch.float32
CH = 128


def _problem(B, H, W, seed, cout=CH):
    """random fp16 input and weights; the input is scaled per image column (log-uniform over 1e-3 .. 1) and the fp32 final weights are
    scaled so that d = |xyz| runs from about 1e-3 (expm1 near 0, the 1e-8 clamp far away) to about 5 (expm1 ~ 150) across a row"""
    g = torch.Generator().manual_seed(seed)
    col = torch.logspace(-3, 0, W).view(1, 1, W, 1)
    x = (torch.randn(B, H, W, CH, generator=g) * col).half()
    Wk = (torch.randn(cout, 9 * CH, generator=g) / (9 * CH) ** 0.5).half()
    bias = torch.randn(cout, generator=g) * 1e-4
    fw = torch.randn(4, CH, generator=g) * 0.35
    fb = torch.randn(4, generator=g) * 1e-4
    return [t.to(DEV) for t in (x, Wk, bias, fw, fb)]


def _unfused(x, Wk, bias, fw, fb, tile=0):
    B, H, W, _ = x.shape
    o = torch.empty(B, H, W, CH, dtype=F16, device=DEV)
    ops.conv3x3_nhwc(x, Wk, o, bias, act=2, tile=tile)
    pts, conf = torch.empty(B, H, W, 3, device=DEV), torch.empty(B, H, W, device=DEV)
    ops.dpt_final(o.view(B * H * W, CH), fw, fb, 0, pts, conf)
    return pts, conf, o


# one 192-pixel tile exactly | a ragged second tile that spans the view boundary and image rows | several tiles and bands
SHAPES = [(1, 6, 32), (2, 10, 14), (3, 16, 24)]


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_fused_equals_unfused_bit_for_bit(B, H, W):
    x, Wk, bias, fw, fb = _problem(B, H, W, 100 + H)
    pts_u, conf_u, o = _unfused(x, Wk, bias, fw, fb)
    pts_f, conf_f = torch.full((B, H, W, 3), float("nan"), device=DEV), torch.full((B, H, W), float("nan"), device=DEV)
    ops.conv3x3_dpt_final(x, Wk, bias, fw, fb, pts_f, conf_f)
    torch.cuda.synchronize()
    d = torch.log1p(pts_u.double().norm(dim=-1))
    print(f"[dpt fused] {B}x{H}x{W}: d in [{float(d.min()):.2e}, {float(d.max()):.2e}], conf in [{float(conf_u.min()):.3f}, {float(conf_u.max()):.3f}], "
          f"pts differ at {int((pts_f != pts_u).sum())} / {pts_u.numel()}, conf at {int((conf_f != conf_u).sum())} / {conf_u.numel()}")
    assert float(d.min()) < 1e-2 and float(d.max()) > 2.0, "the inputs must exercise expm1 and the division over a range of d"
    assert bool(torch.isfinite(pts_u).all()) and bool(torch.isfinite(conf_u).all())
    assert torch.equal(pts_f, pts_u)
    assert torch.equal(conf_f, conf_u)
    # the unfused convolution on the fused launch's own tile: the same bits again (rows do not depend on the tile)
    pts_t, conf_t, o_t = _unfused(x, Wk, bias, fw, fb, tile=192128)
    torch.cuda.synchronize()
    assert torch.equal(o_t, o) and torch.equal(pts_t, pts_f) and torch.equal(conf_t, conf_f)


def test_fused_into_strided_destination_leaves_the_other_slices_alone():
    B, H, W = SHAPES[1]
    x, Wk, bias, fw, fb = _problem(B, H, W, 100 + H)
    pts_u, conf_u, _ = _unfused(x, Wk, bias, fw, fb)
    big_p = torch.full((B, 3, H, W, 3), -7.0, device=DEV)
    big_c = torch.full((B, 3, H, W), -7.0, device=DEV)
    ops.conv3x3_dpt_final(x, Wk, bias, fw, fb, big_p[:, 1], big_c[:, 1])
    torch.cuda.synchronize()
    assert torch.equal(big_p[:, 1], pts_u) and torch.equal(big_c[:, 1], conf_u)
    for s in (0, 2):
        assert bool((big_p[:, s] == -7.0).all()) and bool((big_c[:, s] == -7.0).all()), s


def _torch_dpt_final(x, w, b):
    raw = x.float() @ w.t() + b
    return O.reg_dense_depth_exp(raw[:, :3]), 1 + raw[:, 3].exp()


def test_dpt_final_is_unchanged():
    """cut3r_dpt_final after its tail moved into the shared function: against a torch restatement at the tolerance of
    test_kernels_gpu.test_output_activations (1e-5 of the output scale), for the coalesced kernel (Cin = 128, 32) and for the per-lane kernel
    (Cin = 24: 3 lanes per pixel do not divide a wave).  The two kernels sum the channels in different orders and agree as before: both lie
    within 1e-5 of the restatement, hence within 2e-5 of each other (the same rows, zero-padded from 24 to 32 channels)."""
    g = torch.Generator().manual_seed(9)
    P = 1031
    for Cin in (128, 24):
        x = torch.randn(P, Cin, generator=g).half()
        w = torch.randn(4, Cin, generator=g) * 0.05
        b = torch.randn(4, generator=g) * 0.1
        pts, conf = torch.empty(P, 3, device=DEV), torch.empty(P, device=DEV)
        ops.dpt_final(x.to(DEV), w.to(DEV), b.to(DEV), 0, pts, conf)
        torch.cuda.synchronize()
        rp, rc = _torch_dpt_final(x, w, b)
        for name, got, ref in (("pts", pts.cpu(), rp), ("conf", conf.cpu(), rc)):
            err = float((got.double() - ref.double()).abs().max() / ref.double().abs().max())
            print(f"[dpt_final] Cin={Cin} {name}: rel err {err:.2e}")
            assert err <= 1e-5, (Cin, name, err)
    x32, w32 = torch.zeros(P, 32, dtype=F16), torch.zeros(4, 32)
    x32[:, :24], w32[:, :24] = x, w
    pts2, conf2 = torch.empty(P, 3, device=DEV), torch.empty(P, device=DEV)
    ops.dpt_final(x32.to(DEV), w32.to(DEV), b.to(DEV), 0, pts2, conf2)
    torch.cuda.synchronize()
    for name, a, c in (("pts", pts, pts2), ("conf", conf, conf2)):
        err = float((a.double() - c.double()).abs().max() / c.double().abs().max())
        print(f"[dpt_final] per-lane (Cin 24) vs coalesced (Cin 32, zero-padded) {name}: rel err {err:.2e}")
        assert err <= 2e-5, (name, err)


def test_dpt_final_gives_the_recorded_bits():
    """the points and the confidence that cut3r_dpt_final gave BEFORE its tail became the shared function (recorded on an MI355X from the
    commit before this one: tests/golden/dpt_final_bits.npz), for the coalesced and for the per-lane kernel: equal, bit for bit"""
    f = np.load(os.path.join(GOLD, "dpt_final_bits.npz"))
    for tag in ("c128", "c24"):
        x, w, b = (torch.from_numpy(f[f"{tag}_{k}"]).to(DEV) for k in ("x", "w", "b"))
        P = x.shape[0]
        pts, conf = torch.empty(P, 3, device=DEV), torch.empty(P, device=DEV)
        ops.dpt_final(x, w, b, 0, pts, conf)
        torch.cuda.synchronize()
        assert np.array_equal(pts.cpu().numpy().view(np.uint32), f[f"{tag}_pts"].view(np.uint32)), tag
        assert np.array_equal(conf.cpu().numpy().view(np.uint32), f[f"{tag}_conf"].view(np.uint32)), tag


def _desc(x, Wk, bias, stride=1, out_f16=1, res1=None):
    B, H, W, Cin = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    d = _lib.GemmDesc()
    d.A, d.B, d.bias = x.data_ptr(), Wk.data_ptr(), bias.data_ptr()
    d.act, d.out_f16, d.batch = 2, out_f16, 1
    d.M, d.N, d.K, d.lda, d.ldb, d.ldc = B * Ho * Wo, Wk.shape[0], 9 * Cin, Cin, 9 * Cin, Wk.shape[0]
    d.conv_k, d.H, d.W, d.Cin, d.conv_stride, d.Ho, d.Wo = 3, H, W, Cin, stride, Ho, Wo
    if res1 is not None:
        d.res1, d.ldr1, d.res1_f16 = res1.data_ptr(), Wk.shape[0], 1
    return d


def test_refusals_leave_the_outputs_alone():
    """N = 256, stride 2, a residual, an fp32 convolution output, mode 1, a misaligned destination: CUT3R_ERR_ARG (1) before any launch,
    the sentinel-filled points and confidence untouched.  The same call with none of these is accepted (so the refusals are the rules')."""
    lib = _lib.load()
    B, H, W = 1, 6, 32
    x, Wk, bias, fw, fb = _problem(B, H, W, 3)
    _, Wk256, bias256, _, _ = _problem(B, H, W, 4, cout=256)
    res = torch.zeros(B, H, W, CH, dtype=F16, device=DEV)
    pts, conf = torch.full((B * H * W * 3 + 4,), -7.0, device=DEV), torch.full((B * H * W + 4,), -7.0, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(d, mode=0, pts_off=0, conf_off=0):
        return lib.cut3r_conv3x3_dpt_final(C.byref(d), C.c_void_p(fw.data_ptr()), C.c_void_p(fb.data_ptr()), mode, C.c_void_p(pts.data_ptr() + pts_off),
                                           H * W * 3, C.c_void_p(conf.data_ptr() + conf_off), H * W, stream)

    cases = {"N = 256": lambda: call(_desc(x, Wk256, bias256)), "stride 2": lambda: call(_desc(x, Wk, bias, stride=2)),
             "residual": lambda: call(_desc(x, Wk, bias, res1=res)), "fp32 output": lambda: call(_desc(x, Wk, bias, out_f16=0)),
             "mode 1": lambda: call(_desc(x, Wk, bias), mode=1), "misaligned points": lambda: call(_desc(x, Wk, bias), pts_off=2),
             "misaligned confidence": lambda: call(_desc(x, Wk, bias), conf_off=2)}
    for name, fn in cases.items():
        rc = fn()
        torch.cuda.synchronize()
        assert rc == 1, (name, rc)
        assert bool((pts == -7.0).all()) and bool((conf == -7.0).all()), name
    # ops.conv3x3_dpt_final refuses on the host what it can see there
    with pytest.raises(ValueError):
        ops.conv3x3_dpt_final(x, Wk256, bias256, fw, fb, pts[:B * H * W * 3].view(B, H, W, 3), conf[:B * H * W].view(B, H, W))
    assert bool((pts == -7.0).all()) and bool((conf == -7.0).all())
    assert call(_desc(x, Wk, bias)) == 0
    torch.cuda.synchronize()
    assert bool((pts[:B * H * W * 3] != -7.0).all()) and bool((pts[B * H * W * 3:] == -7.0).all()) and bool((conf[B * H * W:] == -7.0).all())


CHILD_TIMEOUT = 120


def test_model_fused_equals_unfused_on_the_forked_and_the_batched_head_path(tmp_path):
    """Cut3rModel.forward_window at 64 x 96 (the medium config of test_model_gpu) with CUT3R_DPT_FUSE=1 (this process, the default) against
    CUT3R_DPT_FUSE=0 (a fresh child process: the model reads the switch when it is built): pts3d_in_self_view and conf_self, bit for bit,
    on the forked head path (captured graph: every view's head runs beside the next view's decoder and writes its slice of the window's
    output in place) and on the batched path (no graph: all views through the head at the end)."""
    from tests import dpt_fused_child as child
    t0 = time.time()
    mine = child.run(expect_fused=True)
    print(f"[dpt fused] model, both paths, in process: {time.time() - t0:.1f} s")
    path = str(tmp_path / "unfused.pt")
    env = dict(os.environ)
    env["CUT3R_DPT_FUSE"] = "0"
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, "-m", "tests.dpt_fused_child", path], cwd=ROOT, env=env, timeout=CHILD_TIMEOUT, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        pytest.fail(f"the CUT3R_DPT_FUSE=0 child was killed at its time limit of {CHILD_TIMEOUT} s; its output:\n{out[-4000:]}")
    assert r.returncode == 0, f"the CUT3R_DPT_FUSE=0 child exited {r.returncode}; its output:\n{r.stdout[-4000:]}"
    print(f"[dpt fused] child: {r.stdout.strip().splitlines()[-1]} ({time.time() - t0:.1f} s)")
    other = torch.load(path)
    assert set(other) == set(mine)
    for k in sorted(mine):
        assert torch.equal(mine[k], other[k]), k
