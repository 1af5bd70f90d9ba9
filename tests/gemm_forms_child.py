"""Checks of the pair, batched, two-residual and tuning-variant GEMM launches (tests/test_gemm_forms_gpu.py), written so that a compact
subset also runs in a FRESH process: `python -m tests.gemm_forms_child GOLDEN.pt` -- the environment switches of gemm.hip
(CUT3R_GEMM_FASTADDR, CUT3R_GEMM_EPI, CUT3R_GEMM64_STAGES) are latched into function-local statics on first use, so only a new process sees
them.  Not collected by pytest.  Exit status 0: every case held; 1: the failing case is printed.

Every runner makes three checks on each output:
  (a) bits       torch.equal with ops.linear of that problem alone at tile 128 and the default stages (tile 16 for the skinny kernel, whose
                 K order differs by design; the convolution at tile 128 for convolutions);
  (b) value      against a float64 CPU evaluation on the same fp16-rounded operands: 2e-3 of the output scale for fp16 outputs, 2e-5 for fp32
                 (the bounds of test_gemm_bias_gelu_residual);
  (c) footprint  the output is a view inside a larger buffer (guard rows above and below, guard columns to the right, where the entry point
                 accepts a row stride); the guards are filled with a sentinel, the payload with NaN; afterwards the payload is finite and
                 every guard element holds the sentinel's bits.
"""
import contextlib
import sys

import numpy as np
import torch
import torch.nn.functional as F

from cut3r_slam_amd import ops

DEV = "cuda:0"
F16, F32 = torch.float16, torch.float32
SENT = -1111.0                      # exact in fp16 and fp32
TOL = {F16: 2e-3, F32: 2e-5}        # tests/test_kernels_gpu.py::test_gemm_bias_gelu_residual


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def _report(name, got, ref, tol):
    err = _rel(got, ref)
    if not err <= tol:
        d = (got.double().cpu() - ref.double().cpu()).abs()
        idx = np.unravel_index(int(d.argmax()), d.shape)
        nbad = int((d > tol * ref.double().abs().max()).sum())
        raise AssertionError(f"{name}: rel err {err:.3e} > {tol:.1e}; worst at {idx}: got {got.cpu()[idx].item():.6f} "
                             f"ref {ref.cpu()[idx].item():.6f}; {nbad}/{d.numel()} elements out of tolerance; "
                             f"nan={bool(torch.isnan(got).any())}")


def _bits(t):
    return t.view(torch.int16 if t.dtype == F16 else torch.int32)


class Guard:
    """a sentinel-filled buffer and the payload views inside it"""

    def __init__(self, buf, views, nan=True):
        assert buf.storage_offset() == 0
        self.buf, self.views = buf, views
        if nan:
            for v in views:
                v.fill_(float("nan"))

    def check(self, name):
        torch.cuda.synchronize()
        for i, v in enumerate(self.views):
            assert bool(torch.isfinite(v).all()), f"{name}: payload {i} has {int((~torch.isfinite(v)).sum())} elements that were never written"
        c = self.buf.clone()
        for v in self.views:
            torch.as_strided(c, v.size(), v.stride(), v.storage_offset()).fill_(SENT)
        bad = _bits(c) != _bits(torch.full((1,), SENT, dtype=c.dtype, device=c.device))
        if bool(bad.any()):
            where = bad.nonzero()[:4].tolist()
            raise AssertionError(f"{name}: {int(bad.sum())} guard elements overwritten, first at {where} of a {tuple(c.shape)} buffer")

    def untouched(self, name):
        """after a refused launch: guards AND payload as they were (the payload was filled with NaN)"""
        torch.cuda.synchronize()
        for v in self.views:
            assert bool(torch.isnan(v).all()), f"{name}: a refused launch wrote to its output"
            v.fill_(SENT)
        self.check(name)
        for v in self.views:
            v.fill_(float("nan"))


def rows_in(rows, N, dtype, pad=8, nan=True):
    """views of rows[i] x N, one after the other, in ONE [*, N + pad] buffer: a guard row on top, the next problem's rows directly below
    the previous one's where the 16-byte alignment of its first row allows (else the fewest guard rows that restore it), guard rows below"""
    ld, q = N + pad, 8 if dtype == F16 else 4
    starts, r = [], 1
    for m in rows:
        while (r * ld) % q:
            r += 1
        starts.append(r)
        r += m
    buf = torch.full((r + 2, ld), SENT, dtype=dtype, device=DEV)
    return Guard(buf, [buf[s:s + m, :N] for s, m in zip(starts, rows)], nan)


def batch_in(Z, M, N, dtype, pad=8, odd=False, nan=True):
    """[Z, M, N] view inside [Z + 1, top + M + bottom, N + pad]: guard rows above (as many as keep the first row 16-byte aligned) and below
    every batch, one whole guard batch at the end; odd: an odd number of rows per batch"""
    ld, q, top, bottom = N + pad, 8 if dtype == F16 else 4, 1, 1
    while (top * ld) % q:
        top += 1
    if odd and (top + M + bottom) % 2 == 0:
        bottom = 2
    buf = torch.full((Z + 1, top + M + bottom, ld), SENT, dtype=dtype, device=DEV)
    return Guard(buf, [buf[:Z, top:top + M, :N]], nan)


@contextlib.contextmanager
def default_stages():
    """the bit reference is always made by the default kernel of tile 128, whatever stages variant is under test"""
    keep = ops.GEMM_STAGES
    ops.GEMM_STAGES = 0
    try:
        yield
    finally:
        ops.GEMM_STAGES = keep


def operands(M, N, K, seed, bias=True, res=(), Z=None):
    """fp16-rounded A [M,K], W [N,K], fp32 bias [N] and residuals of the given dtypes, on the CPU ([Z, ...] with Z)"""
    g = torch.Generator().manual_seed(seed)
    z = () if Z is None else (Z,)
    A = torch.randn(*z, M, K, generator=g).half()
    W = (torch.randn(*z, N, K, generator=g) / K ** 0.5).half()
    b = torch.randn(*z, N, generator=g) if bias else None
    rs = [torch.randn(*z, M, N, generator=g).to(dt) for dt in res]
    return A, W, b, rs


def ref64(A, W, b, act, res):
    y = A.double() @ W.double().transpose(-1, -2)
    if b is not None:
        y = y + b.double().unsqueeze(-2)
    if act == 1:
        y = F.gelu(y)
    elif act == 2:
        y = F.relu(y)
    for r in res:
        y = y + r.double()
    return y


def single_ref(A, W, b, act, res, odt, tile=128):
    """(a)'s reference: the problem alone, contiguous, at tile 128 with the default stages"""
    M, N = A.shape[0], W.shape[0]
    out = torch.zeros(M, N, dtype=odt, device=DEV)
    with default_stages():
        ops.linear(A, W, out, b, act, *(r.clone() for r in res), tile=tile)
    torch.cuda.synchronize()
    return out


def strided_copy(t, pad):
    """t [M, N] on the GPU as a view with row stride N + pad, one row into its buffer"""
    M, N = t.shape
    buf = torch.zeros(M + 2, N + pad, dtype=t.dtype, device=DEV)
    buf[1:1 + M, :N] = t
    return buf[1:1 + M, :N]


# ------------------------------------------------------------------------------------------------ pair launches
# epilogue of a pair: (act, problem 0, problem 1), a problem = (output dtype, bias?, residual: None | "inplace" | "f32" | "f16", pad of the
# output's row stride, pad of the residual's row stride)
PAIR_EPI = {
    "bias":      (0, (F16, True, None, 8, 0), (F16, True, None, 8, 0)),                     # compile-time epilogue 1 on the 64 tile
    "gelu":      (1, (F16, True, None, 8, 0), (F16, True, None, 8, 0)),                     # 2
    "res32":     (0, (F32, True, "inplace", 8, 0), (F32, True, "inplace", 8, 0)),           # 3: attn.proj / fc2, out is res1
    # mixed pairs: the run-time epilogue
    "bias_one":  (0, (F16, True, None, 8, 0), (F16, False, None, 8, 0)),
    "out_mixed": (0, (F16, True, None, 8, 0), (F32, True, None, 8, 0)),
    "res_one":   (0, (F32, True, "inplace", 8, 0), (F32, True, None, 8, 0)),
    "res16":     (0, (F16, True, "f16", 8, 8), (F16, True, "f16", 8, 8)),
    # row strides of 4 mod 8 elements on ONE side (gemm256_epi_mode 0 for that side only); the first row stays 16-byte aligned
    "ldc_one":   (0, (F16, True, None, 8, 0), (F16, True, None, 4, 0)),
    "ldr_one":   (0, (F16, True, "f16", 8, 4), (F16, True, "f16", 8, 8)),
    "gelu_ldc":  (1, (F16, True, None, 12, 0), (F16, True, None, 8, 0)),
}


def run_pair(M0, M1, N, K, tile, epi, seed=0):
    """ops.linear_pair on two problems of M0 and M1 rows -> the two outputs (CPU)"""
    act, s0, s1 = PAIR_EPI[epi]
    name = f"pair M={M0}+{M1} N={N} K={K} tile={tile} {epi}"
    probs = []
    for i, (M, (odt, bias, res, _, rpad)) in enumerate(((M0, s0), (M1, s1))):
        A, W, b, rs = operands(M, N, K, 1000 * seed + 17 * M + N + K + i, bias, () if res is None else (F16 if res == "f16" else F32,))
        probs.append(dict(A=A, W=W, b=b, rs=rs, odt=odt, res=res, rpad=rpad))
    same = s0[0] == s1[0] and s0[3] == s1[3]
    if same:                            # back to back in one buffer: an overrun of problem 0 lands in problem 1
        gd = [rows_in([M0, M1], N, s0[0], s0[3])]
        outs = gd[0].views
    else:
        gd = [rows_in([M0], N, s0[0], s0[3]), rows_in([M1], N, s1[0], s1[3])]
        outs = [gd[0].views[0], gd[1].views[0]]
    args = []
    for p, out in zip(probs, outs):
        p["dA"], p["dW"] = p["A"].to(DEV), p["W"].to(DEV)
        p["db"] = p["b"].to(DEV) if p["b"] is not None else None
        p["dr"] = [r.to(DEV) for r in p["rs"]]
        r1 = None
        if p["res"] == "inplace":
            out.copy_(p["dr"][0])
            r1 = out
        elif p["res"] is not None:
            r1 = strided_copy(p["dr"][0], p["rpad"]) if p["rpad"] else p["dr"][0]
        args.append((p["dA"], p["dW"], out, p["db"], r1))
    ops.linear_pair(args[0], args[1], act=act, tile=tile)
    got = []
    for g_ in gd:
        g_.check(name)
    for i, (p, out) in enumerate(zip(probs, outs)):
        ref = single_ref(p["dA"], p["dW"], p["db"], act, p["dr"], p["odt"])
        assert torch.equal(out, ref), f"{name}: problem {i} differs from ops.linear at tile 128 in {int((out != ref).sum())} elements"
        _report(f"{name} problem {i}", out.float(), ref64(p["A"], p["W"], p["b"], act, p["rs"]), TOL[p["odt"]])
        got.append(out.cpu().clone())
    return got


# ------------------------------------------------------------------------------------------------ batched launches
def run_batched(Z, M, N, K, tile, odt, layout, bias=True, res=None, act=0, seed=0):
    """ops.linear_batched.  layout: "contig" (contiguous operands, sC = (M + 2)(N + 8)), "embed" (decoder_embed: A = feat[:, i] of
    [Z, V, M, K], out = a3[:, 1:] of [Z, M + 1, N]) or "odd" (batch strides off the vector alignment the compile-time epilogues need:
    sC = 4 mod 8 elements for fp16 outputs, sBias = 2 mod 4, sR1 = 4 mod 8 for fp16 residuals)"""
    name = f"batched Z={Z} M={M} N={N} K={K} tile={tile} {odt} {layout} bias={bias} res={res} act={act}"
    A, W, b, rs = operands(M, N, K, 2000 * seed + 31 * M + N + K + Z, bias, () if res is None else (res,), Z=Z)
    dW = W.to(DEV)
    db = dr = None
    if layout == "embed":
        feat = torch.zeros(Z, 3, M, K, dtype=F16, device=DEV)
        feat[:, 1] = A.to(DEV)
        dA = feat[:, 1]
        buf = torch.full((Z + 1, M + 1, N), SENT, dtype=odt, device=DEV)
        gd = Guard(buf, [buf[:Z, 1:]])
    else:
        dA = A.to(DEV)
        gd = batch_in(Z, M, N, odt, *((4, True) if layout == "odd" else (8, False)))      # odd: row stride N + 4, an odd row count per batch
    out = gd.views[0]
    if layout == "odd" and odt == F16:
        assert out.stride(0) % 8 == 4
    if bias:
        if layout == "odd":
            bb = torch.zeros(Z, N + 2, device=DEV)
            bb[:, :N] = b.to(DEV)
            db = bb[:, :N]
        else:
            db = b.to(DEV)
    if res is not None:
        if layout == "odd":
            assert res == F32 or (N % 8 == 0)
            rb = torch.zeros(Z, M + (3 if M % 2 == 0 else 4), N + 4, dtype=res, device=DEV)
            rb[:, 2:2 + M, :N] = rs[0].to(DEV)
            dr = rb[:, 2:2 + M, :N]
            assert res == F32 or dr.stride(0) % 8 == 4
        else:
            dr = rs[0].to(DEV)
    ops.linear_batched(dA, dW, out, db, act, dr, tile=tile)
    gd.check(name)
    y = ref64(A, W, b, act, rs)
    for z in range(Z):
        ref = single_ref(dA[z].contiguous(), dW[z], None if db is None else db[z].clone(), act, [] if dr is None else [dr[z].contiguous()], odt,
                         tile=16 if tile == 16 else 128)
        assert torch.equal(out[z], ref), f"{name}: z={z} differs from ops.linear alone in {int((out[z] != ref).sum())} elements"
    _report(name, out.float(), y, TOL[odt])
    return [out.cpu().clone()]


# ------------------------------------------------------------------------------------------------ one problem (stages variants, two residuals)
def run_single(M, N, K, tile, odt, act=0, res=(), inplace=False, seed=0):
    """ops.linear on one guarded output with the current ops.GEMM_STAGES; res: dtypes of res1 (and res2)"""
    name = f"linear M={M} N={N} K={K} tile={tile} stages={ops.GEMM_STAGES} {odt} act={act} res={res} inplace={inplace}"
    A, W, b, rs = operands(M, N, K, 3000 * seed + 13 * M + N + K, True, res)
    dA, dW, db, dr = A.to(DEV), W.to(DEV), b.to(DEV), [r.to(DEV) for r in rs]
    gd = rows_in([M], N, odt)
    out = gd.views[0]
    rin = list(dr)
    if inplace:
        out.copy_(dr[0])
        rin[0] = out
    ops.linear(dA, dW, out, db, act, *rin, tile=tile)
    gd.check(name)
    ref = single_ref(dA, dW, db, act, dr, odt, tile=128 if tile != 128 or ops.GEMM_STAGES else 64)
    assert torch.equal(out, ref), f"{name}: differs from the default kernel in {int((out != ref).sum())} elements"
    _report(name, out.float(), ref64(A, W, b, act, rs), TOL[odt])
    return [out.cpu().clone()]


def run_conv(B, H, Wd, Cin, Cout, stride, relu_in, tile, res=(F16, F16), odt=F16, act=0, seed=0):
    """ops.conv3x3_nhwc with two residuals (the DPT fusion blocks' _rcu), or with none and an activation.  The entry point wants a contiguous output: guards of 64 elements
    in front of and behind it.  Bit reference: the same convolution at tile 128 (tile 64 for tile 128 itself)."""
    name = f"conv3x3 {B}x{H}x{Wd} {Cin}->{Cout} s{stride} relu_in={relu_in} tile={tile} res={res} {odt} act={act}"
    g = torch.Generator().manual_seed(4000 * seed + H * 31 + Wd + Cin)
    x = torch.randn(B, Cin, H, Wd, generator=g).half()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5).half()
    b = torch.randn(Cout, generator=g)
    xin = F.relu(x.double()) if relu_in else x.double()
    y = F.conv2d(xin, w.double(), b.double(), stride=stride, padding=1).permute(0, 2, 3, 1)
    if act:
        y = F.gelu(y) if act == 1 else F.relu(y)
    rs = [torch.randn(y.shape, generator=g).to(dt) for dt in res]
    for r in rs:
        y = y + r.double()
    dx = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    wk = w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous().to(DEV)
    db, dr = b.to(DEV), [r.to(DEV) for r in rs]
    n = y.numel()
    buf = torch.full((n + 128,), SENT, dtype=odt, device=DEV)
    gd = Guard(buf, [buf[64:64 + n].view(y.shape)])
    out = gd.views[0]
    ops.conv3x3_nhwc(dx, wk, out, db, stride, relu_in, act, *dr, tile=tile)
    gd.check(name)
    ref = torch.zeros(y.shape, dtype=odt, device=DEV)
    with default_stages():
        ops.conv3x3_nhwc(dx, wk, ref, db, stride, relu_in, act, *dr, tile=128 if tile != 128 else 64)
    torch.cuda.synchronize()
    assert torch.equal(out, ref), f"{name}: differs from the other tile kernel in {int((out != ref).sum())} elements"
    _report(name, out.float(), y, TOL[odt])
    return [out.cpu().clone()]


# ------------------------------------------------------------------------------------------------ the subset a fresh process repeats
# one or two cases per distinct kernel family that the switches re-route: the pair kernels of every tile (64: 4-wave and 8-wave, the three
# compile-time epilogues, the run-time one, a K tail), batched launches on both sides of the stride conditions, two residuals
SUBSET = [
    ("pair64_bias", run_pair, (769, 768, 768, 192, 64, "bias")),
    ("pair64_gelu", run_pair, (130, 1, 256, 768, 64, "gelu")),
    ("pair64_res32", run_pair, (449, 450, 256, 768, 64, "res32")),
    ("pair64_k3072", run_pair, (257, 130, 256, 3072, 64, "res32")),
    ("pair64_k3072_mixed", run_pair, (70, 257, 192, 3072, 64, "out_mixed")),
    ("pair64_ktail", run_pair, (200, 67, 168, 200, 64, "bias_one")),
    ("pair128", run_pair, (300, 257, 360, 768, 128, "res16")),
    ("pair192", run_pair, (385, 200, 360, 192, 192128, "gelu")),
    ("pair256", run_pair, (515, 300, 488, 768, 256, "res32")),
    ("pair256_ktail", run_pair, (300, 257, 512, 200, 256, "ldc_one")),
    ("pair0", run_pair, (768, 769, 768, 768, 0, "res32")),
    ("batched64", run_batched, (2, 197, 256, 768, 64, F16, "embed")),
    ("batched128_odd", run_batched, (2, 300, 264, 192, 128, F16, "odd", True, F16)),
    ("batched256", run_batched, (2, 300, 512, 768, 256, F32, "contig", True, F32)),
    ("batched192_odd", run_batched, (2, 200, 256, 200, 192128, F32, "odd", True, F32)),
    # the single-problem 64 x 64 kernels whose ring depth CUT3R_GEMM64_STAGES sets: epilogues 1 (batched64 above), 2, 3, run-time; 8 waves
    ("single64_gelu", run_single, (130, 128, 768, 64, F16, 1)),
    ("single64_res32", run_single, (130, 128, 768, 64, F32, 0, (F32,), True)),
    ("single64_k3072", run_single, (130, 128, 3072, 64, F32, 0, (F32,), True)),
    ("batched64_k2048", run_batched, (2, 70, 64, 2048, 64, F32, "contig", True, F32)),
    ("res2_256", run_single, (300, 264, 192, 256, F16, 0, (F16, F16))),
    ("res2_64", run_single, (130, 128, 768, 64, F32, 0, (F32, F16))),
    ("conv256", run_conv, (1, 12, 16, 128, 256, 1, True, 256)),
    ("conv192_cin96", run_conv, (2, 9, 9, 96, 128, 2, False, 192128)),
]


def run_subset(golden=None):
    """every SUBSET case with its three checks -> {name: outputs}; with `golden` (the parent's outputs under the default settings) the
    outputs must also equal those bit for bit: the epilogue arithmetic does not depend on its compile-time / run-time form"""
    got = {}
    for name, fn, a in SUBSET:
        try:
            got[name] = fn(*a)
            if golden is not None:
                for i, (o, r) in enumerate(zip(got[name], golden[name])):
                    assert torch.equal(o, r), f"output {i} differs from the default-settings result in {int((o != r).sum())} elements"
        except Exception as e:
            raise AssertionError(f"subset case {name} {a}: {e}") from e
    return got


def main(argv):
    import os
    golden = torch.load(argv[1]) if len(argv) > 1 else None
    sw = {k: v for k, v in os.environ.items() if k.startswith("CUT3R_GEMM")}
    try:
        run_subset(golden)
    except AssertionError as e:
        print(f"FAILED under {sw}: {e}", flush=True)
        return 1
    print(f"ok: {len(SUBSET)} cases under {sw}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
