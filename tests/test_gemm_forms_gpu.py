"""GPU: every launch form of gemm.hip that tests/test_kernels_gpu.py and tests/test_lnfold_gpu.py do not reach -- the pair launches
(cut3r_gemm_f16_pair / ops.linear_pair: gemm256_pair_kernel, gemm_pair_kernel of the 128 x 128, 192 x 128 and 64 x 64 tiles with 4 and 8
waves, the LayerNorm fold and the fused RoPE in pair form, the split of the grid between the two problems), batched launches
(ops.linear_batched: batch strides on either side of the conditions that select a compile-time epilogue), two residuals (ops.linear and
ops.conv3x3_nhwc), and the tuning variants (`stages`, and in a fresh process the environment-latched switches).

Each case makes the three checks described in tests/gemm_forms_child.py: (a) the bits of ops.linear on that problem alone at tile 128,
(b) the value of a float64 CPU evaluation within 2e-3 (fp16 outputs) / 2e-5 (fp32) of the output scale, (c) nothing written outside the
output (sentinel guards around a NaN payload).

ops.linear_pair writes `tile` into both descriptors; cut3r_gemm_f16_pair reads the first one's only (both problems run one kernel)."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np  # noqa: F401
import pytest
import torch
import torch.nn.functional as F  # noqa: F401

pytestmark = pytest.mark.gpu

from cut3r_slam_amd import _lib, ops  # noqa: E402
from tests import gemm_forms_child as GF  # noqa: E402
from tests.gemm_forms_child import DEV, F16, F32, TOL, _report  # noqa: E402
from tests.test_lnfold_gpu import EPS, _folded_setup, _produce, _rows  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))



def _run_all(fn, cases):
    """every case of one tile in ONE test (the per-test set-up / tear-down of this suite costs more than a case does); all failing cases
    are reported, each with its shape, not only the first"""
    bad = []
    for c in cases:
        try:
            fn(*c)
        except (AssertionError, ValueError, _lib.Cut3rHipError) as e:
            bad.append(f"{c}: {e}")
    assert not bad, f"{len(bad)} of {len(cases)} cases failed:\n" + "\n".join(bad)


# ------------------------------------------------------------------------------------------------ 1. pair launches
BLOCK = {64: (64, 64), 128: (128, 128), 192128: (192, 128), 256: (256, 256)}
# (row tiles of problem 0, ragged?, row tiles of problem 1, ragged?, column tiles, columns short of whole tiles); 0 row tiles: ONE row.
# tiles per problem = row tiles x column tiles: 1, 7, 8, 9 and 69 among them; each problem has its own XCD-aware order (swz = 1)
SPLITS = [
    (2, 0, 3, 0, 2, 0),        # both whole
    (2, 1, 2, 0, 2, 24),       # ragged last row tile in problem 0 only (and a ragged column tile)
    (2, 0, 2, 1, 2, 0),        # in problem 1 only
    (3, 1, 2, 1, 3, 28),       # in both; N = 4 mod 8: no compile-time epilogue
    (0, 0, 9, 0, 1, 0),        # one row (1 tile) in front of 9 tiles
    (9, 1, 0, 0, 2, 0),        # 18 tiles in front of one row (2 tiles)
    (7, 0, 8, 1, 1, 0),        # 7 and 8 tiles
    (23, 1, 1, 0, 3, 0),       # 69 tiles (> 64, not a multiple of 8) in front of 3
]
SPLIT_K = [192, 768, 200, 3072, 768, 192, 3072, 192]      # 200: a K tail inside a 64-deep tile (generic addressing); 3072: the 8-wave 64 x 64 kernels
SPLIT_EPI = {
    # tile 64 has compile-time epilogues 1 / 2 / 3 (4 waves) and 3 (8 waves) when BOTH sides qualify, else the run-time one
    64: ["bias", "gelu", "bias_one", "res32", "res32", "ldc_one", "out_mixed", "res16"],
    128: ["res32", "bias_one", "gelu", "res16", "out_mixed", "res_one", "bias", "ldr_one"],
    192128: ["gelu", "res32", "res16", "bias", "ldc_one", "out_mixed", "res_one", "bias_one"],
    256: ["res16", "out_mixed", "res32", "gelu", "bias_one", "gelu_ldc", "ldr_one", "res32"],
}


def _rows_of(mt, rag, bm):
    return 1 if mt == 0 else (mt - 1) * bm + (5 + mt if rag else bm)


def _pair_cases():
    cases = []
    for tile, (bm, bn) in BLOCK.items():
        for i, (t0, r0, t1, r1, npn, short) in enumerate(SPLITS):
            cases.append((_rows_of(t0, r0, bm), _rows_of(t1, r1, bm), npn * bn - short, SPLIT_K[i], tile, SPLIT_EPI[tile][i]))
    cases += [
        # the remaining 64 x 64 pair kernels: 8 waves with generic addressing (K >= 2048 with a K tail), 4 waves with a K tail and a residual
        (130, 67, 128, 2056, 64, "gelu"), (67, 130, 136, 200, 64, "res_one"), (129, 64, 128, 192, 64, "ldr_one"), (64, 129, 192, 768, 64, "gelu_ldc"),
        # the production shapes (768 state rows and 769 image rows per window, x 4 windows) and the tile rule of cut3r_gemm_f16_pair for tile 0:
        # t256 = (ceil(M0 / 256) + ceil(M1 / 256)) ceil(N / 256), 256 if N % 256 == 0 and t256 >= 128 (and the last round >= 85 % full),
        # else t128 = (ceil(M0 / 128) + ceil(M1 / 128)) ceil(N / 128), 128 if t128 >= 128, else 64
        (3072, 3076, 1536, 768, 0, "res32"),        # t256 = 25 x 6 = 150, one round                                -> 256
        (3072, 3076, 768, 768, 0, "gelu"),          # t256 = 25 x 3 = 75;  t128 = 49 x 6 = 294                      -> 128
        (768, 769, 2304, 768, 0, "bias"),           # t256 = 7 x 9 = 63;   t128 = 13 x 18 = 234 (attn.qkv)          -> 128
        (3076, 3072, 1024, 1024, 0, "bias_one"),    # t256 = 25 x 4 = 100; t128 = 49 x 8 = 392                      -> 128
        (768, 769, 768, 768, 0, "res32"),           # t256 = 21;           t128 = 13 x 6 = 78 (attn.proj, 1 window) -> 64
        (768, 769, 1024, 1024, 0, "gelu"),          # t256 = 28;           t128 = 13 x 8 = 104                      -> 64
        (769, 768, 768, 3072, 0, "res32"),          # mlp.fc2 of one window: t128 = 78                              -> 64, 8 waves
        (3076, 3072, 768, 768, 256, "res32"), (769, 768, 1024, 1024, 128, "out_mixed"), (3072, 769, 768, 768, 192128, "res32"),
    ]
    return cases


@pytest.mark.parametrize("tile", [0, 64, 128, 192128, 256])
def test_pair_launch(tile):
    cases = [c for c in _pair_cases() if c[4] == tile]
    assert len(cases) >= 7
    _run_all(GF.run_pair, cases)


def _fold64(x16, st, Wf, d, c):
    """the folded consumer in float64: slab statistics (sum, m2) -> (mu, rstd) by Chan's combination, y = rstd (x16 Wf^T - mu c) + d"""
    K = x16.shape[1]
    s, m2 = st.double().cpu()[..., 0], st.double().cpu()[..., 1]            # [K/64, M]
    mu = s.sum(0) / K
    var = (m2.sum(0) + (64.0 * (s / 64.0 - mu) ** 2).sum(0)) / K
    rstd = 1.0 / torch.sqrt(var + EPS)
    acc = x16.double().cpu() @ Wf.double().T
    return rstd[:, None] * (acc - mu[:, None] * c.double()[None]) + d.double()[None]


def _consumer(M, K, N, seed):
    x, gamma, beta, W, b, Wf, d, c, _ = _folded_setup(M, K, N, seed)
    _, x16, st = _produce(x, 64)
    return dict(x16=x16, st=st, Wf=Wf, dWf=Wf.to(DEV), d=d, dd=d.to(DEV), c=c, dc=c.to(DEV))


@pytest.mark.parametrize("M0,M1,K,N,act", [(769, 768, 768, 1024, 1), (130, 67, 192, 128, 0)])
def test_pair_fold_consumer_on_both_sides(M0, M1, K, N, act):
    ps = [_consumer(M0, K, N, 11), _consumer(M1, K, N, 12)]
    gd = GF.rows_in([M0, M1], N, F16)
    ops.linear_pair(*[(p["x16"], p["dWf"], o, p["dd"], None, {"ln": (p["st"], p["dc"], EPS)}) for p, o in zip(ps, gd.views)], act=act, tile=64)
    gd.check("pair fold consumer")
    for i, (p, o) in enumerate(zip(ps, gd.views)):
        ref = torch.zeros_like(o, memory_format=torch.contiguous_format)
        ops.linear(p["x16"], p["dWf"], ref, p["dd"], act, tile=64, ln=(p["st"], p["dc"], EPS))
        torch.cuda.synchronize()
        assert torch.equal(o, ref), (i, int((o != ref).sum()))
        y = _fold64(p["x16"], p["st"], p["Wf"], p["d"], p["c"])
        _report(f"pair fold consumer {i}", o.float(), F.gelu(y) if act else y, TOL[F16])


def test_pair_fold_consumer_with_rope_beside_a_plain_problem():
    """the attn.qkv call: problem 0 a plain projection, problem 1 the folded consumer with 2-D RoPE (64-wide heads) on q | k.  Value check of
    the rotated columns: the float64 projection, rounded to fp16 as the fused epilogue rounds it, through the stand-alone rope_2d kernel."""
    M0, M1, K, N, cols = 768, 769, 768, 2304, 1536
    A, W, b, _ = GF.operands(M0, N, K, 5)
    p = _consumer(M1, K, N, 13)
    pos = torch.randint(-1, 33, (M1, 2), generator=torch.Generator().manual_seed(3), dtype=torch.int64).to(DEV)
    gd = GF.rows_in([M0, M1], N, F16)
    o0, o1 = gd.views
    extras = {"ln": (p["st"], p["dc"], EPS), "rope": (pos, cols, 100.0)}
    ops.linear_pair((A.to(DEV), W.to(DEV), o0, b.to(DEV), None), (p["x16"], p["dWf"], o1, p["dd"], None, extras), tile=64)
    gd.check("pair qkv")
    assert torch.equal(o0, GF.single_ref(A.to(DEV), W.to(DEV), b.to(DEV), 0, [], F16))
    _report("pair qkv, plain side", o0.float(), GF.ref64(A, W, b, 0, []), TOL[F16])
    ref = torch.zeros(M1, N, dtype=F16, device=DEV)
    ops.linear(p["x16"], p["dWf"], ref, p["dd"], 0, tile=64, **extras)
    torch.cuda.synchronize()
    assert torch.equal(o1, ref), int((o1 != ref).sum())
    y = _fold64(p["x16"], p["st"], p["Wf"], p["d"], p["c"])
    y16 = y.float().half().to(DEV)
    ops.rope_2d(y16.view(1, M1, N // 64, 64)[:, :, :cols // 64], pos.view(1, M1, 2), 100.0, 1.0)
    torch.cuda.synchronize()
    _report("pair qkv, folded + rotated side", o1.float(), y16.float(), TOL[F16])
    assert not torch.equal(o1[:, :cols].cpu(), y.float().half()[:, :cols])          # RoPE did something


@pytest.mark.parametrize("K", [768, 3072])
def test_pair_fold_producer_on_both_sides(K):
    """attn.proj / mlp.fc2: fp32 out = A W^T + b + out (in place) and, beside it, the fp16 copy and the slab statistics"""
    N, Ms = 768, (769, 200)
    gd, g16 = GF.rows_in(Ms, N, F32), GF.rows_in(Ms, N, F16)
    ps, args = [], []
    for i, M in enumerate(Ms):
        A, W, b, _ = GF.operands(M, N, K, 20 + i)
        x = _rows(M, N, 30 + i)
        st = torch.full((N // 64, M, 2), float("nan"), dtype=F32, device=DEV)
        gd.views[i].copy_(x)
        ps.append(dict(A=A, W=W, b=b, x=x, st=st))
        args.append((A.to(DEV), W.to(DEV), gd.views[i], b.to(DEV), gd.views[i], {"emit": (st, g16.views[i])}))
    ops.linear_pair(*args, tile=64)
    gd.check("pair producer, fp32 stream")
    g16.check("pair producer, fp16 copy")
    for i, (p, a) in enumerate(zip(ps, args)):
        M = Ms[i]
        out, o16, st = gd.views[i], g16.views[i], p["st"]
        ref, r16 = torch.zeros(M, N, dtype=F32, device=DEV), torch.zeros(M, N, dtype=F16, device=DEV)
        rst = torch.full((N // 64, M, 2), float("nan"), dtype=F32, device=DEV)
        ops.linear(a[0], a[1], ref, a[3], res1=p["x"].to(DEV), tile=64, emit=(rst, r16))
        torch.cuda.synchronize()
        assert torch.equal(out, ref) and torch.equal(o16, r16) and torch.equal(st, rst), i
        assert torch.equal(out, GF.single_ref(a[0], a[1], a[3], 0, [p["x"].to(DEV)], F32)), i          # and the plain tile-128 rows
        _report(f"pair producer {i}", out, GF.ref64(p["A"], p["W"], p["b"], 0, [p["x"]]), TOL[F32])
        assert torch.equal(o16, out.half())
        rows = out.double().cpu().view(M, N // 64, 64)
        s_ref, m2_ref = rows.sum(-1), ((rows - rows.mean(-1, keepdim=True)) ** 2).sum(-1)
        sd = st.double().cpu().permute(1, 0, 2)
        assert (sd[..., 0] - s_ref).abs().max() <= 2e-6 * rows.abs().sum(-1).max()         # bounds of test_producer_writes_the_fp16_copy_...
        assert ((sd[..., 1] - m2_ref).abs() / m2_ref).max() < 2e-5


def _refused(fn, guards):
    with pytest.raises((ValueError, _lib.Cut3rHipError)):
        fn()
    for g in guards:
        g.untouched("refused pair launch")


def test_pair_refusals_leave_the_outputs_alone():
    lib = _lib.load()
    M, N, K = 130, 128, 192
    A, W, b, _ = GF.operands(M, N, K, 1)
    A, W, b = A.to(DEV), W.to(DEV), b.to(DEV)
    W2, K2 = torch.zeros(N + 64, K, dtype=F16, device=DEV), torch.zeros(N, K + 64, dtype=F16, device=DEV)
    A2 = torch.zeros(M, K + 64, dtype=F16, device=DEV)
    p = _consumer(M, K, N, 14)
    pos = torch.zeros(M, 2, dtype=torch.int64, device=DEV)
    new = lambda n=N: GF.rows_in([M, M], n, F16)

    def raw(d0, d1):
        rc = lib.cut3r_gemm_f16_pair(C.byref(d0), C.byref(d1), ops._stream())
        assert rc == 1, rc
        raise ValueError("refused by cut3r_gemm_f16_pair")

    # different N, different K: by ops and by the C side
    g, g2 = new(), GF.rows_in([M], N + 64, F16)
    _refused(lambda: ops.linear_pair((A, W, g.views[0], b, None), (A, W2, g2.views[0], None, None)), [g, g2])
    _refused(lambda: raw(ops._linear_desc(A, W, g.views[0], b, 0, None, 64), ops._linear_desc(A, W2, g2.views[0], None, 0, None, 64)), [g, g2])
    g = new()
    _refused(lambda: ops.linear_pair((A, W, g.views[0], b, None), (A2, K2, g.views[1], b, None)), [g])
    _refused(lambda: raw(ops._linear_desc(A, W, g.views[0], b, 0, None, 64), ops._linear_desc(A2, K2, g.views[1], b, 0, None, 64)), [g])
    # LayerNorm fold / fused RoPE ride the 64 x 64 pair kernels only
    for tile in (128, 256, 192128):
        g = new()
        _refused(lambda: ops.linear_pair((A, W, g.views[0], b, None), (p["x16"], p["dWf"], g.views[1], p["dd"], None, {"ln": (p["st"], p["dc"], EPS)}),
                                         tile=tile), [g])
        _refused(lambda: ops.linear_pair((A, W, g.views[0], b, None, {"rope": (pos, 64, 100.0)}), (A, W, g.views[1], b, None), tile=tile), [g])
    g32, s32 = GF.rows_in([M, M], N, F32), torch.full((N // 64, M, 2), float("nan"), device=DEV)
    o16 = GF.rows_in([M], N, F16)
    x = torch.zeros(M, N, device=DEV)
    _refused(lambda: ops.linear_pair((A, W, g32.views[0], b, x, {"emit": (s32, o16.views[0])}), (A, W, g32.views[1], b, x), tile=128), [g32, o16])
    assert bool(torch.isnan(s32).all())
    # tiles without a pair kernel
    for tile in (12864, 256128, 128192, 16):
        g = new()
        _refused(lambda: ops.linear_pair((A, W, g.views[0], b, None), (A, W, g.views[1], b, None), tile=tile), [g])
    # a batched descriptor inside a pair (ops cannot express it)
    g = new()
    d0, d1 = ops._linear_desc(A, W, g.views[0], b, 0, None, 64), ops._linear_desc(A, W, g.views[1], b, 0, None, 64)
    d1.batch, d1.strideA, d1.strideB, d1.strideC = 2, 0, 0, 0
    _refused(lambda: raw(d0, d1), [g])
    d1.batch, d0.batch = 1, 2
    _refused(lambda: raw(d0, d1), [g])


def test_single_refusals_leave_the_outputs_alone():
    """the refusal rules of cut3r_gemm_f16 (ops.linear refuses some of these calls itself; `raw` hands the descriptor to the C side): an
    unknown tile, the exclusions of the skinny tile, the LayerNorm fold's producer anywhere but in the default kernels of tiles 64 / 128 / 256
    with whole K-tiles and an fp32 residual, its consumer at tile 256 without a compile-time epilogue.  No kernel runs.
    (tests/test_lnfold_gpu.py holds `ln` at tile 16 through ops.linear.  The skinny cases with `ln` / `emit` have 64 rows: above that ops.linear
    launches 64-row chunks, and the chunks run without `ln` / `emit`.)"""
    lib = _lib.load()
    M, N, K = 130, 128, 192
    A, W, b, _ = GF.operands(M, N, K, 1)
    A, W, b = A.to(DEV), W.to(DEV), b.to(DEV)
    At, Wt = torch.zeros(M, 200, dtype=F16, device=DEV), torch.zeros(N, 200, dtype=F16, device=DEV)      # a K tail: generic addressing
    p = _consumer(M, K, N, 14)
    pos = torch.zeros(M, 2, dtype=torch.int64, device=DEV)
    x, x16 = torch.zeros(M, N, device=DEV), torch.zeros(M, N, dtype=F16, device=DEV)

    def raw(d, **fields):
        for k, v in fields.items():
            setattr(d, k, v)
        rc = lib.cut3r_gemm_f16(C.byref(d), ops._stream())
        assert rc == 1, rc
        raise ValueError("refused by cut3r_gemm_f16")

    g = GF.rows_in([M], N, F16)
    o = g.views[0]
    _refused(lambda: ops.linear(A, W, o, b, tile=999), [g])
    # the skinny tile: at most 64 rows, no relu_in, no fused RoPE, no LayerNorm fold on either side
    _refused(lambda: raw(ops._linear_desc(A[:65], W, o[:65], b, 0, None, 16)), [g])
    _refused(lambda: raw(ops._linear_desc(A[:64], W, o[:64], b, 0, None, 16), relu_in=1), [g])
    _refused(lambda: ops.linear(A, W, o, b, tile=16, rope=(pos, 64, 100.0)), [g])
    _refused(lambda: raw(ops._linear_desc(A[:64], W, o[:64], b, 0, None, 64, rope=(pos[:64], 64, 100.0)), tile=16), [g])
    ln64 = (p["st"][:, :64].contiguous(), p["dc"], EPS)
    _refused(lambda: raw(ops._linear_desc(p["x16"][:64], p["dWf"], o[:64], p["dd"], 0, None, 64, ln=ln64), tile=16), [g])

    # the producer side of the LayerNorm fold
    g32, g16 = GF.rows_in([M], N, F32), GF.rows_in([M], N, F16)
    o32, o16 = g32.views[0], g16.views[0]
    st = torch.full((N // 64, M, 2), float("nan"), device=DEV)
    emit, emit64 = (st, o16), (st[:, :64].contiguous(), o16[:64])
    _refused(lambda: ops.linear(A[:64], W, o32[:64], b, res1=x[:64], tile=16, emit=emit64), [g32, g16])
    _refused(lambda: raw(ops._linear_desc(A[:64], W, o32[:64], b, 0, x[:64], 64, emit=emit64), tile=16), [g32, g16])
    for tile in (128192, 192128, 256128, 12864):            # tiles without the producer's epilogue
        _refused(lambda: ops.linear(A, W, o32, b, res1=x, tile=tile, emit=emit), [g32, g16])
    for tile in (64, 128, 256):                             # generic addressing: no compile-time epilogue
        _refused(lambda: ops.linear(At, Wt, o32, b, res1=x, tile=tile, emit=emit), [g32, g16])
        _refused(lambda: ops.linear(A, W, o32, b, res1=x16, tile=tile, emit=emit), [g32, g16])         # an fp16 residual
        _refused(lambda: raw(ops._linear_desc(A, W, o32, b, 0, x, tile, emit=emit), res1=x16.data_ptr(), res1_f16=1), [g32, g16])
    assert bool(torch.isnan(st).all())

    # the consumer side at tile 256 lives in the compile-time epilogues: N = 4 mod 8 has none
    p = _consumer(M, K, 132, 16)
    g = GF.rows_in([M], 132, F16)
    _refused(lambda: ops.linear(p["x16"], p["dWf"], g.views[0], p["dd"], tile=256, ln=(p["st"], p["dc"], EPS)), [g])


# ------------------------------------------------------------------------------------------------ 2. batched launches
# (Z, M, N, K, tile, out, layout, bias, res1, act).  "odd" puts sC (fp16 outputs), sBias and sR1 (fp16 residuals) off the alignment that
# gemm256_epi_mode asks of a compile-time epilogue (sC & 7, sBias & 3, sR1 & 7); "contig" and "embed" sit on the other side of it
BATCHED = [
    (2, 197, 768, 768, 0, F16, "embed", True, None, 0), (5, 64, 256, 1024, 0, F32, "contig", True, F32, 0), (2, 768, 768, 1024, 0, F32, "embed", True, None, 0),
    (1, 130, 136, 200, 64, F16, "odd", True, F16, 0), (5, 65, 128, 192, 64, F32, "embed", True, None, 0), (2, 128, 128, 3072, 64, F32, "contig", True, F32, 0),
    (2, 70, 64, 2048, 64, F16, "odd", True, None, 1), (2, 130, 128, 768, 64, F16, "contig", True, None, 1),
    (2, 300, 264, 192, 128, F16, "odd", True, F16, 0), (5, 128, 256, 768, 128, F16, "contig", True, None, 1), (2, 257, 256, 768, 128, F32, "odd", True, F32, 0),
    (1, 256, 256, 64, 128, F32, "embed", False, None, 0), (2, 257, 256, 768, 128, F32, "contig", True, F32, 0),
    (2, 300, 512, 768, 256, F32, "contig", True, F32, 0), (2, 515, 264, 200, 256, F16, "odd", True, F16, 0), (5, 256, 256, 128, 256, F16, "embed", True, None, 1),
    (2, 300, 256, 768, 256, F16, "odd", True, None, 0), (2, 300, 256, 768, 256, F16, "contig", True, F16, 0), (2, 300, 256, 768, 256, F16, "contig", True, None, 0), (1, 257, 256, 768, 256, F32, "odd", True, F32, 0),
    (2, 200, 256, 200, 192128, F32, "odd", True, F32, 0), (5, 192, 128, 768, 192128, F16, "contig", True, None, 0), (2, 385, 264, 768, 192128, F16, "embed", True, F16, 0),
    (2, 129, 196, 72, 128192, F16, "contig", True, None, 1), (5, 128, 384, 768, 128192, F32, "embed", True, F32, 0),
    (2, 257, 136, 200, 256128, F16, "contig", True, F16, 0), (1, 512, 256, 768, 256128, F32, "odd", True, None, 0),
    (2, 130, 72, 72, 12864, F32, "contig", True, F32, 0), (5, 128, 64, 768, 12864, F16, "odd", True, None, 2),
    (2, 8, 1536, 1536, 16, F32, "contig", True, None, 0), (5, 33, 40, 2048, 16, F16, "odd", True, F16, 0), (1, 64, 768, 3072, 16, F32, "embed", True, F32, 0),
    (2, 17, 128, 768, 16, F16, "contig", False, None, 1), (2, 8, 1536, 2048, 16, F32, "embed", True, None, 0), (1, 24, 64, 3072, 16, F32, "contig", True, F16, 0),
    (2, 50, 36, 72, 16, F16, "contig", True, None, 2),
]


@pytest.mark.parametrize("tile", [0, 64, 128, 256, 192128, 128192, 256128, 12864, 16])
def test_batched_launch(tile):
    cases = [c for c in BATCHED if c[4] == tile]
    assert len(cases) >= 2 and {c[0] for c in BATCHED} == {1, 2, 5}
    _run_all(GF.run_batched, cases)


def test_batched_layouts_the_c_side_refuses():
    """fill_args wants 16-byte aligned A / B / C and row strides of whole vectors: an output that starts one fp16 row of N = 4 mod 8 elements
    into its buffer (the decoder_embed layout with such an N) is refused, and nothing is written"""
    Z, M, N, K = 2, 70, 68, 64
    A, W, b, _ = GF.operands(M, N, K, 2, Z=Z)
    buf = torch.full((Z + 1, M + 1, N), GF.SENT, dtype=F16, device=DEV)
    gd = GF.Guard(buf, [buf[:Z, 1:]])
    _refused(lambda: ops.linear_batched(A.to(DEV), W.to(DEV), gd.views[0], b.to(DEV)), [gd])
    buf = torch.full((Z + 1, M + 2, N + 2), GF.SENT, dtype=F32, device=DEV)            # a row stride of 2 mod 4 floats
    gd = GF.Guard(buf, [buf[:Z, 2:, :N]])
    _refused(lambda: ops.linear_batched(A.to(DEV), W.to(DEV), gd.views[0], b.to(DEV)), [gd])


# ------------------------------------------------------------------------------------------------ 3. two residuals
@pytest.mark.parametrize("tile", [0, 64, 128, 256, 192128, 128192, 256128, 12864])
def test_linear_with_two_residuals(tile):
    """fp16 output with two fp16 residuals on whole K-tiles is the compile-time epilogue 5 of the 256 tile; every other combination runs the
    run-time epilogue"""
    cases = []
    for odt in (F16, F32):
        for r1, r2 in ((F16, F16), (F16, F32), (F32, F16), (F32, F32)):
            cases.append(((300, 264, 192) if r1 == r2 else (257, 132, 200)) + (tile, odt, 0, (r1, r2)))
    _run_all(GF.run_single, cases)


# (B, H, W, Cin, Cout, stride, relu_in, tile, residual types, output type)
CONVS = [
    # Cin 256 / 128: the tap of a K-tile is wave-uniform (fast addressing); Cin 96: generic addressing
    (1, 12, 16, 256, 256, 1, False, 256, (F16, F16), F16),       # compile-time epilogue 5
    (1, 12, 16, 256, 256, 1, True, 256, (F16, F16), F16),
    (2, 9, 9, 128, 128, 2, False, 256, (F16, F32), F16),
    (2, 5, 7, 96, 256, 1, False, 256, (F16, F16), F16),
    (2, 5, 7, 96, 256, 2, True, 256, (F32, F16), F16),
    (1, 12, 16, 256, 128, 1, False, 192128, (F16, F16), F16),
    (1, 12, 16, 128, 128, 2, True, 192128, (F16, F16), F16),
    (2, 9, 9, 96, 128, 2, True, 192128, (F16, F32), F16),
    (1, 12, 16, 128, 256, 1, True, 128, (F16, F16), F16),
    (2, 5, 7, 96, 128, 2, False, 128, (F32, F32), F32),
    (1, 12, 16, 256, 256, 2, False, 0, (F16, F16), F16),
    (3, 2, 3, 128, 128, 1, True, 0, (F16, F32), F16),
    (1, 8, 8, 96, 96, 1, False, 0, (F16, F16), F16),
    (1, 24, 32, 256, 256, 1, True, 0, (F16, F16), F16),          # the _rcu convolution of the tiny DPT head: 768 rows
    # no residual: the remaining compile-time epilogues of the convolution kernels (1: bias, 4: bias + ReLU), so that a change to the
    # shared bodies meets every instantiation in this file
    (1, 12, 16, 256, 256, 1, False, 256, (), F16), (1, 12, 16, 128, 256, 2, False, 256, (), F16, 2), (1, 12, 16, 256, 256, 1, True, 256, (), F16, 2),
    (1, 12, 16, 256, 128, 1, False, 192128, (), F16), (1, 12, 16, 128, 128, 1, False, 192128, (), F16, 2),
]


@pytest.mark.parametrize("tile", [0, 256, 192128, 128])
def test_conv3x3_with_two_residuals(tile):
    cases = [c for c in CONVS if c[7] == tile]
    assert len(cases) >= 2
    _run_all(GF.run_conv, cases)


def test_single_launches_of_the_256_tile_that_share_gemm256_body_with_the_pair_kernel():
    """the instantiations of gemm256_kernel that no case above launches (tests/test_lnfold_gpu.py and test_kernels_gpu.py check their values):
    LayerNorm-fold consumer with epilogues 1 / 2 / 6, fused RoPE (6), relu_in on a Linear.  Here: footprint, and the bits of the 64 tile."""
    M, K, N, cols = 300, 768, 512, 256
    p = _consumer(M, K, N, 15)
    pos = torch.randint(-1, 33, (M, 2), generator=torch.Generator().manual_seed(4), dtype=torch.int64).to(DEV)
    A, W, b, _ = GF.operands(M, N, K, 6)
    dA, dW, db = A.to(DEV), W.to(DEV), b.to(DEV)
    for act, rope, ln in ((0, None, True), (1, None, True), (0, (pos, cols, 100.0), True), (0, (pos, cols, 100.0), False)):
        a = (p["x16"], p["dWf"], p["dd"]) if ln else (dA, dW, db)
        kw = dict(rope=rope, ln=(p["st"], p["dc"], EPS) if ln else None)
        gd = GF.rows_in([M], N, F16)
        ops.linear(a[0], a[1], gd.views[0], a[2], act, tile=256, **kw)
        gd.check(f"tile 256 act={act} rope={rope is not None} ln={ln}")
        ref = torch.zeros(M, N, dtype=F16, device=DEV)
        ops.linear(a[0], a[1], ref, a[2], act, tile=64, **kw)
        torch.cuda.synchronize()
        assert torch.equal(gd.views[0], ref), (act, rope is not None, ln)
        if rope is None:
            y = _fold64(p["x16"], p["st"], p["Wf"], p["d"], p["c"])
            _report(f"tile 256 fold consumer act={act}", gd.views[0].float(), F.gelu(y) if act else y, TOL[F16])
    # relu_in on a Linear (cut3r_gemm_desc.relu_in; ops.linear has no argument for it): equals the Linear of relu(A)
    A[::2] -= 1.0
    dA = A.to(DEV)
    for odt in (F16, F32):
        gd = GF.rows_in([M], N, odt)
        d = ops._linear_desc(dA, dW, gd.views[0], db, 0, None, 256)
        d.relu_in = 1
        _lib.check(_lib.load().cut3r_gemm_f16(C.byref(d), ops._stream()), "cut3r_gemm_f16 relu_in")
        gd.check(f"relu_in Linear {odt}")
        assert torch.equal(gd.views[0], GF.single_ref(torch.relu(dA), dW, db, 0, [], odt))
        _report(f"relu_in Linear {odt}", gd.views[0].float(), GF.ref64(torch.relu(A), W, b, 0, []), TOL[odt])


# ------------------------------------------------------------------------------------------------ 4. tuning variants
# every (tile, stages) pair for which cut3r_gemm_f16 launches a kernel of its own (other values fall to the tile's default kernel).
# 128: 3 / 4 ring depths at 4 waves, 8 / 9 the two 8-wave layouts, 10 / 14 deeper rings at 8 waves, 12 s_setprio, 13 the XCD-aware order
STAGES = [(128, s) for s in (3, 4, 8, 9, 10, 12, 13, 14)] + [(192128, 3), (256128, 3), (12864, 3), (64, 2), (64, 4), (64, 8)]


@pytest.mark.parametrize("tile,stages", STAGES)
def test_stages_variants(tile, stages, monkeypatch):
    monkeypatch.setattr(ops, "GEMM_STAGES", stages)
    for M, N, K in ((768, 256, 256), (333, 200, 200)):
        GF.run_single(M, N, K, tile, F16, 1)
        GF.run_single(M, N, K, tile, F32, 0, (F32,), inplace=True)
        GF.run_single(M, N, K, tile, F32, 0)


@pytest.mark.parametrize("tile,stages", [(128, 3), (128, 13), (64, 2), (64, 8)])
def test_stages_variants_refuse_the_fold_producer(tile, stages, monkeypatch):
    """the producer side of the LayerNorm fold lives in the default kernels' compile-time epilogue 3"""
    M, N = 130, 128
    A, W = torch.zeros(M, 64, dtype=F16, device=DEV), torch.zeros(N, 64, dtype=F16, device=DEV)
    gd, g16 = GF.rows_in([M], N, F32), GF.rows_in([M], N, F16)
    st = torch.full((N // 64, M, 2), float("nan"), device=DEV)
    x = torch.zeros(M, N, device=DEV)
    monkeypatch.setattr(ops, "GEMM_STAGES", stages)
    _refused(lambda: ops.linear(A, W, gd.views[0], torch.zeros(N, device=DEV), res1=x, tile=tile, emit=(st, g16.views[0])), [gd, g16])
    assert bool(torch.isnan(st).all())


SWITCHES = [("CUT3R_GEMM_FASTADDR", "0"), ("CUT3R_GEMM_EPI", "0"), ("CUT3R_GEMM64_STAGES", "4"), ("CUT3R_GEMM64_STAGES", "6")]
CHILD_TIMEOUT = 30


def test_environment_switches_in_a_fresh_process(tmp_path):
    """CUT3R_GEMM_FASTADDR=0 (generic addressing everywhere), CUT3R_GEMM_EPI=0 (run-time epilogue everywhere), CUT3R_GEMM64_STAGES=4 / 6
    (ring depth of the 64 x 64 kernels): gemm.hip reads them once per process, so each setting gets a new process that repeats
    gemm_forms_child.SUBSET with its three checks and compares every output, bit for bit, with what THIS process computed under the default
    settings.  One child at a time; the first one that does not exit 0 ends the test.
    Measured on an MI355X: the subset takes 0.1 s in this process; a child takes 2.2 - 2.8 s, nearly all of it interpreter start, the import
    of torch and opening the GPU.  Three times that is 9 s; the limit is 30 s because the measurement was taken with the page cache warm (this
    process had just loaded the same files) and a cold start is not covered by it."""
    t0 = time.time()
    golden = GF.run_subset()
    print(f"[gemm forms] subset of {len(GF.SUBSET)} cases in process: {time.time() - t0:.1f} s")
    path = str(tmp_path / "golden.pt")
    torch.save(golden, path)
    for key, val in SWITCHES:
        env = dict(os.environ)
        env[key] = val
        t0 = time.time()
        try:
            r = subprocess.run([sys.executable, "-m", "tests.gemm_forms_child", path], cwd=ROOT, env=env, timeout=CHILD_TIMEOUT,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        except subprocess.TimeoutExpired as e:
            out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
            pytest.fail(f"{key}={val}: the child was killed at its time limit of {CHILD_TIMEOUT} s; its output:\n{out[-4000:]}")
        if r.returncode < 0:
            pytest.fail(f"{key}={val}: the child was killed by signal {-r.returncode}; its output:\n{r.stdout[-4000:]}")
        assert r.returncode == 0, f"{key}={val}: the child exited {r.returncode}; its output:\n{r.stdout[-4000:]}"
        print(f"[gemm forms] {key}={val}: {r.stdout.strip().splitlines()[-1]} ({time.time() - t0:.1f} s)")
