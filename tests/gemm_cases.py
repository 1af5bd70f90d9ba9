"""The one table of GEMM / 3x3-convolution test cases: a descriptor recipe per row and the kernel instance (cut3r_gemm_kernel_for /
cut3r_gemm_pair_kernel_for, codes documented in include/cut3r_hip.h) that recipe must reach.  tests/test_gemm_cpu.py checks the census
on the host (every case reaches its code, the codes reached are ALL the instances the launchers can launch) and the oracle;
tests/test_gemm_gpu.py launches every row and checks every output element against the fp64 reference (tests/gemm_oracle.py).

Shapes are the smallest at which the instance can still go wrong: for a tile BM x BN, M in {BM + 1, 2 BM - 1}, N in {BN + 4, 2 BN},
K in {64, 72 | 200 (generic addressing), 128}, ring-depth instances with K / 64 below and above the ring depth (64 and 512);
convolutions over B >= 2 images of at most 9 x 15 pixels so that an M-tile crosses an image boundary, stride 2 on odd sizes, Cin 64 | 128
(addressing 2) and 96 (generic: a K-tile straddles two taps).  Inputs: N(0, 1) activations, weights scaled by K^-1/2, bias and residuals of
order 1; where there is a GELU, one block of 8 columns has its bias at -3 (the 1 + erf cancellation)."""
import ctypes as C
import dataclasses
import functools
import zlib
from typing import Optional, Tuple

import torch

from cut3r_slam_amd import _lib

F16, F32 = torch.float16, torch.float32
SENT = -1111.0                      # guard value, exact in fp16 and fp32
DT = {"f16": F16, "f32": F32}
ROPE_PMIN, ROPE_NPOS = -1, 258
LN_EPS = 0.5                        # with slab statistics (0, 32) the fold's rstd is exactly 1 and its mean exactly 0


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    code: int                       # the instance the descriptor must reach (default environment)
    tile: int
    M: int = 0                      # linear: rows; conv / convT: derived
    N: int = 0
    K: int = 0
    stages: int = 0
    conv: Optional[Tuple[int, int, int, int, int]] = None      # (B, H, W, Cin, stride); N = Cout
    shuf: Optional[Tuple[int, int, int, int, int]] = None      # (B, H, W, s, Cout); K = Cin
    relu_in: bool = False
    bias: bool = True
    act: int = 0
    res1: Optional[str] = None      # "f16" | "f32"
    res2: Optional[str] = None
    out: str = "f16"
    Z: int = 1                      # batch (blockIdx.z) with element strides
    pair: int = 0                   # > 0: cut3r_gemm_f16_pair, the second problem has this many rows
    apad: int = 0                   # lda = K + apad
    rpad: int = 0                   # ldr = N + rpad
    pad: int = 8                    # ldc = N + pad: guard columns
    ring: bool = False              # the S digit of `code` follows CUT3R_GEMM64_STAGES (3 by default, 4, 6)
    rope: Optional[Tuple[int, int]] = None      # (columns, head dimension): fused 2-D RoPE
    ln: bool = False                # LayerNorm-fold consumer

    @property
    def special(self):
        """RoPE-epilogue and LayerNorm-fold rows: no bound of their own, bit equality with the unfused sequence (tests/test_gemm_gpu.py)"""
        return self.rope is not None or self.ln

    @property
    def kind(self):
        return "conv" if self.conv else ("convT" if self.shuf else "linear")

    def code_at(self, ring_depth=3):
        return self.code + (ring_depth - 3) * 1000 if self.ring else self.code

    @property
    def nwave(self):
        """K-split of the skinny kernel (for the bound), else 0"""
        return (8 if self.K >= 2048 else 4) if self.tile == 16 else 0


# epilogue ingredients by the compile-time epilogue they qualify for (gemm256_epi_mode) when N is a multiple of 8
E1 = dict()
E2 = dict(act=1)
E3 = dict(out="f32", res1="f32")
E4 = dict(act=2)
E5 = dict(res1="f16", res2="f16")
NOB = dict(bias=False)


def L(name, code, tile, M, N, K, **kw):
    return Case(name, code, tile, M, N, K, **kw)


def CV(name, code, tile, B, H, W, Cin, Cout, stride=1, **kw):
    return Case(name, code, tile, N=Cout, K=9 * Cin, conv=(B, H, W, Cin, stride), **kw)


def CT(name, code, tile, B, H, W, Cin, s, Cout, **kw):
    return Case(name, code, tile, M=B * H * W, N=s * s * Cout, K=Cin, shuf=(B, H, W, s, Cout), **kw)


CASES = [
    # ---- tile 16: gemm_skinny_kernel<NW, MB>
    L("t16_m1_k40_gelu32", 500041, 16, 1, 20, 40, act=1, out="f32"),
    L("t16_m16_k40_gelu", 500041, 16, 16, 32, 40, **E2),
    L("t16_m17_k40_res2", 500042, 16, 17, 20, 40, out="f32", res1="f32", res2="f16"),
    L("t16_m33_k40_relu", 500044, 16, 33, 32, 40, act=2, res1="f16"),
    L("t16_m64_k40", 500044, 16, 64, 20, 40, out="f32", **NOB),
    L("t16_m64_k40_z2", 500044, 16, 64, 36, 40, Z=2, **E3),
    L("t16_m1_k2048", 500081, 16, 1, 132, 2048, out="f32"),
    L("t16_m17_k2048", 500082, 16, 17, 20, 2048, **E3),
    L("t16_m64_k2048", 500084, 16, 64, 36, 2048, res1="f32"),
    # ---- tile 64, stages variants and the 8-wave kernels
    L("t64_s2_k200", 112100, 64, 65, 68, 200, stages=2, **E3),
    L("t64_s2_k384", 112100, 64, 127, 128, 384, stages=2, **E2),
    L("t64_s4_k72", 114100, 64, 65, 128, 72, stages=4, **E5),
    L("t64_s4_k384", 114100, 64, 127, 68, 384, stages=4, out="f32"),
    L("t64_s8_k200", 113200, 64, 65, 68, 200, stages=8, **E2),
    L("t64_s8_k64", 113200, 64, 127, 128, 64, stages=8, **E3),
    L("t64_w8_k2048_res", 113213, 64, 130, 128, 2048, ring=True, **E3),
    L("t64_w8_k2048_f16", 113210, 64, 65, 132, 2048),
    CV("t64_w8_conv256", 113220, 64, 2, 5, 7, 256, 68, **E4),
    # ---- tile 64, default kernels (the ring depth follows CUT3R_GEMM64_STAGES)
    L("t64_fast_ragged", 113110, 64, 65, 68, 64, ring=True),
    L("t64_fast_nobias", 113110, 64, 127, 128, 512, ring=True, out="f32", **NOB),
    L("t64_fast_res16", 113110, 64, 65, 128, 128, ring=True, **E5),
    L("t64_fast_gelu32", 113110, 64, 65, 128, 64, ring=True, act=1, out="f32"),
    L("t64_e1", 113111, 64, 65, 128, 64, ring=True),
    L("t64_e1_exact", 113111, 64, 128, 128, 512, ring=True, apad=8),
    L("t64_e1_z2", 113111, 64, 65, 64, 128, ring=True, Z=2),
    L("t64_e2", 113112, 64, 127, 128, 64, ring=True, **E2),
    L("t64_e2_k512", 113112, 64, 65, 64, 512, ring=True, **E2),
    L("t64_e3", 113113, 64, 65, 68, 64, ring=True, **E3),
    L("t64_e3_exact", 113113, 64, 128, 128, 512, ring=True, **E3),
    L("t64_prio", 113100, 64, 65, 128, 128, stages=12),                    # (any stages value but 0 takes generic addressing at tile 64)
    CV("t64_conv64", 113120, 64, 2, 5, 7, 64, 64, **E1),
    CV("t64_conv128_s2", 113120, 64, 2, 9, 11, 128, 68, 2, relu_in=True, **E5),
    L("t64_generic_k72", 113100, 64, 65, 68, 72, **E2),
    L("t64_generic_k200", 113100, 64, 127, 128, 200, **E3),
    CV("t64_conv96", 113100, 64, 2, 5, 7, 96, 64, **E4),
    CT("t64_convT", 113110, 64, 2, 3, 5, 64, 2, 20, ring=True),
    # ---- tile 128
    L("t128_s3", 123100, 128, 129, 132, 200, stages=3, **E3),
    L("t128_s3_k320", 123100, 128, 255, 256, 320, stages=3, **E2),
    L("t128_s4", 122100, 128, 129, 256, 72, stages=4, **E5),
    L("t128_s8", 122200, 128, 255, 132, 200, stages=8, **E2),
    L("t128_s8_k128", 122200, 128, 129, 256, 128, stages=8, **E3),
    L("t128_s9", 122300, 128, 129, 132, 128, stages=9, **E3),
    L("t128_s10", 123300, 128, 129, 132, 200, stages=10, **E2),
    L("t128_s10_k320", 123300, 128, 255, 256, 320, stages=10, **E3),
    L("t128_s14", 124300, 128, 129, 256, 72, stages=14, **E3),
    L("t128_s14_k384", 124300, 128, 255, 132, 384, stages=14, **E4),
    L("t128_generic_k72", 122300, 128, 129, 132, 72, **E2),
    L("t128_generic_k200_z2", 122300, 128, 255, 256, 200, Z=2, **E3),
    CV("t128_conv96", 122300, 128, 2, 9, 11, 96, 128, **E5),
    CV("t128_conv96_s2", 122300, 128, 3, 9, 15, 96, 132, 2, relu_in=True),
    L("t128_fast_ragged", 122310, 128, 129, 132, 64),
    L("t128_fast_gelu32", 122310, 128, 129, 256, 128, act=1, out="f32"),
    L("t128_fast_res2", 122310, 128, 255, 256, 128, out="f32", res1="f16", res2="f32"),
    L("t128_e1", 122311, 128, 129, 256, 64),
    L("t128_e1_swz3x3", 122311, 128, 300, 384, 128, stages=13),
    L("t128_swz3x3_ragged", 122313, 128, 257, 260, 64, stages=13, **E3),
    L("t128_e1_210tiles", 122311, 128, 1793, 1792, 64),
    L("t128_e2", 122312, 128, 255, 256, 128, **E2),
    L("t128_e3", 122313, 128, 129, 132, 64, **E3),
    L("t128_e3_exact_z2", 122313, 128, 256, 128, 128, Z=2, **E3),
    CV("t128_conv64", 122320, 128, 2, 9, 11, 64, 128, **E4),
    CV("t128_conv128_s2", 122320, 128, 3, 9, 15, 128, 132, 2, relu_in=True, **E5),
    CV("t128_conv64_1x2", 122320, 128, 2, 1, 2, 64, 128),
    CT("t128_convT", 122300, 128, 2, 9, 11, 72, 2, 36),
    # ---- 128 x 192, 192 x 128, 256 x 128, 128 x 64
    L("t128192_k72", 132300, 128192, 129, 196, 72, **E2),
    L("t128192_k64", 132300, 128192, 255, 384, 64, **E3),
    L("t192_s3", 143300, 192128, 193, 132, 200, stages=3, **E2),
    L("t192_s3_k320", 143300, 192128, 383, 256, 320, stages=3, **E3),
    CV("t192_conv64_e1", 142321, 192128, 2, 9, 11, 64, 128),
    CV("t192_conv128_e1_s2", 142321, 192128, 5, 9, 15, 128, 256, 2),
    CV("t192_conv64_e4", 142324, 192128, 2, 9, 11, 64, 128, **E4),
    CV("t192_conv64_res", 142320, 192128, 2, 9, 11, 64, 128, relu_in=True, **E5),
    CV("t192_conv128_ragged", 142320, 192128, 3, 9, 11, 128, 132, **E4),
    L("t192_fast", 142310, 192128, 193, 132, 64, **E3),
    L("t192_fast_e2", 142310, 192128, 383, 256, 128, **E2),
    L("t192_generic", 142300, 192128, 193, 132, 72, **E5),
    CV("t192_conv96", 142300, 192128, 3, 9, 11, 96, 128, 2, **E4),
    L("t256128_s3", 153300, 256128, 257, 132, 200, stages=3, **E2),
    L("t256128_s3_k320", 153300, 256128, 511, 256, 320, stages=3, **E3),
    L("t256128", 152300, 256128, 257, 132, 72, **E3),
    L("t256128_k128", 152300, 256128, 511, 256, 128, **E5),
    L("t12864_s3", 163100, 12864, 129, 68, 200, stages=3, **E3),
    L("t12864_s3_k320", 163100, 12864, 255, 128, 320, stages=3, **E2),
    L("t12864", 162100, 12864, 129, 68, 72, **E2),
    L("t12864_k128", 162100, 12864, 255, 128, 128, **E3),
    # ---- tile 256: gemm256_kernel<CONV3, RELU_IN, FAST_DMA, EPI, LN>
    L("t256_generic", 300000, 256, 257, 260, 72, **E2),
    L("t256_generic_k200", 300000, 256, 511, 512, 200, **E3),
    L("t256_relu_in", 301000, 256, 257, 260, 64, relu_in=True, **E3),
    L("t256_relu_in_k200", 301000, 256, 300, 512, 200, relu_in=True, **E2),
    L("t256_fast_ragged", 300100, 256, 257, 260, 64, **E2),
    L("t256_fast_nobias", 300100, 256, 511, 512, 128, out="f32", **NOB),
    L("t256_fast_relu", 300100, 256, 257, 256, 128, **E4),
    L("t256_fast_gelu32", 300100, 256, 257, 264, 64, act=1, out="f32"),
    L("t256_e1", 300110, 256, 257, 512, 64),
    L("t256_e1_exact_z2", 300110, 256, 256, 256, 128, Z=2),
    L("t256_e2", 300120, 256, 511, 264, 128, **E2),
    L("t256_e3", 300130, 256, 257, 260, 64, **E3),
    L("t256_e3_k128", 300130, 256, 511, 512, 128, **E3),
    CV("t256_conv96", 310000, 256, 3, 9, 11, 96, 256, **E5),
    CV("t256_conv96_s2", 310000, 256, 7, 9, 15, 96, 260, 2, **E4),
    CV("t256_conv96_relu_in", 311000, 256, 3, 9, 11, 96, 260, relu_in=True, **E4),
    CV("t256_conv96_relu_in_s2", 311000, 256, 7, 9, 15, 96, 256, 2, relu_in=True, **E5),
    CV("t256_conv64_relu_in_e4", 311140, 256, 3, 9, 11, 64, 256, relu_in=True, **E4),
    CV("t256_conv128_relu_in_e4_s2", 311140, 256, 7, 9, 15, 128, 264, 2, relu_in=True, **E4),
    CV("t256_conv64_relu_in_res", 311100, 256, 3, 9, 11, 64, 256, relu_in=True, **E5),
    CV("t256_conv128_relu_in_ragged", 311100, 256, 3, 9, 11, 128, 260, relu_in=True),
    CV("t256_conv64_e1", 310110, 256, 3, 9, 11, 64, 256),
    CV("t256_conv128_e1_s2", 310110, 256, 7, 9, 15, 128, 264, 2),
    CV("t256_conv64_e4", 310140, 256, 3, 9, 11, 64, 264, **E4),
    CV("t256_conv128_e5", 310150, 256, 3, 9, 11, 128, 256, **E5),
    CV("t256_conv64_e5_res1", 310150, 256, 7, 9, 15, 64, 264, 2, res1="f16"),
    CV("t256_conv64_ragged", 310100, 256, 3, 9, 11, 64, 260, **E4),
    CV("t256_conv128_f32", 310100, 256, 3, 9, 11, 128, 256, **E3),
    CT("t256_convT", 300100, 256, 2, 9, 15, 64, 2, 68),
    # (RoPE epilogue and LayerNorm fold: instances no other recipe reaches)
    L("t256_rope", 300160, 256, 257, 512, 128, rope=(256, 64)),
    L("t256_ln_e1", 300111, 256, 257, 264, 128, ln=True),
    L("t256_ln_e2", 300121, 256, 300, 512, 64, ln=True, **E2),
    L("t256_ln_rope", 300161, 256, 257, 512, 128, ln=True, rope=(256, 64)),
    # ---- pairs (cut3r_gemm_f16_pair), M0 != M1
    L("p64_e1", 213111, 64, 65, 128, 64, pair=127),
    L("p64_e2", 213112, 64, 127, 64, 128, pair=65, **E2),
    L("p64_e3", 213113, 64, 65, 68, 512, pair=130, **E3),
    L("p64_fast", 213110, 64, 65, 68, 64, pair=1, **E2),
    L("p64_fast_nobias", 213110, 64, 127, 128, 128, pair=65, out="f32", **NOB),
    L("p64_generic", 213100, 64, 65, 68, 72, pair=127, **E3),
    L("p64_generic_k200", 213100, 64, 127, 128, 200, pair=64, **E5),
    L("p64_w8_e3", 213213, 64, 130, 128, 2048, pair=65, **E3),
    L("p64_w8_fast", 213210, 64, 65, 132, 2048, pair=70, res1="f16"),
    L("p64_w8_generic", 213200, 64, 65, 68, 2056, pair=66, **E3),
    L("p128", 222300, 128, 129, 132, 72, pair=255, **E2),
    L("p128_k128", 222300, 128, 255, 256, 128, pair=129, **E3),
    L("p192", 242300, 192128, 193, 132, 200, pair=383, **E3),
    L("p192_k64", 242300, 192128, 383, 256, 64, pair=190, **E2),
    L("p256", 400000, 256, 257, 260, 200, pair=300, **E2),
    L("p256_k128", 400000, 256, 511, 256, 128, pair=257, **E3),
]
BY_NAME = {c.name: c for c in CASES}
TILE_DIMS = {16: (64, 16), 64: (64, 64), 128: (128, 128), 256: (256, 256), 128192: (128, 192), 192128: (192, 128), 256128: (256, 128), 12864: (128, 64)}
PINNED = [c for c in CASES if not c.special]         # the rows checked per element against the fp64 reference
assert len(BY_NAME) == len(CASES)

# descriptors the launchers refuse (code 0; a launch returns 1 and writes nothing): (name, base case, descriptor fields to overwrite)
REFUSED = [
    ("k_not_mult_of_8", "t64_e1", dict(K=60)),
    ("n_not_mult_of_4", "t64_e1", dict(N=126)),
    ("unknown_tile", "t64_e1", dict(tile=32)),
    ("skinny_65_rows", "t16_m64_k40", dict(M=65)),
    ("skinny_conv", "t64_conv64", dict(tile=16)),
    ("conv_k_mismatch", "t64_conv64", dict(K=512)),
    ("shuf_n_mismatch", "t64_convT", dict(shuf_cout=24)),
    ("ldr_not_mult_of_4", "t64_e3", dict(ldr1=70)),
    ("pair_n_mismatch", "p64_e1", dict(N=64)),
    ("pair_conv", "p64_e1", dict(conv_k=3, Cin=8, K=72)),
]


# ------------------------------------------------------------------------------------------------ operands
def _problem(c, M, seed):
    """one problem of the case with M rows: fp16-rounded operands, fp32 bias, residuals in their own type, on the CPU"""
    g = torch.Generator().manual_seed(seed)
    Z, N, K = c.Z, c.N, c.K
    p = dict(kind=c.kind, relu_in=c.relu_in, act=c.act, out=DT[c.out], stride=0, shuf=c.shuf, x=None, A=None)
    if c.conv:
        B, H, Wd, Cin, stride = c.conv
        p["x"] = torch.randn(B, H, Wd, Cin, generator=g).half()
        p["stride"] = stride
        M = B * ((H - 1) // stride + 1) * ((Wd - 1) // stride + 1)
    else:
        p["A"] = torch.randn(Z, M, K, generator=g).half()
    p["W"] = (torch.randn(Z, N, K, generator=g) / K ** 0.5).half()
    nb = c.shuf[4] if c.shuf else N
    p["bias"] = torch.randn(Z, nb, generator=g) if c.bias else None
    if c.bias and c.act == 1:
        c0 = (nb // 2) & ~7                                           # the GELU cancellation: pre-activations of about -3
        p["bias"][:, c0:c0 + 8] = -3.0 + 0.1 * torch.randn(Z, min(8, nb - c0), generator=g)
    for k in ("res1", "res2"):
        dt = getattr(c, k)
        p[k] = torch.randn(Z, M, N, generator=g).to(DT[dt]) if dt else None
    p["M"] = M
    return p


@functools.lru_cache(maxsize=None)
def operands(name):
    """the case's problems (two for a pair), generated once per process and never modified"""
    c = BY_NAME[name]
    seed = zlib.crc32(name.encode())
    ps = [_problem(c, c.M, seed)]
    if c.pair:
        ps.append(_problem(c, c.pair, seed + 1))
    return ps


# ------------------------------------------------------------------------------------------------ buffers and descriptors
def _strided(t, ld, device):
    """t [Z, M, n] as a view with row stride ld inside a zero buffer on `device`"""
    Z, M, n = t.shape
    buf = torch.zeros(Z, M, ld, dtype=t.dtype, device=device)
    buf[:, :, :n] = t.to(device)
    return buf[:, :, :n]


def out_buffer(c, p, device):
    """-> (buffer, payload view [Z, Mo, No]): guard rows above and below every batch (as many as keep each batch's first row 16-byte
    aligned), `pad` guard columns, one whole guard batch at the end; guards hold SENT, the payload NaN"""
    Mo, No = (p["M"] * c.shuf[3] ** 2, c.shuf[4]) if c.shuf else (p["M"], c.N)
    dt = p["out"]
    ld, q = No + c.pad, 8 if dt == F16 else 4
    top = 1
    while (top * ld) % q:
        top += 1
    rows = top + Mo + 1
    while (rows * ld) % q:
        rows += 1
    buf = torch.full((c.Z + 1, rows, ld), SENT, dtype=dt, device=device)
    view = buf[:c.Z, top:top + Mo, :No]
    view.fill_(float("nan"))
    return buf, view


def place(c, p, device):
    """the problem's operands on `device` in the case's strided layout, its guarded output, and the descriptor that points at them"""
    t = {}
    if c.conv:
        t["A"] = p["x"].to(device)
    else:
        t["A"] = _strided(p["A"], c.K + c.apad, device)
    t["W"] = p["W"].to(device)
    t["bias"] = p["bias"].to(device) if p["bias"] is not None else None
    for k in ("res1", "res2"):
        t[k] = _strided(p[k], c.N + c.rpad, device) if p[k] is not None else None
    t["buf"], t["out"] = out_buffer(c, p, device)
    d = _lib.GemmDesc()
    d.A, d.B, d.C = t["A"].data_ptr(), t["W"].data_ptr(), t["out"].data_ptr()
    d.bias = t["bias"].data_ptr() if t["bias"] is not None else None
    d.M, d.N, d.K = p["M"], c.N, c.K
    d.lda = c.conv[3] if c.conv else t["A"].stride(1)
    d.ldb, d.ldc = c.K, t["out"].stride(1)
    d.act, d.out_f16 = c.act, int(p["out"] == F16)
    for i, k in ((1, "res1"), (2, "res2")):
        if t[k] is not None:
            setattr(d, k, t[k].data_ptr())
            setattr(d, f"ldr{i}", t[k].stride(1))
            setattr(d, f"res{i}_f16", int(t[k].dtype == F16))
    d.batch = c.Z
    if c.Z > 1:
        d.strideA, d.strideB, d.strideC = t["A"].stride(0), t["W"].stride(0), t["out"].stride(0)
        d.strideBias = t["bias"].stride(0) if t["bias"] is not None else 0
        d.strideR1 = t["res1"].stride(0) if t["res1"] is not None else 0
        d.strideR2 = t["res2"].stride(0) if t["res2"] is not None else 0
    if c.conv:
        B, H, Wd, Cin, stride = c.conv
        d.conv_k, d.H, d.W, d.Cin, d.conv_stride = 3, H, Wd, Cin, stride
        d.Ho, d.Wo = (H - 1) // stride + 1, (Wd - 1) // stride + 1
    if c.shuf:
        B, H, Wd, s, Cout = c.shuf
        d.shuf, d.shuf_cout, d.shuf_Hin, d.shuf_Win = s, Cout, H, Wd
    if c.rope:                      # (contents: the test's business; positions -1 .. 256 as cut3r_slam_amd.ops lays the table out)
        t["pos"] = torch.zeros(p["M"], 2, dtype=torch.int64, device=device)
        t["table"] = torch.zeros(2, ROPE_NPOS, c.rope[1] // 4, dtype=F32, device=device)
        d.rope_pos, d.rope_table, d.rope_cols, d.rope_pmin, d.rope_npos, d.rope_d = t["pos"].data_ptr(), t["table"].data_ptr(), c.rope[0], ROPE_PMIN, ROPE_NPOS, c.rope[1]
    if c.ln:
        t["stats"] = torch.zeros(c.K // 64, p["M"], 2, dtype=F32, device=device)
        t["colsum"] = torch.zeros(c.N, dtype=F32, device=device)
        d.ln_stats, d.ln_colsum, d.ln_nslab, d.ln_eps = t["stats"].data_ptr(), t["colsum"].data_ptr(), c.K // 64, LN_EPS
    d.relu_in = int(c.relu_in)
    d.tile, d.stages = c.tile, c.stages
    t["desc"] = d
    return t


def placed(c, device="cpu"):
    """every problem of the case placed on `device` (the host census uses the CPU copies: the query reads no operand)"""
    return [place(c, p, device) for p in operands(c.name)]


def kernel_for(lib, c, ts):
    """the instance code the library names for the placed case"""
    if c.pair:
        return lib.cut3r_gemm_pair_kernel_for(C.byref(ts[0]["desc"]), C.byref(ts[1]["desc"]))
    return lib.cut3r_gemm_kernel_for(C.byref(ts[0]["desc"]))


def refused(name, base, fields, device="cpu"):
    """a refused descriptor (pair): the base case placed on `device`, then the fields overwritten (in the first descriptor of a pair)"""
    c = BY_NAME[base]
    ts = placed(c, device)
    for k, v in fields.items():
        setattr(ts[0]["desc"], k, v)
    return c, ts
