"""Thin torch-tensor front ends over the C ABI (include/cut3r_hip.h).  torch is used only for device memory and
the current HIP stream; every computation is a hand-written gfx950 kernel in libcut3r_hip.so.

All functions validate shapes/dtypes/strides on the host BEFORE launching (a faulting kernel can reset the GPU).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

from . import _lib, views
from ._lib import GemmDesc, check

F16, F32 = torch.float16, torch.float32


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _req(cond, msg):
    if not cond:
        raise ValueError(msg)


def _aligned(nbytes, **ts):
    """the base address of every tensor given by name is a multiple of nbytes: the kernels read and write 8- / 16-byte vectors, and a view
    that starts at a column offset (big[:, 2:]) keeps an aligned row stride but not an aligned first element"""
    for name, t in ts.items():
        if t is not None:
            _req(t.data_ptr() % nbytes == 0, f"{name} must start on a {nbytes}-byte boundary (a column-offset view?): address % {nbytes} = {t.data_ptr() % nbytes}")


def _cuda(*ts):
    for t in ts:
        if t is not None:
            _req(t.is_cuda, "tensor must live on the GPU (no CPU fallback in the product path)")


# ------------------------------------------------------------------------------------------------ RoPE
def rope_2d(tokens: torch.Tensor, positions: torch.Tensor, base: float, fwd: float) -> None:
    """Drop-in for curope.rope_2d (reference src/croco/models/curope/curope.cpp:49-65): in place on a (B,N,H,D)
    view; same checks/errors as the reference's TORCH_CHECKs (RuntimeError on violation)."""
    if tokens.dim() != 4:
        raise RuntimeError("tokens must have 4 dimensions")
    if positions.dim() != 3:
        raise RuntimeError("positions must have 3 dimensions")
    if tokens.size(0) != positions.size(0):
        raise RuntimeError("batch size differs between tokens & positions")
    if tokens.size(1) != positions.size(1):
        raise RuntimeError("seq_length differs between tokens & positions")
    if positions.size(2) != 2:
        raise RuntimeError("positions.shape[2] must be equal to 2")
    if tokens.is_cuda != positions.is_cuda:
        raise RuntimeError("tokens and positions are not on the same device")
    if not tokens.is_cuda:
        raise RuntimeError("cut3r_slam_amd.rope_2d: GPU tensors only (HIP kernel; no CPU path in the product)")
    B, N, H, D = tokens.shape
    if tokens.stride(3) != 1 or tokens.stride(2) != D:
        raise RuntimeError("tokens are not contiguous")
    if not positions.is_contiguous():
        raise RuntimeError("positions are not contiguous")
    if D % 4 != 0:
        raise RuntimeError("token dim must be multiple of 4")
    if D % 16 != 0:
        raise RuntimeError("cut3r_slam_amd.rope_2d: head dims that are multiples of 16 only (CUT3R uses 16/32/48/64)")
    if positions.dtype != torch.int64:
        raise RuntimeError("positions must be int64")
    dt = {F32: 0, F16: 1}.get(tokens.dtype)
    if dt is None:
        raise RuntimeError(f"unsupported token dtype {tokens.dtype}")
    lib = _lib.load()
    check(lib.cut3r_rope2d(_p(tokens), dt, _p(positions), B, N, H, D, tokens.stride(0), tokens.stride(1),
                           tokens.stride(2), float(base), float(fwd), _stream()), "cut3r_rope2d")


def rope_2d_qk(q, k, positions, base, fwd):
    """rope_2d(q) and rope_2d(k) with shared positions in one launch (self-attention).  q,k: (B,N,H,D) views, head stride D."""
    for t in (q, k):
        if t.dim() != 4 or t.stride(3) != 1 or t.stride(2) != t.size(3) or not t.is_cuda:
            raise RuntimeError("tokens are not contiguous")
    B, N, H, D = q.shape
    if k.shape != q.shape or positions.shape != (B, N, 2) or positions.dtype != torch.int64 or not positions.is_contiguous():
        raise RuntimeError("rope_2d_qk: shape/dtype mismatch")
    dt = {F32: 0, F16: 1}.get(q.dtype)
    if dt is None or k.dtype != q.dtype:
        raise RuntimeError(f"unsupported token dtype {q.dtype}")
    lib = _lib.load()
    check(lib.cut3r_rope2d_qk(_p(q), _p(k), dt, _p(positions), B, N, H, D, q.stride(0), q.stride(1), k.stride(0), k.stride(1),
                              float(base), float(fwd), _stream()), "cut3r_rope2d_qk")


_ROPE_TABLE_LAUNCH = os.environ.get("CUT3R_ROPE_TABLE", "1") != "0"


def _rope_seg(t, pos):
    """(B,N,H,D) fp16 view with head stride D and a uniform token stride -> (ptr, pos ptr, tokens, token stride)"""
    if t.dim() != 4 or t.dtype != F16 or not t.is_cuda or t.stride(3) != 1 or t.stride(2) != t.size(3):
        raise RuntimeError("tokens are not contiguous")
    B, N = t.shape[:2]
    if B > 1 and t.stride(0) != N * t.stride(1):
        raise RuntimeError("rope_2d_pair: the token stride must be uniform over the batch")
    if pos.shape != (B, N, 2) or pos.dtype != torch.int64 or not pos.is_contiguous() or not pos.is_cuda:
        raise RuntimeError("positions must be contiguous int64 [B,N,2]")
    return _p(t), _p(pos), B * N, t.stride(1)


def rope_2d_pair(t0, pos0, t1, pos1, base, fwd=1.0):
    """rope_2d(t0, pos0) and rope_2d(t1, pos1) in ONE table-driven launch (fp16; results are bit-identical to rope_2d): q and k of a
    self-attention (pos1 is pos0) or of a cross-attention (two token streams).  t1 may be None."""
    H, D = t0.shape[2:]
    if D % 16 != 0:
        raise RuntimeError("cut3r_slam_amd.rope_2d: head dims that are multiples of 16 only (CUT3R uses 16/32/48/64)")
    if not _ROPE_TABLE_LAUNCH:            # A/B knob: the one-workgroup-per-token kernel (same bits)
        if t1 is not None and pos1 is pos0 and t1.shape == t0.shape:
            return rope_2d_qk(t0, t1, pos0, base, fwd)
        rope_2d(t0, pos0, base, fwd)
        if t1 is not None:
            rope_2d(t1, pos1, base, fwd)
        return
    if t1 is not None and tuple(t1.shape[2:]) != (H, D):
        raise RuntimeError("rope_2d_pair: both tensors must have the same heads and head dim")
    a = _rope_seg(t0, pos0)
    b = _rope_seg(t1, pos1) if t1 is not None else (None, None, 0, 0)
    tab = rope_table(t0.device, base, fwd, D)
    lib = _lib.load()
    check(lib.cut3r_rope2d_tab(a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3], H, D, _p(tab), ROPE_PMIN, ROPE_NPOS, float(base), float(fwd),
                               _stream()), "cut3r_rope2d_tab")


# ------------------------------------------------------------------------------------------------ LayerNorm
def layernorm(x, gamma, beta, eps=1e-6, out16=None, out32=None, mod_scale=None, mod_shift=None):
    _cuda(x, gamma, beta, out16, out32, mod_scale, mod_shift)
    _req(x.dtype == F32 and x.dim() == 2 and x.stride(1) == 1, "x must be fp32 [M,C] with unit inner stride")
    M, Cc = x.shape
    _req(gamma.dtype == F32 and beta.dtype == F32 and gamma.numel() == Cc and beta.numel() == Cc, "gamma/beta [C] fp32")
    _req(gamma.is_contiguous() and beta.is_contiguous(), "gamma/beta contiguous")
    for o, dt in ((out16, F16), (out32, F32)):
        if o is not None:
            _req(o.dtype == dt and o.shape == x.shape and o.stride(1) == 1, "bad LN output tensor")
    for m in (mod_scale, mod_shift):
        if m is not None:
            _req(m.dtype == F32 and m.numel() == Cc and m.is_contiguous(), "modulation vectors must be fp32 [C]")
    _aligned(16, x=x, gamma=gamma, beta=beta, out32=out32, mod_scale=mod_scale, mod_shift=mod_shift)
    _aligned(8, out16=out16)
    lib = _lib.load()
    check(lib.cut3r_layernorm(_p(x), x.stride(0), _p(gamma), _p(beta), float(eps), M, Cc,
                              _p(out16), out16.stride(0) if out16 is not None else 0,
                              _p(out32), out32.stride(0) if out32 is not None else 0,
                              _p(mod_scale), _p(mod_shift), _stream()), "cut3r_layernorm")


def layernorm_dual(x, g1, b1, out1, g2, b2, out2, eps=1e-6):
    """out1 = LN(x; g1, b1), out2 = LN(x; g2, b2), both fp16, one pass over x (C in {768, 1024, 1536})"""
    _cuda(x, g1, b1, out1, g2, b2, out2)
    M, Cc = x.shape
    _req(x.dtype == F32 and x.stride(1) == 1 and Cc in (768, 1024, 1536), "x fp32 [M,C], C in {768,1024,1536}")
    for o in (out1, out2):
        _req(o.dtype == F16 and o.shape == (M, Cc) and o.stride(1) == 1, "outputs fp16 [M,C]")
    for t in (g1, b1, g2, b2):
        _req(t.dtype == F32 and t.numel() == Cc and t.is_contiguous(), "gamma/beta fp32 [C]")
    _req(float(eps) > 0.0, f"layernorm_dual: eps must be > 0, got {eps}")
    _aligned(16, x=x, g1=g1, b1=b1, g2=g2, b2=b2)
    _aligned(8, out1=out1, out2=out2)
    lib = _lib.load()
    check(lib.cut3r_layernorm_dual(_p(x), x.stride(0), _p(g1), _p(b1), _p(out1), out1.stride(0), _p(g2), _p(b2), _p(out2), out2.stride(0),
                                   float(eps), M, Cc, _stream()), "cut3r_layernorm_dual")


def layernorm_tokens(x, gamma, beta, eps, pose32, pose16, tok16, tok32=None):
    """LayerNorm of Wn groups of N + 1 rows (x fp32 [Wn * (N + 1), C]) written where the consumers read it, in one launch: row 0 of group w
    -> pose32[w] (fp32 [Wn,C]) and pose16[w] (fp16 [Wn,C]); rows 1..N -> tok16[w] (fp16 [Wn,N,C]) and, if given, tok32[w] (fp32 [Wn,N,C]).  The
    destinations may be slices of larger tensors (any group stride, rows of a group contiguous).  Same bits as `layernorm` + copies."""
    _cuda(x, gamma, beta, pose32, pose16, tok16, tok32)
    _req(x.dtype == F32 and x.dim() == 2 and x.stride(1) == 1, "x must be fp32 [M,C] with unit inner stride")
    _req(tok16.dim() == 3, "tok16 [Wn,N,C]")
    Wn, N, Cc = tok16.shape
    _req(Wn > 0 and N > 0 and x.shape == (Wn * (N + 1), Cc), f"x must hold Wn * (N + 1) = {Wn * (N + 1)} rows of {Cc}")
    _req(gamma.dtype == F32 and beta.dtype == F32 and gamma.numel() == Cc and beta.numel() == Cc, "gamma/beta [C] fp32")
    _req(gamma.is_contiguous() and beta.is_contiguous(), "gamma/beta contiguous")
    _req(float(eps) > 0.0, f"layernorm_tokens: eps must be > 0, got {eps}")
    for o, dt in ((pose32, F32), (pose16, F16)):
        _req(o.dtype == dt and o.shape == (Wn, Cc) and o.stride(1) == 1, "pose outputs [Wn,C] with unit inner stride")
    for o, dt in ((tok16, F16), (tok32, F32)):
        if o is not None:
            _req(o.dtype == dt and o.shape == (Wn, N, Cc) and o.stride(2) == 1 and o.stride(1) == Cc, "token outputs [Wn,N,C], rows of a group contiguous")
    _aligned(16, x=x, gamma=gamma, beta=beta, pose32=pose32, tok32=tok32)
    _aligned(8, pose16=pose16, tok16=tok16)
    lib = _lib.load()
    check(lib.cut3r_layernorm_tokens(_p(x), x.stride(0), _p(gamma), _p(beta), float(eps), Wn, N, Cc, _p(pose32), pose32.stride(0),
                                     _p(pose16), pose16.stride(0), _p(tok16), tok16.stride(0), _p(tok32),
                                     tok32.stride(0) if tok32 is not None else 0, _stream()), "cut3r_layernorm_tokens")


# ------------------------------------------------------------------------------------------------ GEMM
LN_FOLD_MAX_K = 1024        # the folded epilogue reads at most 16 slabs of 64 columns per row (LN_MAXS in csrc/gemm.hip)
GEMM_STAGES = int(os.environ.get("CUT3R_GEMM_STAGES", "0"))     # tuning override (0 = kernel default)


def _fill_common(d, A, Bw, out, bias, res1, res2, act, tile):
    d.A, d.B, d.C = A.data_ptr(), Bw.data_ptr(), out.data_ptr()
    d.bias = bias.data_ptr() if bias is not None else None
    d.act = act
    d.out_f16 = 1 if out.dtype == F16 else 0
    d.batch = 1
    d.tile = tile
    d.stages = GEMM_STAGES
    for i, r in ((1, res1), (2, res2)):
        if r is not None:
            _req(r.dtype in (F16, F32) and r.stride(-1) == 1, "residual must be fp16/fp32 with unit inner stride")
            setattr(d, f"res{i}", r.data_ptr())
            setattr(d, f"ldr{i}", r.stride(-2))
            setattr(d, f"res{i}_f16", 1 if r.dtype == F16 else 0)


_ROPE_TABLES = {}
ROPE_PMIN, ROPE_NPOS = -1, 258        # positions -1 (pose token) .. 256


def rope_table(device, base, fwd=1.0, head_dim=64):
    """cos|sin table [2, ROPE_NPOS, head_dim/4] of the RoPE angles (cut3r_rope2d_table), cached per device"""
    key = (str(device), float(base), float(fwd), int(head_dim))
    t = _ROPE_TABLES.get(key)
    if t is None:
        t = torch.empty(2, ROPE_NPOS, head_dim // 4, dtype=F32, device=device)
        lib = _lib.load()
        check(lib.cut3r_rope2d_table(_p(t), ROPE_PMIN, ROPE_NPOS, head_dim // 4, float(base), float(fwd), _stream()), "cut3r_rope2d_table")
        _ROPE_TABLES[key] = t
    return t


def _launch(d, what):
    check(_lib.load().cut3r_gemm_f16(C.byref(d), _stream()), what)


def _linear_desc(A, W, out, bias, act, res1, tile, rope=None, ln=None, emit=None, *, res2=None, pair=False):
    """the checks of one Linear and its descriptor: ops.linear, and each side of ops.linear_pair (pair: 64-wide heads only)"""
    _cuda(A, W, out, bias, res1, res2)
    _req(A.dtype == F16 and W.dtype == F16 and A.dim() == 2 and W.dim() == 2, "A,W must be 2-D fp16")
    M, K = A.shape
    N = W.shape[0]
    _req(W.shape[1] == K and out.shape == (M, N), f"shape mismatch A{tuple(A.shape)} W{tuple(W.shape)} out{tuple(out.shape)}")
    _req(A.stride(1) == 1 and W.stride(1) == 1 and out.stride(1) == 1, "unit inner strides required")
    _req(out.dtype in (F16, F32), "out must be fp16 or fp32")
    if bias is not None:
        _req(bias.dtype == F32 and bias.numel() == N and bias.is_contiguous(), "bias fp32 [N]")
    for r in (res1, res2):
        if r is not None:
            _req(r.shape == (M, N), "residual shape")
    d = GemmDesc()
    if rope is not None:
        pos, cols, base = rope[:3]
        hd = rope[3] if len(rope) > 3 else 64
        _req(pos.dtype == torch.int64 and pos.is_contiguous() and pos.numel() == 2 * M and pos.is_cuda, "rope positions int64 [M,2]")
        _req(out.dtype == F16 and act == 0 and res1 is None and res2 is None and (hd == 64 or (hd == 48 and not pair)) and cols % hd == 0
             and 0 < cols <= N and N % hd == 0 and tile != 16, "fused rope: fp16 output, no activation / residual, whole heads of 64 or 48")
        tab = rope_table(out.device, base, 1.0, hd)
        d.rope_pos, d.rope_table, d.rope_cols, d.rope_pmin, d.rope_npos, d.rope_d = pos.data_ptr(), tab.data_ptr(), int(cols), ROPE_PMIN, ROPE_NPOS, hd
    _fill_common(d, A, W, out, bias, res1, res2, act, tile)
    d.M, d.N, d.K, d.lda, d.ldb, d.ldc = M, N, K, A.stride(0), W.stride(0), out.stride(0)
    if ln is not None:
        st, cs, eps = ln
        _cuda(st, cs)
        _req(K <= LN_FOLD_MAX_K, f"LayerNorm fold: K = {K} > {LN_FOLD_MAX_K}, the widest row the folded epilogue normalises (run ops.layernorm in front instead)")
        _req(K % 64 == 0 and st.dtype == F32 and st.is_contiguous() and st.numel() == M * (K // 64) * 2, f"ln stats fp32 [K/64={K // 64}, M={M}, 2]")
        _req(cs.dtype == F32 and cs.is_contiguous() and cs.numel() == N and bias is not None and tile != 16, "ln colsum fp32 [N], folded bias required")
        d.ln_stats, d.ln_colsum, d.ln_nslab, d.ln_eps = st.data_ptr(), cs.data_ptr(), K // 64, float(eps)
    if emit is not None:
        so, o16 = emit
        _cuda(so, o16)
        _req(N % 64 == 0 and so.dtype == F32 and so.is_contiguous() and so.numel() == M * (N // 64) * 2, f"stats_out fp32 [N/64={N // 64}, M={M}, 2]")
        _req(o16.dtype == F16 and o16.shape == (M, N) and o16.stride(1) == 1, "out16 fp16 [M,N]")
        _req(out.dtype == F32 and res1 is not None and res1.dtype == F32 and res2 is None and act == 0 and tile != 16, "emit: fp32 output with an fp32 residual")
        d.stats_out, d.out16, d.ld16 = so.data_ptr(), o16.data_ptr(), o16.stride(0)
    return d


def linear(A, W, out, bias=None, act=0, res1=None, res2=None, tile=0, rope=None, ln=None, emit=None):
    """out[M,N] = act(A[M,K] @ W[N,K]^T + bias) (+res1)(+res2).  A,W fp16; out fp16|fp32 (any row stride).
    rope = (positions int64 [M,2] contiguous, cols, base[, head_dim = 64 | 48]): 2-D RoPE fused on the first `cols` columns
    (48-wide heads use the 128 x 192 tile).
    LayerNorm fold (include/cut3r_hip.h, cut3r_gemm_desc):
      ln = (stats fp32 [K/64, M, 2] (slab-major), colsum fp32 [N], eps): A holds the UN-normalised rows (fp16 copy of the residual stream), W the
           gamma-folded panel, bias the folded d; the epilogue normalises per row from the slab statistics;
      emit = (stats_out fp32 [N/64, M, 2], out16 fp16 [M, N]): an fp32 + fp32-residual GEMM also writes the fp16 copy of its
           output and the slab statistics the next consumer needs."""
    if tile == 16 and A.dim() == 2 and A.shape[0] > 64:           # skinny kernel: 64 rows per launch (row results do not depend on the chunking)
        M = A.shape[0]
        _linear_desc(A, W, out, bias, act, res1, tile, rope, res2=res2)       # the whole problem's checks (kept as it is: the chunks run without ln / emit)
        for m0 in range(0, M, 64):
            sl = slice(m0, min(M, m0 + 64))
            linear(A[sl], W, out[sl], bias, act, None if res1 is None else res1[sl], None if res2 is None else res2[sl], tile=16)
        return out
    d = _linear_desc(A, W, out, bias, act, res1, tile, rope, ln, emit, res2=res2)
    _launch(d, f"cut3r_gemm_f16 M={d.M} N={d.N} K={d.K}")
    return out


def linear_pair(p0, p1, act=0, tile=0):
    """Two independent linears in ONE launch (cut3r_gemm_f16_pair): p = (A [M,K], W [N,K], out [M,N], bias | None, res1 | None[, extras]) with
    the same N and K; rows are bit-identical to ops.linear.  The decoder runs its state-side and image-side projection of a layer this
    way.  extras: dict with any of rope / ln / emit as in ops.linear (per problem).  `tile` is written into both descriptors; the C side reads
    the first one's only (both problems run the same tile kernel)."""
    x0 = p0[5] if len(p0) > 5 and p0[5] else {}
    x1 = p1[5] if len(p1) > 5 and p1[5] else {}
    d0 = _linear_desc(p0[0], p0[1], p0[2], p0[3], act, p0[4], tile, pair=True, **x0)
    d1 = _linear_desc(p1[0], p1[1], p1[2], p1[3], act, p1[4], tile, pair=True, **x1)
    _req(d0.N == d1.N and d0.K == d1.K, "pair: same N and K")
    lib = _lib.load()
    check(lib.cut3r_gemm_f16_pair(C.byref(d0), C.byref(d1), _stream()), f"cut3r_gemm_f16_pair M={d0.M}+{d1.M} N={d0.N} K={d0.K}")


def linear_batched(A, W, out, bias=None, act=0, res1=None, tile=0):
    """Z independent problems in ONE launch (blockIdx.z): A [Z,M,K], W [Z,N,K] fp16; out [Z,M,N] fp16|fp32;
    bias [Z,N] fp32; res1 [Z,M,N].  Used to run the state-side and image-side decoder GEMMs of a layer together."""
    _cuda(A, W, out, bias, res1)
    _req(A.dtype == F16 and W.dtype == F16 and A.dim() == 3 and W.dim() == 3 and out.dim() == 3, "3-D fp16 operands")
    Z, M, K = A.shape
    N = W.shape[1]
    _req(W.shape == (Z, N, K) and out.shape == (Z, M, N), "batched shapes")
    _req(A.stride(2) == 1 and W.stride(2) == 1 and out.stride(2) == 1, "unit inner strides")
    d = GemmDesc()
    _fill_common(d, A, W, out, bias, None, None, act, tile)
    if bias is not None:
        _req(bias.dtype == F32 and bias.shape == (Z, N) and bias.stride(1) == 1, "bias [Z,N]")
        d.strideBias = bias.stride(0)
    if res1 is not None:
        _req(res1.shape == (Z, M, N) and res1.stride(2) == 1 and res1.dtype in (F16, F32), "res1 [Z,M,N]")
        d.res1, d.ldr1, d.res1_f16, d.strideR1 = res1.data_ptr(), res1.stride(1), int(res1.dtype == F16), res1.stride(0)
    d.M, d.N, d.K, d.lda, d.ldb, d.ldc = M, N, K, A.stride(1), W.stride(1), out.stride(1)
    d.batch, d.strideA, d.strideB, d.strideC = Z, A.stride(0), W.stride(0), out.stride(0)
    _launch(d, f"cut3r_gemm_f16 batched Z={Z} M={M} N={N} K={K}")
    return out


def conv3x3_nhwc(x, Wk, out, bias=None, stride=1, relu_in=False, act=0, res1=None, res2=None, tile=0):
    """3x3 / pad 1 convolution as implicit GEMM.  x fp16 [B,H,W,Cin] contiguous; Wk fp16 [Cout, 9*Cin] ordered
    (ky,kx,ci); out fp16 [B,Ho,Wo,Cout] contiguous."""
    _cuda(x, Wk, out, bias, res1, res2)
    _req(x.dtype == F16 and x.dim() == 4 and x.is_contiguous(), "x must be contiguous NHWC fp16")
    Bn, H, Wd, Cin = x.shape
    Cout = Wk.shape[0]
    Ho, Wo = (H + 2 - 3) // stride + 1, (Wd + 2 - 3) // stride + 1
    _req(Wk.dtype == F16 and Wk.shape == (Cout, 9 * Cin) and Wk.is_contiguous(), "Wk must be fp16 [Cout, 9*Cin]")
    _req(out.shape == (Bn, Ho, Wo, Cout) and out.is_contiguous() and out.dtype in (F16, F32), "bad conv output")
    M = Bn * Ho * Wo
    r1 = res1.reshape(M, Cout) if res1 is not None else None
    r2 = res2.reshape(M, Cout) if res2 is not None else None
    d = GemmDesc()
    _fill_common(d, x, Wk, out, bias, r1, r2, act, tile)
    d.M, d.N, d.K, d.lda, d.ldb, d.ldc = M, Cout, 9 * Cin, Cin, 9 * Cin, Cout
    d.conv_k, d.H, d.W, d.Cin, d.conv_stride, d.Ho, d.Wo, d.relu_in = 3, H, Wd, Cin, stride, Ho, Wo, int(relu_in)
    _launch(d, f"cut3r_gemm_f16(conv3x3) M={M} N={Cout} K={9*Cin}")
    return out


def conv_transpose_nhwc(x, Wt, out, bias, s):
    """ConvTranspose2d(kernel == stride == s).  x fp16 [B,H,W,Cin]; Wt fp16 [s*s*Cout, Cin] ordered (i,j,co);
    out fp16 [B,H*s,W*s,Cout]."""
    _cuda(x, Wt, out, bias)
    Bn, H, Wd, Cin = x.shape
    Cout = Wt.shape[0] // (s * s)
    _req(x.dtype == F16 and x.is_contiguous() and Wt.dtype == F16 and Wt.is_contiguous(), "fp16 contiguous inputs")
    _req(Wt.shape == (s * s * Cout, Cin) and out.shape == (Bn, H * s, Wd * s, Cout) and out.is_contiguous(), "bad shapes")
    _req(bias is not None and bias.numel() == Cout, "bias [Cout]")
    d = GemmDesc()
    _fill_common(d, x, Wt, out, bias, None, None, 0, 0)
    d.M, d.N, d.K, d.lda, d.ldb, d.ldc = Bn * H * Wd, s * s * Cout, Cin, Cin, Cin, Cout
    d.shuf, d.shuf_cout, d.shuf_Hin, d.shuf_Win = s, Cout, H, Wd
    _launch(d, "cut3r_gemm_f16(convT)")
    return out


def gemv(X, W, out, bias=None, act=0, res=None, silu_in=False):
    """out[M,N] = act(X[M,K] @ W[N,K]^T + bias) (+res); X,out fp32, W fp16, M <= 64."""
    _cuda(X, W, out, bias, res)
    _req(X.dtype == F32 and W.dtype == F16 and out.dtype == F32, "dtypes: X fp32, W fp16, out fp32")
    M, K = X.shape
    N = W.shape[0]
    _req(W.shape[1] == K and out.shape == (M, N) and X.stride(1) == 1 and W.stride(1) == 1 and out.stride(1) == 1, "shapes")
    if bias is not None:
        _req(bias.dtype == F32 and bias.numel() == N, "bias")
    if res is not None:
        _req(res.dtype == F32 and res.shape == (M, N) and res.stride(1) == 1, "res")
    _req(act in (0, 1), f"gemv: act must be 0 (none) or 1 (GELU), got {act} (the kernel has no ReLU)")
    _req(M <= 64 and K % 8 == 0 and W.stride(0) % 8 == 0, "gemv: M <= 64, K and the row stride of W multiples of 8")
    _aligned(16, W=W)
    lib = _lib.load()
    check(lib.cut3r_gemv_f16w(_p(X), X.stride(0), _p(W), W.stride(0), _p(bias), _p(out), out.stride(0), M, N, K, act,
                              _p(res), res.stride(0) if res is not None else 0, int(silu_in), _stream()), "cut3r_gemv_f16w")
    return out


# ------------------------------------------------------------------------------------------------ attention
def attention_kernel_for(B, H, Nq, D):
    """The kernel instance `attention` launches for this problem: 100 * pipelined + waves per workgroup (104, 4 or 2; 0 = none)."""
    return _lib.load().cut3r_attention_kernel_for(int(B), int(H), int(Nq), int(D))


def attention(q, k, v, out, scale):
    """q [B,Nq,H,D], k/v [B,Nk,H,D] fp16 views with unit d-stride and head stride D; out [B,Nq,H,D] fp16."""
    _cuda(q, k, v, out)
    B, Nq, H, D = q.shape
    Nk = k.shape[1]
    for t in (q, k, v, out):
        _req(t.dtype == F16 and t.dim() == 4 and t.stride(3) == 1 and t.stride(2) == D, "attention operands: fp16 (B,N,H,D) views")
    _req(k.shape == (B, Nk, H, D) and v.shape == (B, Nk, H, D) and out.shape == (B, Nq, H, D), "attention shapes")
    _req(D in (16, 32, 48, 64, 128), f"unsupported head dim {D}")
    _req(0.0 < float(scale) < float("inf"), f"attention scale must be finite and > 0, got {scale}")
    lib = _lib.load()
    check(lib.cut3r_attention_f16(_p(q), _p(k), _p(v), _p(out), B, H, Nq, Nk, D, q.stride(0), q.stride(1), k.stride(0),
                                  k.stride(1), v.stride(0), v.stride(1), out.stride(0), out.stride(1), float(scale),
                                  _stream()), f"cut3r_attention_f16 B={B} H={H} Nq={Nq} Nk={Nk} D={D}")
    return out


def attention_one_key(v, out):
    """`attention` over ONE key without the work: v [B,1,H,D], out [B,Nq,H,D] fp16 views as in `attention`; every query row of (b, h) becomes
    v[b, 0, h, :] -- the softmax of one score is 1, and these are the bits `attention` writes (finite q and k)."""
    _cuda(v, out)
    for t in (v, out):
        _req(t.dtype == F16 and t.dim() == 4 and t.stride(3) == 1 and t.stride(2) == t.shape[3], "attention operands: fp16 (B,N,H,D) views")
    B, Nq, H, D = out.shape
    _req(v.shape == (B, 1, H, D), "attention_one_key: v [B,1,H,D]")
    _req(D % 8 == 0 and D <= 256, f"unsupported head dim {D}")
    _aligned(16, v=v, out=out)
    lib = _lib.load()
    check(lib.cut3r_attention_one_key_f16(_p(v), _p(out), B, H, Nq, D, v.stride(0), v.stride(1), out.stride(0), out.stride(1), _stream()),
          f"cut3r_attention_one_key_f16 B={B} H={H} Nq={Nq} D={D}")
    return out


# ------------------------------------------------------------------------------------------------ helpers
def im2col_patch(img, P, out):
    _cuda(img, out)
    _req(img.dim() == 4 and img.is_contiguous() and img.dtype in (F32, torch.uint8), "img [B,C,H,W] fp32|u8 contiguous")
    B, Cc, H, W = img.shape
    _req(out.dtype == F16 and out.is_contiguous() and out.shape == (B * (H // P) * (W // P), Cc * P * P), "im2col out shape")
    lib = _lib.load()
    check(lib.cut3r_im2col_patch(_p(img), int(img.dtype == torch.uint8), B, Cc, H, W, P, _p(out), _stream()), "cut3r_im2col_patch")
    return out


def cast_f16(x, out):
    _cuda(x, out)
    _req(x.dtype == F32 and out.dtype == F16 and x.shape == out.shape and x.dim() == 2, "cast: 2-D fp32 -> fp16")
    _req(x.stride(1) == 1 and out.stride(1) == 1, "unit inner stride")
    _aligned(16, x=x)
    _aligned(8, out=out)
    lib = _lib.load()
    check(lib.cut3r_cast_f32_f16(_p(x), x.stride(0), _p(out), out.stride(0), x.shape[0], x.shape[1], _stream()), "cut3r_cast_f32_f16")
    return out


def colmean(x, out):
    _cuda(x, out)
    _req(x.dtype == F32 and x.dim() == 2 and x.stride(1) == 1 and out.dtype == F32 and out.numel() == x.shape[1], "colmean")
    lib = _lib.load()
    check(lib.cut3r_colmean(_p(x), x.stride(0), x.shape[0], x.shape[1], _p(out), _stream()), "cut3r_colmean")
    return out


def colmean_batched(x, out):
    """x fp32 [B,M,C] (any batch / row stride, unit inner stride) -> out fp32 [B,C]: per-matrix column means, one launch"""
    _cuda(x, out)
    _req(x.dtype == F32 and x.dim() == 3 and x.stride(2) == 1 and out.dtype == F32 and out.shape == (x.shape[0], x.shape[2]) and out.stride(1) == 1,
         "colmean_batched")
    lib = _lib.load()
    check(lib.cut3r_colmean_batched(_p(x), x.shape[0], x.stride(0), x.stride(1), x.shape[1], x.shape[2], _p(out), out.stride(0), _stream()),
          "cut3r_colmean_batched")
    return out


def upsample2x(x, out):
    _cuda(x, out)
    B, H, W, Cc = x.shape
    _req(x.dtype == F16 and x.is_contiguous() and out.dtype == F16 and out.is_contiguous() and out.shape == (B, 2 * H, 2 * W, Cc), "upsample2x")
    _aligned(16, x=x, out=out)
    lib = _lib.load()
    check(lib.cut3r_upsample2x_nhwc(_p(x), _p(out), B, H, W, Cc, _stream()), "cut3r_upsample2x_nhwc")
    return out


def dpt_final(x, w, b, mode, pts, conf=None):
    _cuda(x, w, b, pts, conf)
    P, Cin = x.shape
    nout = 4 if mode == 0 else 3
    _req(x.dtype == F16 and x.is_contiguous() and w.dtype == F32 and w.shape == (nout, Cin) and w.is_contiguous(), "dpt_final in/w")
    _req(b.dtype == F32 and b.numel() == nout and pts.dtype == F32 and pts.numel() == 3 * P and pts.is_contiguous(), "dpt_final b/pts")
    if mode == 0:
        _req(conf is not None and conf.dtype == F32 and conf.numel() == P and conf.is_contiguous(), "conf")
    _aligned(16, x=x)
    lib = _lib.load()
    check(lib.cut3r_dpt_final(_p(x), P, Cin, _p(w), _p(b), mode, _p(pts), _p(conf), _stream()), "cut3r_dpt_final")


def conv3x3_dpt_final_ok(Cin, Cout, w):
    """the shapes cut3r_conv3x3_dpt_final serves: a 3x3 convolution Cin -> 128 (Cin a power of two >= 64) and a final weight [4, 128]"""
    return Cout == 128 and Cin >= 64 and (Cin & (Cin - 1)) == 0 and tuple(w.shape) == (4, 128)


def conv3x3_dpt_final(x, Wk, bias, w, b, pts, conf):
    """3x3 / pad 1 / stride 1 convolution + ReLU (head.2), final 1x1 convolution (head.4) and the point / confidence activations in
    ONE launch: the bits of conv3x3_nhwc(act=2) followed by dpt_final(mode 0), without the fp16 [B,H,W,128] tensor in between.
    x fp16 [B,H,W,Cin] contiguous; Wk fp16 [128, 9*Cin]; bias fp32 [128]; w fp32 [4,128]; b fp32 [4]; pts fp32 [B,H,W,3] and
    conf fp32 [B,H,W]: every view contiguous, any stride between views (a slice of a larger tensor)."""
    _cuda(x, Wk, bias, w, b, pts, conf)
    _req(x.dtype == F16 and x.dim() == 4 and x.is_contiguous(), "x must be contiguous NHWC fp16")
    Bn, H, Wd, Cin = x.shape
    _req(Wk.dtype == F16 and Wk.dim() == 2 and Wk.shape[1] == 9 * Cin and Wk.is_contiguous(), "Wk must be fp16 [Cout, 9*Cin]")
    Cout = Wk.shape[0]
    _req(w.dtype == F32 and w.dim() == 2 and w.is_contiguous() and conv3x3_dpt_final_ok(Cin, Cout, w), "conv3x3_dpt_final serves Cin = 2^k >= 64, Cout = 128, w [4,128]")
    _req(bias is not None and bias.dtype == F32 and bias.numel() == Cout and bias.is_contiguous(), "conv3x3_dpt_final bias")
    _req(b.dtype == F32 and b.numel() == 4 and b.is_contiguous(), "conv3x3_dpt_final b")
    for t, shape, per_view in ((pts, (Bn, H, Wd, 3), H * Wd * 3), (conf, (Bn, H, Wd), H * Wd)):
        _req(t.dtype == F32 and tuple(t.shape) == shape and Bn > 0 and t[0].is_contiguous() and (Bn == 1 or t.stride(0) >= per_view),
             "conv3x3_dpt_final destinations: fp32 [B,H,W,3] / [B,H,W], contiguous views that do not overlap")
    M = Bn * H * Wd
    d = GemmDesc()
    d.A, d.B, d.bias = x.data_ptr(), Wk.data_ptr(), bias.data_ptr()
    d.act, d.out_f16, d.batch = 2, 1, 1
    d.M, d.N, d.K, d.lda, d.ldb, d.ldc = M, Cout, 9 * Cin, Cin, 9 * Cin, Cout
    d.conv_k, d.H, d.W, d.Cin, d.conv_stride, d.Ho, d.Wo = 3, H, Wd, Cin, 1, H, Wd
    check(_lib.load().cut3r_conv3x3_dpt_final(C.byref(d), _p(w), _p(b), 0, _p(pts), pts.stride(0) if Bn > 1 else H * Wd * 3, _p(conf),
                                              conf.stride(0) if Bn > 1 else H * Wd, _stream()),
          f"cut3r_conv3x3_dpt_final M={M} K={9*Cin}")


def postprocess_pts(raw, pos_z, pts, conf=None):
    _cuda(raw, pts, conf)
    P, nch = raw.shape
    _req(raw.dtype == F32 and raw.is_contiguous() and pts.dtype == F32 and pts.numel() == 3 * P and pts.is_contiguous(), "postprocess_pts")
    if nch == 4:
        _req(conf is not None and conf.numel() == P and conf.dtype == F32 and conf.is_contiguous(), "conf")
    lib = _lib.load()
    check(lib.cut3r_postprocess_pts(_p(raw), P, nch, int(pos_z), _p(pts), _p(conf), _stream()), "cut3r_postprocess_pts")


def postprocess_pose(raw, out):
    _cuda(raw, out)
    _req(raw.dtype == F32 and raw.is_contiguous() and raw.shape[-1] == 7 and out.shape == raw.shape and out.is_contiguous(), "pose")
    lib = _lib.load()
    check(lib.cut3r_postprocess_pose(_p(raw), raw.numel() // 7, _p(out), _stream()), "cut3r_postprocess_pose")
    return out


# ------------------------------------------------------------------------------------------------ geometry
def patch_overlap_count(feat0, feat1, thr, ws, count):
    _cuda(feat0, feat1, ws, count)
    N, Cc = feat0.shape
    _req(feat0.dtype == F32 and feat1.dtype == F32 and feat1.shape == (N, Cc) and feat0.is_contiguous() and feat1.is_contiguous(), "features fp32 [N,C]")
    _req(ws.dtype == F32 and ws.numel() >= 2 * (N - 1) * Cc + (N - 1) and count.dtype == torch.int32, "workspace/count")
    _req(float(thr) >= 0.0, "similarity threshold >= 0 (the row maxima are clamped at 0)")
    lib = _lib.load()
    check(lib.cut3r_patch_overlap(_p(feat0), _p(feat1), N, Cc, float(thr), _p(ws), _p(count), _stream()), "cut3r_patch_overlap")


def patch_overlap_chain(feat_last, feats, thr_sim, thr_ratio, forced, ws, state, counts, decisions):
    """Keyframe decisions of B consecutive tested frames on the device (motion_filter.py:98-124 without a host round trip per
    frame): feat_last [N,C], feats [B,N,C] fp32; forced: list of B bools (always-keyframe frames) or None;
    state int32[1], counts / decisions int32[B] on the device."""
    _cuda(feat_last, feats, ws, state, counts, decisions)
    B, N, Cc = feats.shape
    _req(feats.dtype == F32 and feat_last.dtype == F32 and feat_last.shape == (N, Cc) and feats.is_contiguous() and feat_last.is_contiguous(),
         "features fp32 [B,N,C] / [N,C]")
    _req(ws.dtype == F32 and ws.numel() >= (B + 1) * (N - 1) * Cc + (N - 1), "workspace of (B+1)*(N-1)*C + N-1 floats")
    _req(state.dtype == torch.int32 and counts.dtype == torch.int32 and decisions.dtype == torch.int32 and counts.numel() >= B and decisions.numel() >= B,
         "state / counts / decisions int32")
    _req(float(thr_sim) >= 0.0, "similarity threshold >= 0 (the row maxima are clamped at 0)")
    arr = (C.c_int32 * B)(*[1 if f else 0 for f in forced]) if forced is not None else None
    lib = _lib.load()
    check(lib.cut3r_patch_overlap_chain(_p(feat_last), _p(feats), B, N, Cc, float(thr_sim), float(thr_ratio), arr, _p(ws), _p(state), _p(counts),
                                        _p(decisions), _stream()), "cut3r_patch_overlap_chain")


def overlap_fwd(pm, w2c, K4, W, H, counts, P12=None, s_align=1.0, clamp_z=True):
    """counts[b] = #points of pm (optionally mapped p <- P*(s*p) first) that land inside camera b's W x H image."""
    _cuda(pm, w2c, counts)
    N = pm.numel() // 3
    B = w2c.shape[0]
    _req(pm.dtype == F32 and pm.is_contiguous() and w2c.dtype == F32 and w2c.shape == (B, 12) and w2c.is_contiguous(), "overlap_fwd inputs")
    _req(counts.dtype == torch.int32 and counts.numel() >= B, "counts int32[B]")
    arr = (C.c_float * 12)(*[float(v) for v in P12]) if P12 is not None else None
    lib = _lib.load()
    check(lib.cut3r_overlap_fwd(_p(pm), N, arr, float(s_align), _p(w2c), B, *[float(v) for v in K4], int(W), int(H),
                                int(clamp_z), _p(counts), _stream()), "cut3r_overlap_fwd")


def overlap_bwd(pms, w2c, K4, W, H, counts, B=None, N=None, grp=0, grp_stride=0):
    """counts[b] = #points of pointmap b inside the ONE camera w2c.  pms: contiguous [B,N,3]-like store; with grp > 0
    pointmap b sits at slot (b//grp)*grp_stride + b%grp of a [slots, N, 3] store (keyframe order of submap_ds)."""
    _cuda(pms, w2c, counts)
    if B is None:
        B = pms.shape[0]
    if N is None:
        N = pms[0].numel() // 3
    _req(pms.dtype == F32 and pms.is_contiguous() and w2c.dtype == F32 and w2c.numel() == 12 and w2c.is_contiguous(), "overlap_bwd inputs")
    nslots = pms.numel() // (3 * N)
    last = (B - 1) if grp == 0 else ((B - 1) // grp) * grp_stride + (B - 1) % grp
    _req(B >= 1 and last < nslots, "overlap_bwd: pointmap store too small for B")
    _req(counts.dtype == torch.int32 and counts.numel() >= B, "counts int32[B]")
    lib = _lib.load()
    check(lib.cut3r_overlap_bwd(_p(pms), B, N, int(grp), int(grp_stride), _p(w2c), *[float(v) for v in K4], int(W), int(H),
                                _p(counts), _stream()), "cut3r_overlap_bwd")


def align_view(pts, conf, P12, s, ds, pm_ds, conf_ds, depth):
    _cuda(pts, conf, pm_ds, conf_ds, depth)
    H, W = conf.shape[-2:]
    _req(pts.dtype == F32 and pts.is_contiguous() and pts.numel() == H * W * 3 and conf.dtype == F32 and conf.is_contiguous(), "align inputs")
    _req(pm_ds.is_contiguous() and pm_ds.numel() == (H // ds) * (W // ds) * 3 and conf_ds.is_contiguous() and conf_ds.numel() == (H // ds) * (W // ds), "align ds outputs")
    _req(depth.is_contiguous() and depth.numel() == H * W and depth.dtype == F32, "depth output")
    arr = (C.c_float * 12)(*[float(v) for v in P12])
    lib = _lib.load()
    check(lib.cut3r_align_view(_p(pts), _p(conf), H, W, arr, float(s), int(ds), _p(pm_ds), _p(conf_ds), _p(depth), _stream()), "cut3r_align_view")


def window_update(pts, conf, P12s, s, ds, pm_ds, conf_ds, depth, store, w2c, t0, first, K4, counts, grp=5, grp_stride=6,
                  w2c_new=None, lsum_reset=None):
    """Whole-window align + overlap counts (cut3r_window_update).  pts [V,H,W,3], conf [V,H,W]; pm_ds [V,h,w,3], conf_ds [V,h,w],
    depth [V,H,W] are the window's consecutive store slots; store = the full [submaps,6,h,w,3] pointmap store; w2c [>=t0+V,12];
    counts int32 [V,2,ldc] receives forward (row 0) / backward (row 1) counts of keyframes t0+v >= first.  w2c_new: V*12 host
    floats written to rows t0.. of w2c by the kernel; lsum_reset: fp64[1] accumulator zeroed for the next window."""
    _cuda(pts, conf, pm_ds, conf_ds, depth, store, w2c, counts)
    V, H, W = conf.shape
    h, w = H // ds, W // ds
    _req(pts.dtype == F32 and pts.is_contiguous() and pts.shape == (V, H, W, 3) and conf.dtype == F32 and conf.is_contiguous(), "window inputs")
    _req(1 <= V <= 6 and len(P12s) == V * 12, "V <= 6 views with 12 floats each")
    _req(pm_ds.is_contiguous() and pm_ds.numel() == V * h * w * 3 and conf_ds.is_contiguous() and conf_ds.numel() == V * h * w, "ds outputs")
    _req(depth.is_contiguous() and depth.numel() == V * H * W and depth.dtype == F32, "depth rows")
    _req(store.dtype == F32 and store.is_contiguous() and w2c.dtype == F32 and w2c.is_contiguous() and w2c.shape[0] >= t0 + V and w2c.shape[1] == 12, "store / w2c")
    last = t0 + V - 1
    nslots = store.numel() // (3 * h * w)
    _req(last < 1 or ((last - 1) // grp) * grp_stride + (last - 1) % grp < nslots, "pointmap store too small")
    ldc = counts.shape[-1]
    _req(counts.dtype == torch.int32 and counts.is_contiguous() and counts.shape == (V, 2, ldc) and ldc >= t0 + V, "counts int32 [V,2,ldc]")
    arr = (C.c_float * (12 * V))(*[float(v) for v in P12s])
    arr_w = None
    if w2c_new is not None:
        _req(len(w2c_new) == 12 * V, "w2c_new: V*12 floats")
        arr_w = (C.c_float * (12 * V))(*[float(v) for v in w2c_new])
    if lsum_reset is not None:
        _cuda(lsum_reset)
        _req(lsum_reset.dtype == torch.float64 and lsum_reset.numel() == 1, "lsum_reset fp64[1]")
    lib = _lib.load()
    check(lib.cut3r_window_update(_p(pts), _p(conf), V, H, W, arr, float(s), int(ds), _p(pm_ds), _p(conf_ds), _p(depth), _p(store),
                                  int(grp), int(grp_stride), _p(w2c), arr_w, int(t0), int(first), *[float(v) for v in K4], _p(counts), ldc,
                                  _p(lsum_reset), _stream()), "cut3r_window_update")


def logdepth_sum(prev_depth, pts, out):
    _cuda(prev_depth, pts, out)
    n = prev_depth.numel()
    _req(prev_depth.dtype == F32 and prev_depth.is_contiguous() and pts.dtype == F32 and pts.is_contiguous() and pts.numel() == 3 * n, "logdepth inputs")
    _req(out.dtype == torch.float64 and out.numel() == 1, "out fp64[1]")
    lib = _lib.load()
    check(lib.cut3r_logdepth_sum(_p(prev_depth), _p(pts), n, _p(out), _stream()), "cut3r_logdepth_sum")


def logdepth_accum(prev_depth, pts, out):
    """out += sum(log prev - log z); out must hold 0 beforehand (window_update's lsum_reset keeps it so)."""
    _cuda(prev_depth, pts, out)
    n = prev_depth.numel()
    _req(prev_depth.dtype == F32 and prev_depth.is_contiguous() and pts.dtype == F32 and pts.is_contiguous() and pts.numel() == 3 * n, "logdepth inputs")
    _req(out.dtype == torch.float64 and out.numel() == 1, "out fp64[1]")
    lib = _lib.load()
    check(lib.cut3r_logdepth_accum(_p(prev_depth), _p(pts), n, _p(out), _stream()), "cut3r_logdepth_accum")


def remap_linear_u8(src_hwc, map_ix, map_iy, out=None):
    """cv2.remap(INTER_LINEAR, BORDER_CONSTANT 0) with a fixed-point map (1/32 pixel): src uint8 [H,W,C]; map_ix/map_iy int32 [Ho,Wo]"""
    _cuda(src_hwc, map_ix, map_iy, out)
    _req(src_hwc.dtype == torch.uint8 and src_hwc.dim() == 3 and src_hwc.is_contiguous(), "src uint8 [H,W,C] contiguous")
    H, W, Cc = src_hwc.shape
    _req(map_ix.dtype == torch.int32 and map_iy.dtype == torch.int32 and map_ix.shape == map_iy.shape and map_ix.dim() == 2
         and map_ix.is_contiguous() and map_iy.is_contiguous(), "maps int32 [Ho,Wo]")
    Ho, Wo = map_ix.shape
    if out is None:
        out = torch.empty((Ho, Wo, Cc), dtype=torch.uint8, device=src_hwc.device)
    _req(out.dtype == torch.uint8 and out.shape == (Ho, Wo, Cc) and out.is_contiguous(), "out uint8 [Ho,Wo,C]")
    lib = _lib.load()
    check(lib.cut3r_remap_linear_u8(_p(src_hwc), H, W, Cc, _p(map_ix), _p(map_iy), _p(out), Ho, Wo, _stream()), "cut3r_remap_linear_u8")
    return out


def resize_linear_u8(img_hwc, H1, W1, chw_out=True, out=None):
    """cv2.resize(img, (W1, H1)) (INTER_LINEAR, u8) on the GPU.  img_hwc u8 [H0,W0,C] -> u8 [C,H1,W1] (or [H1,W1,C]); `out`: write
    there (e.g. straight into the keyframe store) instead of a new tensor."""
    _cuda(img_hwc, out)
    _req(img_hwc.dtype == torch.uint8 and img_hwc.dim() == 3 and img_hwc.is_contiguous() and img_hwc.shape[2] <= 4, "u8 [H,W,C<=4] contiguous")
    H0, W0, Cc = img_hwc.shape
    shape = (Cc, int(H1), int(W1)) if chw_out else (int(H1), int(W1), Cc)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=img_hwc.device)
    _req(out.dtype == torch.uint8 and tuple(out.shape) == shape and out.is_contiguous(), f"out u8 {shape} contiguous")
    lib = _lib.load()
    check(lib.cut3r_resize_linear_u8(_p(img_hwc), H0, W0, Cc, _p(out), int(H1), int(W1), int(bool(chw_out)), _stream()), "cut3r_resize_linear_u8")
    return out


# ------------------------------------------------------------------------------------------------ loop closure
LC_GROUPS = {"se3": (6, ""), "sim3": (7, "_sim3")}          # group -> (tangent dimension, suffix of the C entry points)


def _lc_group(group):
    _req(group in LC_GROUPS, f"group: one of {sorted(LC_GROUPS)}, not {group!r}")
    return LC_GROUPS[group]


def lc_optimize(submaps, mask, cur, cur_lc, iters, lr=5e-4, return_loss=False, group="se3"):
    """Fused Adam over per-submap se(3) corrections (track_backend.py:256-299).  submaps: [B,6,h,w,3] fp32 contiguous
    (slot 0 = first, slot 5 = last pointmap of each submap); mask: bool/uint8 [B-1,h*w] or None; cur, cur_lc: [h*w,3].
    Returns (xi [B,6], T [B,3,4]) (+ per-iteration loss).  group="sim3": the same objective over similarities, xi [B,7] =
    [tau, phi, sigma], T = [e^sigma R | W tau]."""
    K, sfx = _lc_group(group)
    _cuda(submaps, mask, cur, cur_lc)
    _req(submaps.dtype == F32 and submaps.dim() == 5 and submaps.is_contiguous() and submaps.shape[1] == 6 and submaps.shape[4] == 3, "submaps [B,6,h,w,3]")
    B = submaps.shape[0]
    N = submaps.shape[2] * submaps.shape[3]
    _req(B >= 2, "need at least two submaps")
    cur = cur.reshape(-1, 3).contiguous()
    cur_lc = cur_lc.reshape(-1, 3).contiguous()
    _req(cur.shape == (N, 3) and cur_lc.shape == (N, 3) and cur.dtype == F32 and cur_lc.dtype == F32, "cur / cur_lc [N,3] fp32")
    dev = submaps.device
    if mask is not None:
        mask = mask.reshape(B - 1, N).to(torch.uint8).contiguous()
        n_masked = int(mask.sum().item())
    else:
        n_masked = (B - 1) * N
    lib = _lib.load()
    xi = torch.zeros(B, K, device=dev)
    m, v = torch.zeros_like(xi), torch.zeros_like(xi)
    T = torch.eye(4, device=dev)[:3].reshape(1, 12).repeat(B, 1).contiguous()
    ws = torch.empty(lib.cut3r_lc_workspace_floats(B, N), device=dev)
    loss = torch.zeros(max(iters, 1), device=dev) if return_loss else None
    first = submaps
    last_ptr = C.c_void_p(submaps.data_ptr() + 5 * N * 3 * 4)
    fn = "cut3r_lc_optimize" + sfx
    check(getattr(lib, fn)(_p(first), last_ptr, 6 * N * 3, _p(mask), _p(cur), _p(cur_lc), B, N, n_masked, int(iters), float(lr),
                           _p(xi), _p(m), _p(v), _p(T), _p(ws), _p(loss), _stream()), fn)
    T = T.view(B, 3, 4)
    return (xi, T, loss) if return_loss else (xi, T)


def lc_optimize_terms(terms, P, N, iters, lr=5e-4, return_loss=False, group="se3"):
    """Fused Adam over P-1 se(3) vectors for a list of L1 terms (track_backend.py:400-461).  terms: list of
    (a [N,3] fp32 cuda, ia, c [N,3] fp32 cuda, ic, weight, mask uint8 [N] | None) with transform indices in [0, P), 0 = the
    fixed identity.  Returns (xi [P,6], T [P,3,4]) (+ per-iteration loss).  group="sim3": xi [P,7], as in lc_optimize."""
    K, sfx = _lc_group(group)
    _req(len(terms) >= 1 and P >= 2, "at least one term and one free transform")
    keep = []
    arr = (_lib.LcTerm * len(terms))()
    dev = terms[0][0].device
    for t, (a, ia, c, ic, w, mask) in enumerate(terms):
        _cuda(a, c, mask)
        _req(a.dtype == F32 and c.dtype == F32 and a.is_contiguous() and c.is_contiguous() and a.numel() == 3 * N and c.numel() == 3 * N,
             "term operands: contiguous fp32 [N,3]")
        _req(0 <= ia < P and 0 <= ic < P, "transform index out of range")
        if mask is not None:
            _req(mask.dtype == torch.uint8 and mask.is_contiguous() and mask.numel() == N, "mask uint8 [N]")
        arr[t].a, arr[t].c, arr[t].mask = a.data_ptr(), c.data_ptr(), (mask.data_ptr() if mask is not None else None)
        arr[t].ia, arr[t].ic, arr[t].w, arr[t].pad = int(ia), int(ic), float(w), 0
        keep.append((a, c, mask))
    raw = bytes(arr)
    terms_dev = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    lib = _lib.load()
    xi = torch.zeros(P, K, device=dev)
    m, v = torch.zeros_like(xi), torch.zeros_like(xi)
    T = torch.eye(4, device=dev)[:3].reshape(1, 12).repeat(P, 1).contiguous()
    ws = torch.empty(lib.cut3r_lc_workspace_floats(len(terms), N), device=dev)
    loss = torch.zeros(max(iters, 1), device=dev) if return_loss else None
    fn = "cut3r_lc_optimize_terms" + sfx
    check(getattr(lib, fn)(_p(terms_dev), len(terms), int(P), int(N), int(iters), float(lr), _p(xi), _p(m), _p(v), _p(T), _p(ws),
                           _p(loss), _stream()), fn)
    T = T.view(P, 3, 4)
    return (xi, T, loss) if return_loss else (xi, T)


def transform_submaps(submaps, T):
    """in place: every point of submap b <- T[b] (3x4) applied (track_backend.py:301-310)."""
    _cuda(submaps, T)
    B = submaps.shape[0]
    _req(submaps.dtype == F32 and submaps.is_contiguous() and T.dtype == F32 and T.is_contiguous() and T.numel() == 12 * B, "transform_submaps")
    per = submaps[0].numel() // 3
    lib = _lib.load()
    check(lib.cut3r_transform_submaps(_p(submaps), _p(T), B, per, _stream()), "cut3r_transform_submaps")
    return submaps


def scale_planes(planes, scale):
    """in place: plane i of `planes` [n, ...] fp32 <- scale[i] * plane i (one fp32 multiply per element, one launch): the depth maps of
    the keyframes a sim(3) loop correction rescales."""
    _cuda(planes, scale)
    n = planes.shape[0]
    _req(planes.dtype == F32 and planes.is_contiguous() and planes.dim() >= 1 and 0 < n <= 65535 and planes.numel() > 0, "planes: contiguous fp32 [n<=65535, ...]")
    _req(scale.dtype == F32 and scale.is_contiguous() and scale.numel() == n, "scale: contiguous fp32 [n]")
    lib = _lib.load()
    check(lib.cut3r_scale_planes(_p(planes), _p(scale), n, planes.numel() // n, _stream()), "cut3r_scale_planes")
    return planes


# ------------------------------------------------------------------------------------------------ TSDF fusion / mesh extraction
TSDF_MAX_VIEWS = 16


def _tsdf_planes(tsdf, weight, color):
    """(tsdf [Z,Y,X], weight [Z,Y,X], color [3,Z,Y,X]) fp32 contiguous GPU planes -> (X, Y, Z)"""
    _cuda(tsdf, weight, color)
    _req(tsdf.dim() == 3 and tsdf.dtype == F32 and tsdf.is_contiguous(), "tsdf: contiguous fp32 [Z,Y,X]")
    Z, Y, X = tsdf.shape
    _req(X > 0 and Y > 0 and Z > 0 and X * Y * Z < 2 ** 31, "TSDF grid: dims > 0 and X*Y*Z < 2^31")
    _req(weight.shape == tsdf.shape and weight.dtype == F32 and weight.is_contiguous(), "weight: contiguous fp32 like tsdf")
    _req(color.shape == (3, Z, Y, X) and color.dtype == F32 and color.is_contiguous(), "color: contiguous fp32 [3,Z,Y,X]")
    return X, Y, Z


def _tsdf_views(what, depth, pose, pose_name, K, voxel, trunc, max_views=None, rgb=None, conf=None, conf_ds=1):
    """the views of a TSDF launch: depth [B,H,W], pose (w2c or c2w rows) [B,12], K [B,4] fp32, rgb u8 [B,3,H,W] or None, conf fp32 [B,h,w] or
    None, all contiguous on the GPU -> (B, H, W, ch, cw).  max_views: the limit on B of one launch; None: any B with B*H*W < 2^31."""
    _cuda(depth, pose, K, rgb, conf)
    _req(depth.dim() == 3 and depth.dtype == F32 and depth.is_contiguous(), "depth: contiguous fp32 [B,H,W]")
    B, H, W = depth.shape
    if max_views is None:
        _req(B >= 1 and H > 0 and W > 0 and B * H * W < 2 ** 31, "depth: 1 .. 2^31 - 1 pixels")
    else:
        _req(1 <= B <= max_views, f"{what}: 1..{max_views} views per launch")
        _req(H > 0 and W > 0, "depth: empty image")
    _req(pose.shape == (B, 12) and pose.dtype == F32 and pose.is_contiguous(), f"{pose_name}: contiguous fp32 [B,12]")
    _req(K.shape == (B, 4) and K.dtype == F32 and K.is_contiguous(), "K: contiguous fp32 [B,4]")
    _req(float(voxel) > 0 and float(trunc) > 0, "voxel size and truncation must be > 0")
    if rgb is not None:
        _req(rgb.shape == (B, 3, H, W) and rgb.dtype == torch.uint8 and rgb.is_contiguous(), "rgb: contiguous uint8 [B,3,H,W]")
    ch = cw = 0
    if conf is not None:
        _req(conf.dim() == 3 and conf.shape[0] == B and conf.dtype == F32 and conf.is_contiguous(), "conf: contiguous fp32 [B,h,w]")
        ch, cw = conf.shape[1:]
        _req(int(conf_ds) >= 1 and ch > 0 and cw > 0, "conf: stride >= 1, non-empty")
    return B, H, W, ch, cw


def _tsdf_mesh(dev, voxel, workspace_bytes, count, emit, what, store):
    """the driver of the two extract_mesh: workspace, count + scans, one read-back of the two totals, allocate, emit.  count(ws, nbytes,
    totals) and emit(ws, nbytes, verts, cols, faces, nv, nf) return the status of the C entry points named cut3r_{what}_mesh_*; store names what is too large when no workspace fits."""
    _req(float(voxel) > 0, "voxel size must be > 0")
    nbytes = workspace_bytes()
    _req(nbytes > 0, f"{store} too large")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    check(count(_p(ws), nbytes, _p(totals)), f"cut3r_{what}_mesh_count")
    nv, nf = (int(v) for v in totals.cpu())
    _req(nv < 2 ** 31, f"mesh of {nv} vertices: int32 face indices cannot address it")
    verts = torch.empty(nv, 3, dtype=F32, device=dev)
    cols = torch.empty(nv, 3, dtype=torch.uint8, device=dev)
    faces = torch.empty(nf, 3, dtype=torch.int32, device=dev)
    check(emit(_p(ws), nbytes, _p(verts), _p(cols), _p(faces), nv, nf), f"cut3r_{what}_mesh_emit")
    return verts, cols, faces


def tsdf_integrate(tsdf, weight, color, origin, voxel, depth, w2c, K, trunc, depth_max, rgb=None, conf=None, conf_ds=1, conf_min=0.0):
    """in place: fuse B <= 16 views (VoxelBlockGrid.integrate, tsdf_integrate.py:31-62) in one launch.  depth [B,H,W] fp32 metres, w2c
    [B,12] / K [B,4] fp32 on the GPU, rgb u8 [B,3,H,W] or None, conf fp32 [B,h,w] at stride conf_ds with conf_min, or None."""
    X, Y, Z = _tsdf_planes(tsdf, weight, color)
    B, H, W, ch, cw = _tsdf_views("tsdf_integrate", depth, w2c, "w2c", K, voxel, trunc, TSDF_MAX_VIEWS, rgb, conf, conf_ds)
    lib = _lib.load()
    check(lib.cut3r_tsdf_integrate(_p(tsdf), _p(weight), _p(color), X, Y, Z, float(origin[0]), float(origin[1]), float(origin[2]),
                                   float(voxel), _p(depth), _p(rgb), _p(conf), B, H, W, ch, cw, int(conf_ds), float(conf_min), _p(w2c),
                                   _p(K), float(trunc), float(depth_max), _stream()), "cut3r_tsdf_integrate")


def tsdf_extract_mesh(tsdf, weight, color, origin, voxel, weight_threshold=1.0):
    """marching tetrahedra over the fused planes (VoxelBlockGrid.extract_triangle_mesh, tsdf_integrate.py:83-88): count, scan, one
    read-back of the two totals, emit -> (vertices fp32 [V,3], colors u8 [V,3], faces int32 [F,3]) on the GPU"""
    X, Y, Z = _tsdf_planes(tsdf, weight, color)
    lib = _lib.load()
    o = [float(v) for v in origin]
    return _tsdf_mesh(
        tsdf.device, voxel, lambda: lib.cut3r_tsdf_mesh_workspace_bytes(X, Y, Z),
        lambda ws, nbytes, totals: lib.cut3r_tsdf_mesh_count(_p(tsdf), _p(weight), X, Y, Z, float(weight_threshold), ws, nbytes, totals, _stream()),
        lambda ws, nbytes, *out: lib.cut3r_tsdf_mesh_emit(_p(tsdf), _p(color), X, Y, Z, *o, float(voxel), ws, nbytes, *out, _stream()), "tsdf",
        "TSDF grid")


# ------------------------------------------------------------------------------------------------ sparse brick TSDF volume
TSDF_BRICK = 8
TSDF_BRICK_VOXELS = TSDF_BRICK ** 3
TSDF_SPARSE_MAX_DIM = 2 ** 20           # virtual dims per axis: voxel indices stay exact in fp32
TSDF_SPARSE_MAX_TABLE = 2 ** 28         # entries of the brick table


def tsdf_brick_dims(dims):
    """(BX, BY, BZ) bricks of 8 voxels covering the virtual grid (X, Y, Z)"""
    return tuple((int(d) + TSDF_BRICK - 1) // TSDF_BRICK for d in dims)


def _tsdf_sparse_grid(dims):
    X, Y, Z = (int(d) for d in dims)
    _req(min(X, Y, Z) > 0 and max(X, Y, Z) <= TSDF_SPARSE_MAX_DIM, f"sparse TSDF grid: dims in 1..{TSDF_SPARSE_MAX_DIM} per axis")
    BX, BY, BZ = tsdf_brick_dims((X, Y, Z))
    _req(BX * BY * BZ <= TSDF_SPARSE_MAX_TABLE, f"sparse TSDF grid: more than {TSDF_SPARSE_MAX_TABLE} table entries")
    return X, Y, Z, BX * BY * BZ


def _tsdf_table(t, name, dtype, T):
    _cuda(t)
    _req(t.dtype == dtype and t.is_contiguous() and t.numel() == T, f"{name}: contiguous {dtype} with one entry per brick of the grid")


def _tsdf_pool(tsdf, weight, color, bricks, T):
    """(tsdf [nb,512], weight [nb,512], color [3,nb,512]) fp32 and bricks int32 [nb] on the GPU -> nb"""
    _cuda(tsdf, weight, color, bricks)
    _req(tsdf.dim() == 2 and tsdf.shape[1] == TSDF_BRICK_VOXELS and tsdf.dtype == F32 and tsdf.is_contiguous(), "tsdf: contiguous fp32 [nb,512]")
    nb = tsdf.shape[0]
    _req(0 < nb <= T and nb * TSDF_BRICK_VOXELS < 2 ** 31, "sparse TSDF pool: 1 .. table entries bricks, fewer than 2^31 voxels")
    _req(weight.shape == tsdf.shape and weight.dtype == F32 and weight.is_contiguous(), "weight: contiguous fp32 like tsdf")
    _req(color.shape == (3, nb, TSDF_BRICK_VOXELS) and color.dtype == F32 and color.is_contiguous(), "color: contiguous fp32 [3,nb,512]")
    _req(bricks.shape == (nb,) and bricks.dtype == torch.int32 and bricks.is_contiguous(), "bricks: contiguous int32 [nb]")
    return nb


def tsdf_sparse_mark(flags, dims, origin, voxel, depth, c2w, K, trunc, depth_max):
    """in place: flag (u8 [BZ,BY,BX], never cleared) every brick that the views can give a negative tsdf or a 26-neighbour of one.
    depth [B,H,W] fp32, c2w [B,12] camera->world rows (the inverse of the views' w2c), K [B,4], any B >= 1."""
    X, Y, Z, T = _tsdf_sparse_grid(dims)
    _tsdf_table(flags, "flags", torch.uint8, T)
    B, H, W, _, _ = _tsdf_views("tsdf_sparse_mark", depth, c2w, "c2w", K, voxel, trunc)
    lib = _lib.load()
    check(lib.cut3r_tsdf_sparse_mark(_p(flags), X, Y, Z, float(origin[0]), float(origin[1]), float(origin[2]), float(voxel), _p(depth), B, H, W,
                                     _p(c2w), _p(K), float(trunc), float(depth_max), _stream()), "cut3r_tsdf_sparse_mark")


def tsdf_sparse_assign(flags, table, dims):
    """in place: table (int32 [BZ,BY,BX]) <- the pool slot of every flagged brick, numbered by ascending brick index, -1 elsewhere;
    returns the number of flagged bricks (one read-back)"""
    X, Y, Z, T = _tsdf_sparse_grid(dims)
    _tsdf_table(flags, "flags", torch.uint8, T)
    _tsdf_table(table, "table", torch.int32, T)
    lib = _lib.load()
    nbytes = lib.cut3r_tsdf_sparse_assign_workspace_bytes(X, Y, Z)
    _req(nbytes >= 0, "sparse TSDF grid too large")
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=flags.device)
    total = torch.empty(1, dtype=torch.int64, device=flags.device)
    check(lib.cut3r_tsdf_sparse_assign(_p(flags), _p(table), X, Y, Z, _p(ws), nbytes, _p(total), _stream()), "cut3r_tsdf_sparse_assign")
    return int(total.cpu())


def tsdf_sparse_integrate(tsdf, weight, color, bricks, dims, origin, voxel, depth, w2c, K, trunc, depth_max, rgb=None, conf=None, conf_ds=1,
                          conf_min=0.0):
    """in place: tsdf_integrate over the allocated bricks of the virtual grid `dims` (B <= 16 views, one launch); the arguments of
    tsdf_integrate with the pool (tsdf [nb,512], weight, color [3,nb,512]) and its brick list in place of the planes."""
    X, Y, Z, T = _tsdf_sparse_grid(dims)
    nb = _tsdf_pool(tsdf, weight, color, bricks, T)
    B, H, W, ch, cw = _tsdf_views("tsdf_sparse_integrate", depth, w2c, "w2c", K, voxel, trunc, TSDF_MAX_VIEWS, rgb, conf, conf_ds)
    lib = _lib.load()
    check(lib.cut3r_tsdf_sparse_integrate(_p(tsdf), _p(weight), _p(color), _p(bricks), nb, X, Y, Z, float(origin[0]), float(origin[1]),
                                          float(origin[2]), float(voxel), _p(depth), _p(rgb), _p(conf), B, H, W, ch, cw, int(conf_ds),
                                          float(conf_min), _p(w2c), _p(K), float(trunc), float(depth_max), _stream()),
          "cut3r_tsdf_sparse_integrate")


def tsdf_sparse_extract_mesh(tsdf, weight, color, table, bricks, dims, origin, voxel, weight_threshold=1.0):
    """tsdf_extract_mesh over the pool: vertices in (pool voxel, direction mask) order, faces in (pool cell, tetrahedron, triangle)
    order -> (vertices fp32 [V,3], colors u8 [V,3], faces int32 [F,3]) on the GPU"""
    X, Y, Z, T = _tsdf_sparse_grid(dims)
    nb = _tsdf_pool(tsdf, weight, color, bricks, T)
    _tsdf_table(table, "table", torch.int32, T)
    lib = _lib.load()
    o = [float(v) for v in origin]
    pool = (_p(table), _p(bricks), nb, X, Y, Z)
    return _tsdf_mesh(
        tsdf.device, voxel, lambda: lib.cut3r_tsdf_sparse_mesh_workspace_bytes(nb),
        lambda ws, nbytes, totals: lib.cut3r_tsdf_sparse_mesh_count(_p(tsdf), _p(weight), *pool, float(weight_threshold), ws, nbytes, totals,
                                                                    _stream()),
        lambda ws, nbytes, *out: lib.cut3r_tsdf_sparse_mesh_emit(_p(tsdf), _p(color), *pool, *o, float(voxel), ws, nbytes, *out, _stream()),
        "tsdf_sparse", "sparse TSDF pool")


# ------------------------------------------------------------------------------------------------ live TSDF volume
TSDF_LIVE_Q = 32768                     # q = rint(t * 32768): the fixed point of a view's tsdf sample
TSDF_LIVE_MAX_VIEWS = 65535             # views that may be in at once: 65535 * 32768 < 2^31


def _tsdf_live_pool(acc, bricks, slots, T):
    """acc int32 [5,nb,512] and bricks int32 [nb] on the GPU, slots int32 [ns] (ascending, distinct, in 0..nb-1: one read-back) or None
    -> (nb, ns)"""
    _cuda(acc, bricks, slots)
    _req(acc.dim() == 3 and acc.shape[0] == 5 and acc.shape[2] == TSDF_BRICK_VOXELS and acc.dtype == torch.int32 and acc.is_contiguous(),
         "acc: contiguous int32 [5,nb,512]")
    nb = acc.shape[1]
    _req(0 < nb <= T and nb * TSDF_BRICK_VOXELS < 2 ** 31, "live TSDF pool: 1 .. table entries bricks, fewer than 2^31 voxels")
    _req(bricks.shape == (nb,) and bricks.dtype == torch.int32 and bricks.is_contiguous(), "bricks: contiguous int32 [nb]")
    if slots is None:
        return nb, 0
    _req(slots.dim() == 1 and slots.dtype == torch.int32 and slots.is_contiguous(), "slots: contiguous int32 [ns]")
    ns = slots.shape[0]
    _req(1 <= ns <= nb, f"slots: 1..{nb} pool slots, got {ns}")
    ok = (slots[0] >= 0) & (slots[-1] < nb) & (slots[1:] > slots[:-1]).all()
    _req(bool(ok), f"slots: ascending distinct pool slots in 0..{nb - 1}")
    return nb, ns


def tsdf_live_integrate(acc, bricks, dims, origin, voxel, depth, w2c, K, trunc, depth_max, rgb=None, conf=None, conf_ds=1, conf_min=0.0,
                        slots=None, subtract_mask=0):
    """in place on the accumulators acc int32 [5,nb,512] (sum_q, count, sum_r, sum_g, sum_b) of a live volume: B <= 16 views put in -- or,
    where bit b of subtract_mask is set, taken out -- in one launch, under the gates of tsdf_sparse_integrate.  slots: the pool slots to
    visit (int32, ascending and distinct), None = all.  rgb None: the colour sums are left alone."""
    X, Y, Z, T = _tsdf_sparse_grid(dims)
    nb, ns = _tsdf_live_pool(acc, bricks, slots, T)
    B, H, W, ch, cw = _tsdf_views("tsdf_live_integrate", depth, w2c, "w2c", K, voxel, trunc, TSDF_MAX_VIEWS, rgb, conf, conf_ds)
    mask = int(subtract_mask)
    _req(0 <= mask < (1 << B), f"subtract_mask {mask:#x}: a bit at or above the {B} views of the launch")
    lib = _lib.load()
    check(lib.cut3r_tsdf_live_integrate(_p(acc), _p(bricks), nb, _p(slots), ns, X, Y, Z, float(origin[0]), float(origin[1]), float(origin[2]),
                                        float(voxel), _p(depth), _p(rgb), _p(conf), B, H, W, ch, cw, int(conf_ds), float(conf_min), _p(w2c),
                                        _p(K), mask, float(trunc), float(depth_max), _stream()), "cut3r_tsdf_live_integrate")


def tsdf_live_resolve(acc, tsdf, weight, color, slots=None):
    """the accumulators as the fp32 pool planes of the sparse volume (tsdf [nb,512], weight [nb,512], color [3,nb,512], written in place on
    the slots given, None = all): correctly rounded means; a voxel with count 0 reads tsdf 1, weight 0, colour 0"""
    _cuda(acc, tsdf, weight, color, slots)
    _req(acc.dim() == 3 and acc.shape[0] == 5 and acc.shape[2] == TSDF_BRICK_VOXELS and acc.dtype == torch.int32 and acc.is_contiguous(),
         "acc: contiguous int32 [5,nb,512]")
    nb = acc.shape[1]
    _req(nb > 0 and nb * TSDF_BRICK_VOXELS < 2 ** 31, "live TSDF pool: at least one brick, fewer than 2^31 voxels")
    _req(tsdf.shape == (nb, TSDF_BRICK_VOXELS) and tsdf.dtype == F32 and tsdf.is_contiguous(), "tsdf: contiguous fp32 [nb,512]")
    _req(weight.shape == tsdf.shape and weight.dtype == F32 and weight.is_contiguous(), "weight: contiguous fp32 like tsdf")
    _req(color.shape == (3, nb, TSDF_BRICK_VOXELS) and color.dtype == F32 and color.is_contiguous(), "color: contiguous fp32 [3,nb,512]")
    _aligned(16, acc=acc, tsdf=tsdf, weight=weight, color=color)
    ns = 0
    if slots is not None:
        _req(slots.dim() == 1 and slots.dtype == torch.int32 and slots.is_contiguous(), "slots: contiguous int32 [ns]")
        ns = slots.shape[0]
        _req(1 <= ns <= nb, f"slots: 1..{nb} pool slots, got {ns}")
        _req(bool((slots[0] >= 0) & (slots[-1] < nb) & (slots[1:] > slots[:-1]).all()), f"slots: ascending distinct pool slots in 0..{nb - 1}")
    lib = _lib.load()
    check(lib.cut3r_tsdf_live_resolve(_p(acc), nb, _p(slots), ns, _p(tsdf), _p(weight), _p(color), _stream()), "cut3r_tsdf_live_resolve")


# ------------------------------------------------------------------------------------------------ ray cast of the TSDF volumes
def _tsdf_cast(what, dev, c2w, K, H, W, t_min, t_max, step, voxel, normals, colors, count):
    """the views and the outputs of a ray-cast launch: c2w [B,12], K [B,4] fp32 on the GPU, B <= 16 -> (B, H, W, depth [B,H,W], normal
    [B,H,W,3] or None, rgb u8 [B,3,H,W] or None, samples int32 [B,H,W] or None)"""
    _cuda(c2w, K)
    _req(c2w.dim() == 2 and c2w.shape[1] == 12 and c2w.dtype == F32 and c2w.is_contiguous(), "c2w: contiguous fp32 [B,12]")
    B, H, W = c2w.shape[0], int(H), int(W)
    _req(1 <= B <= TSDF_MAX_VIEWS, f"{what}: 1..{TSDF_MAX_VIEWS} views per launch")
    _req(K.shape == (B, 4) and K.dtype == F32 and K.is_contiguous(), "K: contiguous fp32 [B,4]")
    _req(H > 0 and W > 0 and B * H * W < 2 ** 31, "image: H, W > 0 and fewer than 2^31 pixels per launch")
    _req(float(voxel) > 0 and float(step) > 0, "voxel size and step must be > 0")
    _req(0 <= float(t_min) <= float(t_max), "ray range: 0 <= t_min <= t_max")
    depth = torch.empty(B, H, W, dtype=F32, device=dev)
    normal = torch.empty(B, H, W, 3, dtype=F32, device=dev) if normals else None
    rgb = torch.empty(B, 3, H, W, dtype=torch.uint8, device=dev) if colors else None
    samples = torch.empty(B, H, W, dtype=torch.int32, device=dev) if count else None
    return B, H, W, depth, normal, rgb, samples


def tsdf_ray_cast(tsdf, weight, color, origin, voxel, c2w, K, H, W, t_min, t_max, step, weight_threshold=1.0, normals=True, colors=True,
                  count=False):
    """ray cast of the dense planes (VoxelBlockGrid.ray_cast, tsdf_integrate.py:34) from B <= 16 views in one launch: c2w [B,12]
    camera->world rows, K [B,4] -> (depth [B,H,W] z-depth, 0 on a miss; normal [B,H,W,3] world frame or None; rgb u8 [B,3,H,W] or None;
    samples int32 [B,H,W] looked up per ray, or None)"""
    X, Y, Z = _tsdf_planes(tsdf, weight, color)
    B, H, W, depth, normal, rgb, samples = _tsdf_cast("tsdf_ray_cast", tsdf.device, c2w, K, H, W, t_min, t_max, step, voxel, normals, colors,
                                                      count)
    lib = _lib.load()
    check(lib.cut3r_tsdf_ray_cast(_p(tsdf), _p(weight), _p(color), X, Y, Z, float(origin[0]), float(origin[1]), float(origin[2]), float(voxel),
                                  _p(c2w), _p(K), B, H, W, float(t_min), float(t_max), float(step), float(weight_threshold), _p(depth),
                                  _p(normal), _p(rgb), _p(samples), _stream()), "cut3r_tsdf_ray_cast")
    return depth, normal, rgb, samples


def tsdf_sparse_ray_cast(tsdf, weight, color, table, bricks, dims, origin, voxel, c2w, K, H, W, t_min, t_max, step, weight_threshold=1.0,
                         normals=True, colors=True, count=False):
    """tsdf_ray_cast over the brick pool: a voxel of a brick that is not allocated is not stored, and a cell with such a corner is invalid"""
    X, Y, Z, T = _tsdf_sparse_grid(dims)
    nb = _tsdf_pool(tsdf, weight, color, bricks, T)
    _tsdf_table(table, "table", torch.int32, T)
    B, H, W, depth, normal, rgb, samples = _tsdf_cast("tsdf_sparse_ray_cast", tsdf.device, c2w, K, H, W, t_min, t_max, step, voxel, normals,
                                                      colors, count)
    lib = _lib.load()
    check(lib.cut3r_tsdf_sparse_ray_cast(_p(tsdf), _p(weight), _p(color), _p(table), _p(bricks), nb, X, Y, Z, float(origin[0]),
                                         float(origin[1]), float(origin[2]), float(voxel), _p(c2w), _p(K), B, H, W, float(t_min), float(t_max),
                                         float(step), float(weight_threshold), _p(depth), _p(normal), _p(rgb), _p(samples), _stream()),
          "cut3r_tsdf_sparse_ray_cast")
    return depth, normal, rgb, samples


# ------------------------------------------------------------------------------------------------ reconstruction metrics
def _points(t, name):
    _cuda(t)
    _req(t.dim() == 2 and t.shape[1] == 3 and t.dtype == F32 and t.is_contiguous(), f"{name}: contiguous fp32 [N,3]")
    _req(0 < t.shape[0] < 2 ** 31, f"{name}: 1 .. 2^31 - 1 points")
    _req(bool(torch.isfinite(t).all()), f"{name}: non-finite coordinates")
    return t.shape[0]


def _transform34(T, dev):
    if T is None:
        return None
    T = torch.as_tensor(T, dtype=torch.float64).reshape(1, -1)               # one 3x4 or 4x4 in any shape
    T = views.pose_rows(T, torch.float64).reshape(12).to(dev, F32).contiguous()
    _req(bool(torch.isfinite(T).all()), "transform: non-finite entries")
    return T


def mesh_area_cdf(verts, faces):
    """face areas fp32 [F] and their inclusive fp64 scan [F] (the area weights of trimesh.sample.sample_surface, eval_recon.py:104-107);
    faces int32 [F,3] must index verts"""
    V = _points(verts, "verts")
    _cuda(faces)
    _req(faces.dim() == 2 and faces.shape[1] == 3 and faces.dtype == torch.int32 and faces.is_contiguous(), "faces: contiguous int32 [F,3]")
    F = faces.shape[0]
    _req(0 < F < 2 ** 31, "faces: 1 .. 2^31 - 1 faces")
    _req(int(faces.min()) >= 0 and int(faces.max()) < V, "faces: vertex index out of range")
    lib = _lib.load()
    nbytes = lib.cut3r_mesh_cdf_workspace_bytes(F)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=verts.device)
    area = torch.empty(F, dtype=F32, device=verts.device)
    cdf = torch.empty(F, dtype=torch.float64, device=verts.device)
    check(lib.cut3r_mesh_area_cdf(_p(verts), V, _p(faces), F, _p(area), _p(cdf), _p(ws), nbytes, _stream()), "cut3r_mesh_area_cdf")
    return area, cdf


def mesh_sample(verts, faces, cdf, n, seed=0, stream_id=0):
    """n points [n,3] fp32, uniform over the surface by area (cdf from mesh_area_cdf); sample i depends on (seed, stream_id, i) only"""
    V = _points(verts, "verts")
    _cuda(faces, cdf)
    _req(faces.dim() == 2 and faces.shape[1] == 3 and faces.dtype == torch.int32 and faces.is_contiguous(), "faces: contiguous int32 [F,3]")
    F = faces.shape[0]
    _req(F > 0 and cdf.shape == (F,) and cdf.dtype == torch.float64 and cdf.is_contiguous(), "cdf: contiguous fp64 [F]")
    _req(int(n) > 0, "n must be > 0")
    _req(float(cdf[-1]) > 0, "mesh has zero total area")
    out = torch.empty(int(n), 3, dtype=F32, device=verts.device)
    lib = _lib.load()
    check(lib.cut3r_mesh_sample(_p(verts), V, _p(faces), F, _p(cdf), int(n), int(seed) % 2 ** 64, int(stream_id) % 2 ** 64, _p(out), _stream()),
          "cut3r_mesh_sample")
    return out


class NNGrid:
    """exact 1-NN searches among a fixed reference set ref [P,3] fp32 (cKDTree(ref).query, eval_recon.py:22-41): the grid is built once,
    then query() any number of query sets of up to `max_queries` points"""

    def __init__(self, ref, max_queries):
        self.P = _points(ref, "ref")
        self.ref = ref
        self.max_queries = int(max_queries)
        _req(0 < self.max_queries < 2 ** 31, "max_queries: 1 .. 2^31 - 1")
        lib = _lib.load()
        self.nbytes = lib.cut3r_nn_workspace_bytes(self.P, self.max_queries)
        _req(self.nbytes > 0, "NN workspace")
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=ref.device)
        check(lib.cut3r_nn_build(_p(ref), self.P, _p(self.ws), self.nbytes, _stream()), "cut3r_nn_build")

    def query(self, query, max_dist=None, transform=None):
        """(dist2 fp32 [Q], idx int32 [Q]) of every query point (under `transform`, 3x4 or 4x4, applied in fp32 on load); ties to the
        smallest reference index; no reference point with d2 <= max_dist^2: idx -1, dist2 +inf"""
        Q = _points(query, "query")
        _req(Q <= self.max_queries, f"query: {Q} points, the grid was sized for {self.max_queries}")
        md = float("inf") if max_dist is None else float(max_dist)
        _req(md >= 0, "max_dist must be >= 0")
        T = _transform34(transform, query.device)
        dist2 = torch.empty(Q, dtype=F32, device=query.device)
        idx = torch.empty(Q, dtype=torch.int32, device=query.device)
        lib = _lib.load()
        check(lib.cut3r_nn_query(self.P, _p(query), Q, _p(T), md, _p(dist2), _p(idx), _p(self.ws), self.nbytes, _stream()), "cut3r_nn_query")
        return dist2, idx

    def moments(self, query, dist2, idx, transform=None):
        """fp64 [17] over the correspondences idx >= 0: count, sum dist2, sum src [3], sum dst [3], sum src_a dst_b [3,3] (src = the query
        point under `transform` as query() loaded it, dst = ref[idx])"""
        Q = _points(query, "query")
        _cuda(dist2, idx)
        _req(dist2.shape == (Q,) and dist2.dtype == F32 and idx.shape == (Q,) and idx.dtype == torch.int32, "dist2 / idx of this query")
        _req(int(idx.max()) < self.P, "idx: reference index out of range")
        T = _transform34(transform, query.device)
        lib = _lib.load()
        nbytes = lib.cut3r_icp_moments_workspace_bytes(Q)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=query.device)
        out = torch.empty(17, dtype=torch.float64, device=query.device)
        check(lib.cut3r_icp_moments(_p(query), Q, _p(self.ref), self.P, _p(T), _p(dist2), _p(idx.contiguous()), _p(out), _p(ws), nbytes,
                                    _stream()), "cut3r_icp_moments")
        return out

    def moments_scaled(self, query, dist2, idx, transform=None):
        """fp64 [18]: the 17 of moments(), bit for bit, and sum |src|^2 (csrc/prstats.hip): what a similarity update needs"""
        Q = _points(query, "query")
        _cuda(dist2, idx)
        _req(dist2.shape == (Q,) and dist2.dtype == F32 and idx.shape == (Q,) and idx.dtype == torch.int32, "dist2 / idx of this query")
        _req(int(idx.max()) < self.P, "idx: reference index out of range")
        T = _transform34(transform, query.device)
        lib = _lib.load()
        nbytes = lib.cut3r_icp_moments_scaled_workspace_bytes(Q)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=query.device)
        out = torch.empty(18, dtype=torch.float64, device=query.device)
        check(lib.cut3r_icp_moments_scaled(_p(query), Q, _p(self.ref), self.P, _p(T), _p(dist2.contiguous()), _p(idx.contiguous()), _p(out),
                                           _p(ws), nbytes, _stream()), "cut3r_icp_moments_scaled")
        return out


def nn_query(ref, query, max_dist=None, transform=None):
    """one-shot NNGrid(ref).query(query)"""
    return NNGrid(ref, query.shape[0] if query.dim() == 2 else 0).query(query, max_dist=max_dist, transform=transform)


# ------------------------------------------------------------------------------------------------ precision / recall reductions
DIST_STATS_MAX_BINS = 4096


def _dist2(dist2):
    _cuda(dist2)
    _req(dist2.dim() == 1 and dist2.dtype == F32 and dist2.is_contiguous(), "dist2: contiguous fp32 [Q]")
    _req(0 < dist2.shape[0] < 2 ** 31, "dist2: 1 .. 2^31 - 1 entries")
    return dist2.shape[0]


def dist_stats(dist2, tau, bin_width=None, nbins=0):
    """(counts int64 [3], moments fp64 [4], hist int64 [nbins]) on the device, over the squared distances dist2 fp32 [Q] of NNGrid.query
    (csrc/prstats.hip; include/cut3r_hip.h states the rule and the order of the sums): counts = (good entries, good entries with d =
    sqrt(dist2) < tau, bad entries: NaN, negative, +inf), moments = (sum d, sum dist2, min d, max d), hist[k] = entries with k bin_width
    <= d < (k + 1) bin_width.  nbins = 0: no histogram (bin_width may be None)."""
    Q = _dist2(dist2)
    nbins = int(nbins)
    _req(0 <= nbins <= DIST_STATS_MAX_BINS, f"nbins: 0 .. {DIST_STATS_MAX_BINS}")
    bin_width = float(tau) if bin_width is None and nbins == 0 else bin_width
    _req(bin_width is not None, "bin_width: needed with nbins > 0")
    tau, bin_width = float(tau), float(bin_width)
    _req(tau > 0 and bin_width > 0, "tau and bin_width must be > 0")
    lib = _lib.load()
    nbytes = lib.cut3r_dist_stats_workspace_bytes(Q)
    _req(nbytes > 0, "dist_stats workspace")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dist2.device)
    counts = torch.empty(3, dtype=torch.int64, device=dist2.device)
    moments = torch.empty(4, dtype=torch.float64, device=dist2.device)
    hist = torch.empty(nbins, dtype=torch.int32, device=dist2.device)          # uint32 counts: Q < 2^31, so no sign
    check(lib.cut3r_dist_stats(_p(dist2), Q, tau, bin_width, nbins, _p(counts), _p(moments), _p(hist) if nbins else _p(None), _p(ws), nbytes,
                               _stream()), "cut3r_dist_stats")
    return counts, moments, hist.long()


def dist_median(dist2):
    """fp32 [2] on the device: the dist2 values of ascending ranks (n - 1) / 2 and n / 2 among the n good entries of dist2 fp32 [Q] (NaN
    when there is none), by a radix select (csrc/prstats.hip)"""
    Q = _dist2(dist2)
    lib = _lib.load()
    nbytes = lib.cut3r_dist_median_workspace_bytes(Q)
    _req(nbytes > 0, "dist_median workspace")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dist2.device)
    out = torch.empty(2, dtype=F32, device=dist2.device)
    check(lib.cut3r_dist_median(_p(dist2), Q, _p(out), _p(ws), nbytes, _stream()), "cut3r_dist_median")
    return out


# ------------------------------------------------------------------------------------------------ mesh depth rasteriser, 2-D metric
RASTER_MAX_VIEWS = 16


def _views(w2c, K, dev):
    """(w2c [B,12] fp32, K [B,4] fp32, B) on `dev` from the poses and intrinsics views.pose_rows / views.intrinsics take"""
    w2c = views.pose_rows(w2c, F32).reshape(-1, 12).to(dev).contiguous()
    B = w2c.shape[0]
    _req(B > 0, "w2c: no poses")
    K = views.intrinsics(K, B, F32).to(dev)
    _req(bool(torch.isfinite(w2c).all()) and bool(torch.isfinite(K).all()), "w2c / K: non-finite entries")
    _req(bool((K[:, :2] > 0).all()), "K: fx and fy must be > 0")
    return w2c, K, B


def _image_size(H, W):
    H, W = int(H), int(W)
    _req(1 <= H <= 65535 and 1 <= W <= 65535, "H, W: 1 .. 65535")
    return H, W


def mesh_raster(verts, faces, w2c, K, H, W, z_near=0.0, z_far=20.0, face_id=False):
    """depth [B,H,W] fp32 (0 = nothing hit) of the mesh from B cameras, and with face_id=True also the int32 [B,H,W] index of the face
    seen (-1 = nothing): the depth buffer the reference captures from its Open3D window (scripts/eval_recon.py:189-213).  w2c world->camera
    (OpenCV axes), K = fx fy cx cy per view, pixel centres at integer coordinates; both faces of a triangle are drawn, the nearest z in
    (z_near, z_far] wins, ties go to the smaller face index.  Any B: 16 views go into one launch."""
    V = _points(verts, "verts")
    _cuda(faces)
    _req(faces.dim() == 2 and faces.shape[1] == 3 and faces.dtype == torch.int32 and faces.is_contiguous(), "faces: contiguous int32 [F,3]")
    F = faces.shape[0]
    _req(0 < F < 2 ** 31, "faces: 1 .. 2^31 - 1 faces")
    _req(int(faces.min()) >= 0 and int(faces.max()) < V, "faces: vertex index out of range")
    H, W = _image_size(H, W)
    z_near, z_far = float(z_near), float(z_far)
    _req(z_near >= 0 and z_far > z_near and z_far < float("inf"), "0 <= z_near < z_far < inf")
    w2c, K, B = _views(w2c, K, verts.device)
    depth = torch.empty(B, H, W, dtype=F32, device=verts.device)
    fid = torch.empty(B, H, W, dtype=torch.int32, device=verts.device) if face_id else None
    lib = _lib.load()
    ws = None
    for b0 in range(0, B, RASTER_MAX_VIEWS):
        nb = min(RASTER_MAX_VIEWS, B - b0)
        nbytes = lib.cut3r_mesh_raster_workspace_bytes(F, nb, H, W)
        _req(nbytes > 0, "raster workspace")
        if ws is None or ws.numel() < nbytes:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=verts.device)
        check(lib.cut3r_mesh_raster(_p(verts), V, _p(faces), F, _p(w2c[b0:b0 + nb]), _p(K[b0:b0 + nb]), nb, H, W, z_near, z_far,
                                    _p(depth[b0:b0 + nb]), _p(fid[b0:b0 + nb]) if face_id else C.c_void_p(0), _p(ws), nbytes, _stream()),
              "cut3r_mesh_raster")
    return (depth, fid) if face_id else depth


def depth_l1(gt, ours):
    """fp64 [B,2] per view: the number of pixels with ours > 0 and the sum of |gt - ours| over them (scripts/eval_recon.py:216-218 before
    the mean); gt, ours fp32 [B,H,W].  The same bits on every run."""
    _cuda(gt, ours)
    _req(ours.dim() == 3 and ours.numel() > 0 and ours.shape == gt.shape, "gt, ours: [B,H,W] of one shape")
    _req(gt.dtype == F32 and ours.dtype == F32 and gt.is_contiguous() and ours.is_contiguous(), "gt, ours: contiguous fp32")
    B, H, W = ours.shape
    _req(H * W < 2 ** 31, "image too large")
    out = torch.empty(B, 2, dtype=torch.float64, device=ours.device)
    lib = _lib.load()
    for b0 in range(0, B, 65535):
        nb = min(65535, B - b0)
        nbytes = lib.cut3r_depth_l1_workspace_bytes(nb)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=ours.device)
        check(lib.cut3r_depth_l1(_p(gt[b0:b0 + nb]), _p(ours[b0:b0 + nb]), nb, H, W, _p(out[b0:b0 + nb]), _p(ws), nbytes, _stream()),
              "cut3r_depth_l1")
    return out


def points_in_view(points, w2c, K, H, W, edge=10.0):
    """int32 [B]: how many of points [N,3] each camera sees strictly inside the image shrunk by `edge` pixels, in front of it (the test of
    the reference's check_proj, scripts/eval_recon.py:60-89, for B candidate cameras)"""
    N = _points(points, "points")
    H, W = _image_size(H, W)
    edge = float(edge)
    _req(edge >= 0, "edge must be >= 0")
    w2c, K, B = _views(w2c, K, points.device)
    counts = torch.empty(B, dtype=torch.int32, device=points.device)
    lib = _lib.load()
    for b0 in range(0, B, RASTER_MAX_VIEWS):
        nb = min(RASTER_MAX_VIEWS, B - b0)
        check(lib.cut3r_points_in_view(_p(points), N, _p(w2c[b0:b0 + nb]), _p(K[b0:b0 + nb]), nb, H, W, edge, _p(counts[b0:b0 + nb]),
                                       _stream()), "cut3r_points_in_view")
    return counts


def mesh_vertex_visible(verts, depth, w2c, K, eps=0.03, z_far=20.0, flags=None):
    """u8 [V]: flags (given ones are kept: OR) set where a vertex is seen by one of the B views whose rendered depth [B,H,W] is `depth`:
    0 < z <= z_far, its nearest pixel inside the image, and not more than eps behind the depth there"""
    V = _points(verts, "verts")
    _cuda(depth)
    _req(depth.dim() == 3 and depth.dtype == F32 and depth.is_contiguous() and depth.numel() > 0, "depth: contiguous fp32 [B,H,W]")
    B, H, W = depth.shape
    H, W = _image_size(H, W)
    w2c, K, Bv = _views(w2c, K, verts.device)
    _req(Bv == B, "depth and w2c: one view each")
    eps, z_far = float(eps), float(z_far)
    _req(eps >= 0 and z_far > 0, "eps >= 0, z_far > 0")
    if flags is None:
        flags = torch.zeros(V, dtype=torch.uint8, device=verts.device)
    _cuda(flags)
    _req(flags.shape == (V,) and flags.dtype == torch.uint8 and flags.is_contiguous(), "flags: contiguous u8 [V]")
    lib = _lib.load()
    for b0 in range(0, B, RASTER_MAX_VIEWS):
        nb = min(RASTER_MAX_VIEWS, B - b0)
        check(lib.cut3r_mesh_vertex_visible(_p(verts), V, _p(depth[b0:b0 + nb]), _p(w2c[b0:b0 + nb]), _p(K[b0:b0 + nb]), nb, H, W, eps, z_far,
                                            _p(flags), _stream()), "cut3r_mesh_vertex_visible")
    return flags


# ------------------------------------------------------------------------------------------------ dense point clouds of depth maps
CLOUD_MAX_VIEWS = 16
VOXEL_MAX_INDEX = 2 ** 21 - 1           # three voxel indices in one 63-bit sort key


def depth_cloud(depth, c2w, K, depth_trunc, size=None, rgb=None):
    """the world point cloud of B depth maps (Open3D create_from_color_and_depth + create_from_rgbd_image(project_valid_depth_only) +
    transform, scripts/eval7_scenes_dense.py:72-96) -> (points fp32 [N,3], colors u8 [N,3] or None, counts int64 [B]), ordered by view,
    then row-major pixel.  depth fp32 [B,H,W] metres on the GPU, any B (16 views per launch); c2w [B,12] / [B,3,4] / [B,4,4], any 3x4
    affine, used in fp64; K [B,4] or [4] = fx fy cx cy OF THE SAMPLING GRID, fp64; rgb u8 [B,3,H,W] or None.  A pixel counts iff its depth
    is finite, > 0 and < fp32(depth_trunc).  size=(H1, W1): sample the maps on an H1 x W1 nearest-neighbour grid, grid pixel (i, j) reading
    source pixel (min(i H // H1, H - 1), min(j W // W1, W - 1)), the exact floor.  cv2.resize(INTER_NEAREST), which the reference's
    vggt_resize uses, multiplies by a rounded reciprocal and may pick the neighbour where j W / W1 is an integer: parity with cv2 is NOT
    pinned (cv2 was not available to compare against).  z = d, x = (j - cx) z / fx, y = (i - cy) z / fy and the affine in fp64, rounded
    once to fp32.  All views are counted first, the output is allocated once, and each launch emits at its offset."""
    _cuda(depth, rgb)
    _req(depth.dim() == 3 and depth.dtype == F32 and depth.is_contiguous(), "depth: contiguous fp32 [B,H,W]")
    B, H, W = depth.shape
    _req(B >= 1 and H > 0 and W > 0, "depth: empty")
    H1, W1 = (H, W) if size is None else (int(size[0]), int(size[1]))
    _req(H1 > 0 and W1 > 0, "size: H1, W1 > 0")
    _req(max(H * W, H1 * W1) < 2 ** 31 // CLOUD_MAX_VIEWS, "depth_cloud: image too large")
    trunc = float(depth_trunc)
    _req(trunc > 0, "depth_trunc must be > 0")
    c2w = views.pose_rows(c2w, torch.float64).reshape(-1, 12).cpu().contiguous()
    _req(c2w.shape[0] == B, f"c2w: {c2w.shape[0]} poses for {B} depth maps")
    K = views.intrinsics(K, B, torch.float64).cpu()
    _req(bool(torch.isfinite(c2w).all()) and bool(torch.isfinite(K).all()), "c2w / K: non-finite entries")
    _req(bool((K[:, :2] > 0).all()), "K: fx and fy must be > 0")
    if rgb is not None:
        _req(rgb.shape == (B, 3, H, W) and rgb.dtype == torch.uint8 and rgb.is_contiguous(), "rgb: contiguous uint8 [B,3,H,W]")
    dev = depth.device
    lib = _lib.load()
    batches = [(b0, min(CLOUD_MAX_VIEWS, B - b0)) for b0 in range(0, B, CLOUD_MAX_VIEWS)]
    nbytes = lib.cut3r_depth_cloud_workspace_bytes(CLOUD_MAX_VIEWS, H1, W1)
    _req(nbytes > 0, "depth_cloud workspace")
    ws = torch.empty(len(batches), nbytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(B, dtype=torch.int64, device=dev)
    for k, (b0, nb) in enumerate(batches):
        check(lib.cut3r_depth_cloud_count(_p(depth[b0:b0 + nb]), nb, H, W, H1, W1, trunc, _p(ws[k]), nbytes, _p(counts[b0:b0 + nb]), _stream()),
              "cut3r_depth_cloud_count")
    host = counts.cpu()
    N = int(host.sum())
    points = torch.empty(N, 3, dtype=F32, device=dev)
    colors = torch.empty(N, 3, dtype=torch.uint8, device=dev) if rgb is not None else None
    at = 0
    for k, (b0, nb) in enumerate(batches):
        n = int(host[b0:b0 + nb].sum())
        if n:
            check(lib.cut3r_depth_cloud_emit(_p(depth[b0:b0 + nb]), _p(rgb[b0:b0 + nb]) if rgb is not None else C.c_void_p(0), nb, H, W, H1, W1,
                                             C.c_void_p(c2w[b0:b0 + nb].data_ptr()), C.c_void_p(K[b0:b0 + nb].data_ptr()), trunc, _p(ws[k]),
                                             nbytes, _p(points[at:at + n]), _p(colors[at:at + n]) if colors is not None else C.c_void_p(0), n,
                                             N - at, _stream()), "cut3r_depth_cloud_emit")
        at += n
    return points, colors, counts


def cloud_bounds(points):
    """(lo fp32 [3], hi fp32 [3]) host tensors: the exact bounds of points fp32 [N,3]; ValueError on a non-finite coordinate"""
    _cuda(points)
    _req(points.dim() == 2 and points.shape[1] == 3 and points.dtype == F32 and points.is_contiguous(), "points: contiguous fp32 [N,3]")
    N = points.shape[0]
    _req(0 < N < 2 ** 31, "points: 1 .. 2^31 - 1 points")
    lib = _lib.load()
    nbytes = lib.cut3r_cloud_bounds_workspace_bytes(N)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=points.device)
    out = torch.empty(7, dtype=F32, device=points.device)
    check(lib.cut3r_cloud_bounds(_p(points), N, _p(out), _p(ws), nbytes, _stream()), "cut3r_cloud_bounds")
    out = out.cpu()
    _req(float(out[6]) == 0, "points: non-finite coordinates")
    return out[:3].contiguous(), out[3:6].contiguous()


def voxel_downsample(points, voxel, colors=None):
    """Open3D PointCloud.voxel_down_sample as eval_recon.voxel_down_sample states it -> (points fp32 [M,3], colors u8 [M,3] or None, counts
    int32 [M]): voxel index floor(((double)p - (min - voxel / 2)) / voxel) per axis, one output per occupied voxel sorted by (ix, iy,
    iz), each the fp64 mean of the voxel's points summed in ascending point index and rounded once to fp32 (colours: floor(mean + 0.5)).
    Refused before any sort: voxel <= 0 or not finite, non-finite points, an extent of 2^21 voxels or more on an axis."""
    voxel = float(voxel)
    _req(voxel > 0 and voxel < float("inf"), "voxel must be > 0 and finite")
    lo, hi = cloud_bounds(points)
    N = points.shape[0]
    top = torch.floor((hi.double() - (lo.double() - voxel * 0.5)) / voxel)
    _req(bool((top <= VOXEL_MAX_INDEX).all()), f"voxel_downsample: the extent spans more than 2^21 voxels of {voxel:g}")
    if colors is not None:
        _cuda(colors)
        _req(colors.shape == (N, 3) and colors.dtype == torch.uint8 and colors.is_contiguous(), "colors: contiguous uint8 [N,3]")
    dev = points.device
    lib = _lib.load()
    nbytes = lib.cut3r_voxel_downsample_workspace_bytes(N)
    _req(nbytes > 0, "voxel_downsample workspace")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    check(lib.cut3r_voxel_downsample_count(_p(points), N, voxel, C.c_void_p(lo.data_ptr()), C.c_void_p(hi.data_ptr()), _p(ws), nbytes, _p(total),
                                           _stream()), "cut3r_voxel_downsample_count")
    M = int(total.cpu())
    out = torch.empty(M, 3, dtype=F32, device=dev)
    out_col = torch.empty(M, 3, dtype=torch.uint8, device=dev) if colors is not None else None
    cnt = torch.empty(M, dtype=torch.int32, device=dev)
    check(lib.cut3r_voxel_downsample_emit(_p(points), _p(colors), N, _p(ws), nbytes, _p(out), _p(out_col), _p(cnt), M, M, _stream()),
          "cut3r_voxel_downsample_emit")
    return out, out_col, cnt


# ------------------------------------------------------------------------------------------------ mesh clean-up after the extraction
class _StageClock:
    """HIP events between the stages of one call (tools/bench_mesh_clean.py); off unless a `timing` dict is passed.  mark(name) closes
    the stage `name` on the stream; inside(n) hands n events to a C entry point that records them between its own stages."""

    def __init__(self, timing):
        self.timing, self.marks = timing, []

    def mark(self, name):
        if self.timing is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.marks.append((name, e))

    def inside(self, *names):
        if self.timing is None:
            return C.c_void_p(0)
        for n in names:
            self.mark(n)                                     # recorded once here so that the handle exists; the callee records it again
        return (C.c_void_p * len(names))(*[C.c_void_p(e.cuda_event) for _, e in self.marks[-len(names):]])

    def close(self):
        if self.timing is None:
            return
        torch.cuda.synchronize()
        for (_, a), (name, b) in zip(self.marks[:-1], self.marks[1:]):
            if name != "host":                               # "host": the stretch that ends after a read-back, not a stage
                self.timing[name] = self.timing.get(name, 0.0) + a.elapsed_time(b)


def _mesh(verts, colors, faces):
    _cuda(verts, colors, faces)
    _req(verts.dim() == 2 and verts.shape[1] == 3 and verts.dtype == F32 and verts.is_contiguous(), "vertices: contiguous fp32 [V,3]")
    _req(faces.dim() == 2 and faces.shape[1] == 3 and faces.dtype == torch.int32 and faces.is_contiguous(), "faces: contiguous int32 [F,3]")
    V, F = verts.shape[0], faces.shape[0]
    _req(0 < V < 2 ** 31 and 0 < F < 2 ** 31, "mesh: 1 .. 2^31 - 1 vertices and faces")
    if colors is not None:
        _req(colors.shape == (V, 3) and colors.dtype == torch.uint8 and colors.is_contiguous(), "colors: contiguous uint8 [V,3]")
    return V, F


def mesh_faces_check(faces, V):
    """ValueError when an index of faces int32 [F,3] lies outside [0, V): a flag kernel, run before anything gathers through the faces"""
    bad = torch.empty(1, dtype=torch.int32, device=faces.device)
    check(_lib.load().cut3r_mesh_faces_check(_p(faces), faces.shape[0], V, _p(bad), _stream()), "cut3r_mesh_faces_check")
    _req(int(bad.item()) == 0, f"faces: an index outside [0, {V})")


def _capacity(capacity, need_v, need_f):
    cap_v, cap_f = (need_v, need_f) if capacity is None else (int(capacity[0]), int(capacity[1]))
    _req(cap_v >= need_v and cap_f >= need_f, f"capacity ({cap_v}, {cap_f}) below the counted totals ({need_v}, {need_f})")
    return cap_v, cap_f


def mesh_cluster(verts, colors, faces, cell, passes=0, capacity=None, timing=None):
    """vertex clustering of a mesh on the GPU (include/cut3r_hip.h, the mesh clean-up block, states the definition) -> dict: vertices fp32
    [V',3], colors u8 [V',3] or None, faces int32 [F',3], vertex_map int32 [V], face_map int32 [F'] and the counts clusters, degenerate,
    duplicate, unreferenced.  passes: 0 chooses the sort passes of the de-duplication, 1 / 2 force them (the result is the same).
    capacity=(rows of vertices, rows of faces) the outputs are allocated with (default: the counted totals).  ValueError before any sort
    or gather: sizes, a face index outside [0, V), non-finite vertices, cell <= 0 or not finite, 2^21 cells or more on an axis,
    a capacity below the counted totals."""
    V, F = _mesh(verts, colors, faces)
    cell = float(cell)
    _req(cell > 0 and cell < float("inf"), "cell must be > 0 and finite")
    _req(passes in (0, 1, 2), "passes: 0, 1 or 2")
    clock = _StageClock(timing)
    clock.mark("host")
    mesh_faces_check(faces, V)
    clock.mark("face check")
    lo, hi = cloud_bounds(verts)
    top = torch.floor((hi.double() - (lo.double() - cell * 0.5)) / cell)
    _req(bool((top <= VOXEL_MAX_INDEX).all()), f"mesh_cluster: the extent spans more than 2^21 cells of {cell:g}")
    dev = verts.device
    lib = _lib.load()
    nbytes = lib.cut3r_mesh_cluster_workspace_bytes(V, F)
    _req(nbytes > 0, "mesh_cluster workspace")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    totals = torch.empty(4, dtype=torch.int64, device=dev)
    clock.mark("host")
    check(lib.cut3r_mesh_cluster_count(_p(verts), V, F, cell, C.c_void_p(lo.data_ptr()), C.c_void_p(hi.data_ptr()), _p(ws), nbytes, _p(totals),
                                       _stream()), "cut3r_mesh_cluster_count")
    clock.mark("keys + sort")
    M = int(totals[0].item())
    if passes == 1:
        _req(3 * max(1, (M - 1).bit_length()) <= 64, f"passes=1: three ids below {M} do not fit one 64-bit key")
    clock.mark("host")
    ev = clock.inside("remap", "de-duplication")
    check(lib.cut3r_mesh_cluster_faces(_p(faces), V, F, M, passes, _p(ws), nbytes, _p(totals), ev, _stream()), "cut3r_mesh_cluster_faces")
    clock.mark("compaction")
    Fo, Vo, deg, dup = (int(x) for x in totals.cpu())
    cap_v, cap_f = _capacity(capacity, Vo, Fo)
    out_v = torch.empty(cap_v, 3, dtype=F32, device=dev)
    out_c = torch.empty(cap_v, 3, dtype=torch.uint8, device=dev) if colors is not None else None
    out_f = torch.empty(cap_f, 3, dtype=torch.int32, device=dev)
    vmap = torch.empty(V, dtype=torch.int32, device=dev)
    fmap = torch.empty(cap_f, dtype=torch.int32, device=dev)
    clock.mark("host")
    ev = clock.inside("means")
    check(lib.cut3r_mesh_cluster_emit(_p(verts), _p(colors), V, F, M, _p(ws), nbytes, _p(out_v), _p(out_c), _p(out_f), _p(vmap), _p(fmap), Vo, Fo,
                                      cap_v, cap_f, ev, _stream()), "cut3r_mesh_cluster_emit")
    clock.mark("compaction")
    clock.close()
    return {"vertices": out_v[:Vo], "colors": None if out_c is None else out_c[:Vo], "faces": out_f[:Fo], "vertex_map": vmap, "face_map": fmap[:Fo],
            "clusters": M, "degenerate": deg, "duplicate": dup, "unreferenced": M - Vo}


def mesh_labels(faces, V, timing=None):
    """(labels int32 [V], rounds): label(v) = the smallest vertex index of v's connected component (two vertices are connected when a face
    holds both).  Min-label hooking and pointer jumping, one launch each per round; the loop runs here, reading a device word back after
    every round, and stops when a round changes nothing.  RuntimeError past V rounds (every other round removes a label, so V suffice)."""
    _cuda(faces)
    _req(faces.dim() == 2 and faces.shape[1] == 3 and faces.dtype == torch.int32 and faces.is_contiguous(), "faces: contiguous int32 [F,3]")
    V, F = int(V), faces.shape[0]
    _req(0 < V < 2 ** 31 and 0 < F < 2 ** 31, "mesh: 1 .. 2^31 - 1 vertices and faces")
    dev = faces.device
    lib = _lib.load()
    labels = torch.empty(V, dtype=torch.int32, device=dev)
    scratch = torch.empty(V, dtype=torch.int32, device=dev)
    changed = torch.empty(1, dtype=torch.int32, device=dev)
    clock = _StageClock(timing)
    clock.mark("host")
    check(lib.cut3r_mesh_label_init(_p(labels), _p(scratch), V, _stream()), "cut3r_mesh_label_init")
    rounds = 0
    while True:
        if rounds >= V:
            raise RuntimeError(f"mesh_labels: no fixed point after {rounds} rounds over {V} vertices")
        check(lib.cut3r_mesh_label_round(_p(faces), V, F, _p(labels), _p(scratch), _p(changed), _stream()), "cut3r_mesh_label_round")
        rounds += 1
        if int(changed.item()) == 0:
            break
    clock.mark("labelling")
    clock.close()
    return labels, rounds


def mesh_components(verts, colors, faces, min_faces=None, keep_largest=None, capacity=None, timing=None):
    """small-component removal of a mesh on the GPU (include/cut3r_hip.h states the definition) -> dict: vertices, colors, faces,
    vertex_map int32 [V], face_map int32 [F'], labels int32 [V], components int32 [K,2] = (label, size) of the kept components by (size
    descending, label ascending), n_components, rounds.  Exactly one of min_faces >= 1 (components of at least that many faces stay) and
    keep_largest >= 1.  ValueError as mesh_cluster, and for the options."""
    V, F = _mesh(verts, colors, faces)
    _req((min_faces is None) != (keep_largest is None), "exactly one of min_faces and keep_largest")
    opt = int(min_faces if min_faces is not None else keep_largest)
    _req(1 <= opt < 2 ** 31, "min_faces / keep_largest must be >= 1")
    mesh_faces_check(faces, V)
    cloud_bounds(verts)                                      # refuses non-finite vertices
    dev = verts.device
    lib = _lib.load()
    nbytes = lib.cut3r_mesh_components_workspace_bytes(V, F)
    _req(nbytes > 0, "mesh_components workspace")
    labels, rounds = mesh_labels(faces, V, timing)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    totals = torch.empty(4, dtype=torch.int64, device=dev)
    clock = _StageClock(timing)
    clock.mark("host")
    check(lib.cut3r_mesh_components_count(_p(faces), V, F, _p(labels), opt if min_faces is not None else 0, opt if keep_largest is not None else 0,
                                          _p(ws), nbytes, _p(totals), _stream()), "cut3r_mesh_components_count")
    n_comp, K, Fo, Vo = (int(x) for x in totals.cpu())
    cap_v, cap_f = _capacity(capacity, Vo, Fo)
    out_v = torch.empty(cap_v, 3, dtype=F32, device=dev)
    out_c = torch.empty(cap_v, 3, dtype=torch.uint8, device=dev) if colors is not None else None
    out_f = torch.empty(cap_f, 3, dtype=torch.int32, device=dev)
    vmap = torch.empty(V, dtype=torch.int32, device=dev)
    fmap = torch.empty(cap_f, dtype=torch.int32, device=dev)
    comps = torch.empty(K, 2, dtype=torch.int32, device=dev)
    check(lib.cut3r_mesh_components_emit(_p(verts), _p(colors), V, _p(faces), F, _p(ws), nbytes, _p(out_v), _p(out_c), _p(out_f), _p(vmap), _p(fmap),
                                         _p(comps), Vo, Fo, K, cap_v, cap_f, K, _stream()), "cut3r_mesh_components_emit")
    clock.mark("filter")
    clock.close()
    if timing is not None:
        timing["rounds"] = rounds
    return {"vertices": out_v[:Vo], "colors": None if out_c is None else out_c[:Vo], "faces": out_f[:Fo], "vertex_map": vmap, "face_map": fmap[:Fo],
            "labels": labels, "components": comps, "n_components": n_comp, "rounds": rounds}


# ------------------------------------------------------------------------------------------------ LPIPS (csrc/lpips.hip)
LPIPS_NORMS = {"torchmetrics": 0, "lpips": 1}


def _lpips_act(x, name):
    _cuda(x)
    _req(x.dim() == 4 and x.dtype == F32 and x.is_contiguous() and x.numel() > 0, f"{name}: contiguous fp32 [n,H,W,C]")
    return tuple(int(v) for v in x.shape)


def lpips_input(a, b):
    """a, b fp32 [B,3,H,W] in [0,1] -> channels-last fp32 [2B,H,W,3] = ((2 v - 1) - shift) / scale, the B images of a first"""
    _cuda(a, b)
    _req(a.dim() == 4 and a.shape[1] == 3 and a.shape == b.shape and a.numel() > 0, "a, b: [B,3,H,W] of one shape")
    _req(a.dtype == F32 and b.dtype == F32 and a.is_contiguous() and b.is_contiguous(), "a, b: contiguous fp32")
    B, _, H, W = a.shape
    out = torch.empty(2 * B, H, W, 3, dtype=F32, device=a.device)
    check(_lib.load().cut3r_lpips_input(_p(a), _p(b), B, H, W, _p(out), _stream()), "cut3r_lpips_input")
    return out


def lpips_conv(x, w, bias, stride, pad, impl=0):
    """relu(conv(x) + bias): x [n,H,W,Ci], w [KH,KW,Ci,Co], bias [Co] -> [n,Ho,Wo,Co], every output the k-ascending fmaf chain from its
    bias (impl 0: on the fp32 MFMA, the tile chosen by the number of rows; 1: the same chain on the VALU; 2 / 3: the MFMA kernel with 128- /
    64-row tiles; all four give the same bits)"""
    n, H, W, Ci = _lpips_act(x, "x")
    _cuda(w, bias)
    _req(w.dim() == 4 and w.dtype == F32 and w.is_contiguous() and w.shape[2] == Ci, f"w: contiguous fp32 [KH,KW,{Ci},Co]")
    KH, KW, _, Co = (int(v) for v in w.shape)
    _req(bias.shape == (Co,) and bias.dtype == F32 and bias.is_contiguous(), f"bias: contiguous fp32 [{Co}]")
    lib = _lib.load()
    Ho, Wo = lib.cut3r_lpips_conv_out(H, KH, stride, pad), lib.cut3r_lpips_conv_out(W, KW, stride, pad)
    _req(Ho > 0 and Wo > 0, f"a {KH}x{KW} convolution of a {H}x{W} map has no output")
    y = torch.empty(n, Ho, Wo, Co, dtype=F32, device=x.device)
    check(lib.cut3r_lpips_conv(_p(x), _p(w), _p(bias), _p(y), n, H, W, Ci, Co, KH, KW, int(stride), int(pad), int(impl), _stream()),
          f"cut3r_lpips_conv n={n} {H}x{W}x{Ci} -> {Co} k={KH}")
    return y


def lpips_pool(x):
    """3x3 stride-2 max-pool without padding of a channels-last map"""
    n, H, W, Cc = _lpips_act(x, "x")
    _req(H >= 3 and W >= 3, f"a 3x3 pool of a {H}x{W} map has no output")
    y = torch.empty(n, (H - 3) // 2 + 1, (W - 3) // 2 + 1, Cc, dtype=F32, device=x.device)
    check(_lib.load().cut3r_lpips_pool(_p(x), _p(y), n, H, W, Cc, _stream()), "cut3r_lpips_pool")
    return y


def lpips_tail(feat, lin, score, accumulate, norm="torchmetrics"):
    """one tap: feat [2B,Hl,Wl,C], lin [C] -> v [B,Hl,Wl]; score [B] fp64 (+)= the fp64 mean of v per pair, in a fixed order"""
    n, H, W, Cc = _lpips_act(feat, "feat")
    _cuda(lin, score)
    _req(norm in LPIPS_NORMS, f"norm must be one of {sorted(LPIPS_NORMS)}")
    _req(n % 2 == 0 and Cc % 4 == 0, "feat: an even number of images, C a multiple of 4")
    _req(lin.shape == (Cc,) and lin.dtype == F32 and lin.is_contiguous(), f"lin: contiguous fp32 [{Cc}]")
    _req(score.shape == (n // 2,) and score.dtype == torch.float64 and score.is_contiguous(), f"score: contiguous fp64 [{n // 2}]")
    v = torch.empty(n // 2, H, W, dtype=F32, device=feat.device)
    check(_lib.load().cut3r_lpips_tail(_p(feat), _p(lin), n // 2, H * W, Cc, LPIPS_NORMS[norm], int(bool(accumulate)), _p(v), _p(score),
                                       _stream()), "cut3r_lpips_tail")
    return v


# ------------------------------------------------------------------------------------------------ focal length from self-view pointmaps
def _focal_args(pts, pp, conf, conf_min):
    _cuda(pts, pp, conf)
    _req(pts.dim() == 4 and pts.shape[3] == 3 and pts.dtype == F32 and pts.is_contiguous(), "pts: contiguous fp32 [B,H,W,3]")
    B, H, W, _ = pts.shape
    _req(B >= 1 and H * W >= 1 and 2 * H * W < 2 ** 31, "pts: B >= 1 and 1 <= H W < 2^30")
    _req(pp.shape == (B, 2) and pp.dtype == F32 and pp.is_contiguous() and pp.device == pts.device, "pp: contiguous fp32 [B,2] on the device of pts")
    _req((conf is None) == (conf_min is None), "conf and conf_min go together")
    if conf is not None:
        _req(conf.shape == (B, H, W) and conf.dtype == F32 and conf.is_contiguous() and conf.device == pts.device,
             "conf: contiguous fp32 [B,H,W] on the device of pts")
    return B, H, W, float(conf_min) if conf_min is not None else 0.0


def focal_workspace(B, H, W, device):
    lib = _lib.load()
    nbytes = lib.cut3r_focal_workspace_bytes(B, H, W)
    _req(nbytes > 0, "focal workspace")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _focal_ws(B, H, W, device, workspace):
    if workspace is None:
        return focal_workspace(B, H, W, device)
    _cuda(workspace)
    _req(workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.device == device, "workspace: contiguous uint8 on the device of pts")
    _req(workspace.numel() >= _lib.load().cut3r_focal_workspace_bytes(B, H, W), "workspace shorter than cut3r_focal_workspace_bytes(B, H, W)")
    return workspace


def focal_weiszfeld(pts, pp, iters=10, conf=None, conf_min=None, workspace=None):
    """post_process.py:38-55 without the final clip -> focal fp32 [B] on the device (csrc/calib.hip states the arithmetic and the order of
    the sums; tests/focal_oracle.py restates them).  pts fp32 [B,H,W,3], pp fp32 [B,2]; a pixel with conf < conf_min takes no part."""
    B, H, W, cmin = _focal_args(pts, pp, conf, conf_min)
    _req(int(iters) >= 0, "iters >= 0")
    ws = _focal_ws(B, H, W, pts.device, workspace)
    focal = torch.empty(B, dtype=F32, device=pts.device)
    check(_lib.load().cut3r_focal_weiszfeld(_p(pts), _p(conf), cmin, _p(pp), B, H, W, int(iters), _p(focal), _p(ws), ws.numel(), _stream()),
          "cut3r_focal_weiszfeld")
    return focal


def focal_median(pts, pp, conf=None, conf_min=None, workspace=None):
    """post_process.py:27-36 without the final clip -> focal fp32 [B] on the device: torch.nanmedian of the 2 H W votes (u z) / x, (v z) / y
    of every view by a radix select (csrc/calib.hip)."""
    B, H, W, cmin = _focal_args(pts, pp, conf, conf_min)
    ws = _focal_ws(B, H, W, pts.device, workspace)
    focal = torch.empty(B, dtype=F32, device=pts.device)
    check(_lib.load().cut3r_focal_median(_p(pts), _p(conf), cmin, _p(pp), B, H, W, _p(focal), _p(ws), ws.numel(), _stream()),
          "cut3r_focal_median")
    return focal


# ------------------------------------------------------------------------------------------------ multi-view depth consistency
CONSISTENCY_MAX_SOURCES = 16
CONSISTENCY_MAX_REFS = 65535


def depth_consistency(depth, K, ref, src, fwd, bwd, depth_max, pix=1.0, rel=0.01, z_min=1e-3, average=False):
    """cross-check R views of a depth stack against up to 16 source views each (csrc/consistency.hip; include/cut3r_hip.h states the rule,
    tests/consistency_oracle.py restates it) -> (support u8 [R,H,W], violation u8 [R,H,W], depth_avg fp32 [R,H,W] or None).  depth fp32
    [N,H,W] and K fp32 [N,4] on the GPU; ref [R] and src [R,S] HOST integer tables (src -1: no source), checked here against [0, N) since
    the kernel cannot refuse what lies in device memory; fwd, bwd HOST fp64 [R,S,12], the rigid rows reference -> source and back
    (depth_consistency.relative_rows)."""
    import numpy as np
    _cuda(depth, K)
    _req(depth.dim() == 3 and depth.dtype == F32 and depth.is_contiguous(), "depth: contiguous fp32 [N,H,W]")
    N, H, W = depth.shape
    _req(N >= 1 and H > 0 and W > 0, "depth: empty")
    _req(H * W < 2 ** 31 // 16, "depth_consistency: image too large")
    _req(K.shape == (N, 4) and K.dtype == F32 and K.is_contiguous() and K.device == depth.device, "K: contiguous fp32 [N,4] on the device of depth")
    ref = np.asarray(ref)
    src = np.asarray(src)
    _req(ref.ndim == 1 and src.ndim == 2 and src.shape[0] == ref.shape[0] and ref.dtype.kind in "iu" and src.dtype.kind in "iu",
         "ref: integers [R], src: integers [R,S]")
    R, S = src.shape
    _req(1 <= R <= CONSISTENCY_MAX_REFS, f"ref: 1 .. {CONSISTENCY_MAX_REFS} views a launch")
    _req(1 <= S <= CONSISTENCY_MAX_SOURCES, f"src: 1 .. {CONSISTENCY_MAX_SOURCES} sources a view")
    _req(bool(((ref >= 0) & (ref < N)).all()), "ref: index outside the depth stack")
    _req(bool(((src >= -1) & (src < N)).all()), "src: index outside the depth stack (-1: no source)")
    _req(not bool((src == ref[:, None]).any()), "src: a view cannot be its own source")
    fwd = np.ascontiguousarray(fwd, np.float64)
    bwd = np.ascontiguousarray(bwd, np.float64)
    _req(fwd.shape == (R, S, 12) and bwd.shape == (R, S, 12), "fwd, bwd: fp64 [R,S,12]")
    used = src >= 0
    _req(bool(np.isfinite(fwd[used]).all()) and bool(np.isfinite(bwd[used]).all()), "fwd / bwd: non-finite rows")
    depth_max, pix, rel, z_min = float(depth_max), float(pix), float(rel), float(z_min)
    _req(depth_max > 0 and pix > 0 and 0 < rel < 1 and z_min >= 0, "depth_max, pix > 0, 0 < rel < 1, z_min >= 0")
    dev = depth.device
    ref_d = torch.from_numpy(np.ascontiguousarray(ref, np.int32)).to(dev)
    src_d = torch.from_numpy(np.ascontiguousarray(src, np.int32)).to(dev)
    fwd_d = torch.from_numpy(np.where(used[..., None], fwd, 0.0)).to(dev)
    bwd_d = torch.from_numpy(np.where(used[..., None], bwd, 0.0)).to(dev)
    support = torch.empty(R, H, W, dtype=torch.uint8, device=dev)
    violation = torch.empty(R, H, W, dtype=torch.uint8, device=dev)
    avg = torch.empty(R, H, W, dtype=F32, device=dev) if average else None
    check(_lib.load().cut3r_depth_consistency(_p(depth), _p(K), N, H, W, _p(ref_d), _p(src_d), R, S, _p(fwd_d), _p(bwd_d), depth_max, pix, rel,
                                              z_min, _p(support), _p(violation), _p(avg), _stream()), "cut3r_depth_consistency")
    return support, violation, avg


# ------------------------------------------------------------------------------------------------ GS panels and frames
PANEL_MAX_PIXELS = 2 ** 26
FRAME_LAYERS = {"rgb": 0, "depth": 1, "normal": 2}


def turbo_u8():
    """the committed turbo byte table (csrc/turbo_u8.h, the kernels' own copy) as a numpy uint8 [256,3]"""
    import re

    import numpy as np
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "turbo_u8.h"), encoding="ascii") as fh:
        body = "".join(ln for ln in fh if not ln.lstrip().startswith("//"))
    t = np.array([int(v) for v in re.findall(r"\d+", body)], np.int64)
    _req(t.size == 768 and int(t.max()) <= 255, "csrc/turbo_u8.h: 768 bytes expected")
    return t.astype(np.uint8).reshape(256, 3)


def _map(t, name, shape, dev=None):
    _req(t.is_cuda and t.dtype == F32 and t.is_contiguous() and tuple(t.shape) == tuple(shape) and (dev is None or t.device == dev),
         f"{name}: contiguous fp32 {list(shape)} on the GPU")


def gs_panel_ranges(a=None, b=None, alpha=None):
    """min / max of the maps a, b, |a - b| and (alpha > 0.5) in one launch (csrc/gs_panel.hip) -> the kernels' uint32 [8] device buffer
    (include/cut3r_hip.h states its layout; gs_panel_ranges_decode gives floats).  The maps are fp32, equal in size, finite."""
    maps = [t for t in (a, b, alpha) if t is not None]
    _req(len(maps) > 0, "gs_panel_ranges: at least one map")
    n = maps[0].numel()
    _req(1 <= n < PANEL_MAX_PIXELS, f"gs_panel_ranges: 1 .. {PANEL_MAX_PIXELS - 1} elements")
    for t in maps:
        _map(t, "gs_panel_ranges", maps[0].shape, maps[0].device)
    ranges = torch.empty(8, dtype=torch.int32, device=maps[0].device)
    check(_lib.load().cut3r_gs_panel_ranges(_p(a), _p(b), _p(alpha), n, _p(ranges), _stream()), "cut3r_gs_panel_ranges")
    return ranges


def gs_panel_ranges_decode(ranges):
    """the uint32 [8] buffer of gs_panel_ranges as host fp32 [4,2] = (min, max) of a, b, |a - b|, alpha > 0.5 (NaN for a map not given)"""
    import numpy as np
    k = ranges.cpu().numpy().view(np.uint32).reshape(4, 2).copy()
    k[:, 0] = ~k[:, 0]
    bits = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7fffffff), ~k).astype(np.uint32)
    return bits.view(np.float32)


def gs_panel(gt, render, exposure_a, exposure_b, gt_depth, depth, normal, alpha, fx, fy, cx, cy):
    """the nine-cell diagnostic panel uint8 [3H,3W,3] of one view in two launches (include/cut3r_hip.h states the cells and their arithmetic,
    tests/gs_panel_oracle.py restates them): gt, render, normal fp32 [3,H,W]; gt_depth [H,W]; depth, alpha [1,H,W] or [H,W]; exposure_a
    [3,3], exposure_b [3]; all on one GPU, contiguous, finite."""
    _req(gt.dim() == 3 and gt.shape[0] == 3, "gt: [3,H,W]")
    H, W = int(gt.shape[1]), int(gt.shape[2])
    _req(H >= 1 and W >= 1 and H * W < PANEL_MAX_PIXELS, "gs_panel: H, W >= 1 and H W < 2^26")
    dev = gt.device
    depth, alpha, gt_depth = depth.reshape(H, W), alpha.reshape(H, W), gt_depth.reshape(H, W)
    for t, name, shape in ((gt, "gt", (3, H, W)), (render, "render", (3, H, W)), (normal, "normal", (3, H, W)), (gt_depth, "gt_depth", (H, W)),
                           (depth, "depth", (H, W)), (alpha, "alpha", (H, W)), (exposure_a, "exposure_a", (3, 3)), (exposure_b, "exposure_b", (3,))):
        _map(t, name, shape, dev)
    _req(float(fx) != 0.0 and float(fy) != 0.0, "gs_panel: fx, fy != 0")
    ranges = gs_panel_ranges(gt_depth, depth, alpha)
    out = torch.empty(3 * H, 3 * W, 3, dtype=torch.uint8, device=dev)
    check(_lib.load().cut3r_gs_panel(_p(gt), _p(render), _p(exposure_a), _p(exposure_b), _p(gt_depth), _p(depth), _p(normal), _p(alpha), float(fx),
                                     float(fy), float(cx), float(cy), H, W, _p(ranges), _p(out), _stream()), "cut3r_gs_panel")
    return out


def gs_frame(src, layer, depth_range=None):
    """one layer of one image as uint8 [H,W,3] (csrc/gs_panel.hip, the panel's cell code): "rgb" and "normal" of src [3,H,W], "depth" of
    src [H,W] or [1,H,W] in turbo over the map's own range (depth_range None: one more launch, no host read) or over a fixed (near, far)"""
    _req(layer in FRAME_LAYERS, f"layer: one of {sorted(FRAME_LAYERS)}")
    code = FRAME_LAYERS[layer]
    if code == 1:
        _req(src.dim() in (2, 3) and (src.dim() == 2 or src.shape[0] == 1), "depth: [H,W] or [1,H,W]")
        src = src.reshape(src.shape[-2], src.shape[-1])
    else:
        _req(src.dim() == 3 and src.shape[0] == 3, f"{layer}: [3,H,W]")
    H, W = int(src.shape[-2]), int(src.shape[-1])
    _req(H >= 1 and W >= 1 and H * W < PANEL_MAX_PIXELS, "gs_frame: H, W >= 1 and H W < 2^26")
    _map(src, layer, src.shape)
    ranges, lo, hi = None, 0.0, 0.0
    if code == 1 and depth_range is None:
        ranges = gs_panel_ranges(src)
    elif code == 1:
        lo, hi = float(depth_range[0]), float(depth_range[1])
        import math
        _req(math.isfinite(lo) and math.isfinite(hi), "depth_range: finite (near, far)")
    out = torch.empty(H, W, 3, dtype=torch.uint8, device=src.device)
    check(_lib.load().cut3r_gs_frame(_p(src), code, H, W, _p(ranges), lo, hi, _p(out), _stream()), "cut3r_gs_frame")
    return out
