"""GPU: attention over ONE key as a copy (cut3r_attention_one_key_f16 / ops.attention_one_key).

With Nk = 1 the softmax is exp2(s - s) / 1 = 1 for every finite score, P = fp16(1), and the PV product accumulates 1 * v + 0: the general
kernel writes the value row of (b, h) into every query row, bit for bit.  So every comparison here is torch.equal against
cut3r_attention_f16 itself, for the register-staged kernel (heads of 128, and 48 / 64 with cut3r_attention_variant(0)) and for the
pipelined kernel (48 / 64 by default).
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from cut3r_slam_amd import _lib, ops  # noqa: E402

DEV = "cuda:0"
F16 = torch.float16


def _values(B, H, D, seed):
    """a [B,1,2,H,D] k|v buffer: random values, and in every value row +-65504 (the largest fp16), +-2^-24 (the smallest subnormal), a larger
    subnormal and both zeros"""
    g = torch.Generator().manual_seed(seed)
    kv = torch.randn(B, 1, 2, H, D, generator=g).half()
    edge = torch.tensor([65504.0, -65504.0, 2.0 ** -24, -2.0 ** -24, 3 * 2.0 ** -20, 0.0, -0.0, 1.0], dtype=F16)
    kv[:, 0, 1, :, :8] = edge
    kv[:, 0, 1, :, D - 8:] = edge.flip(0)
    return kv.to(DEV)


@pytest.mark.parametrize("D", [48, 64, 128])
@pytest.mark.parametrize("Nq", [1, 5, 130])
@pytest.mark.parametrize("B,H", [(1, 1), (2, 3)])
def test_one_key_equals_the_general_kernel_bit_for_bit(B, H, Nq, D):
    kv = _values(B, H, D, 7 * D + Nq + B)
    k, v = kv[:, :, 0], kv[:, :, 1]                     # strided slices of the k|v buffer, as the decoder passes them
    assert not v.is_contiguous() or B * H == 1
    g = torch.Generator().manual_seed(Nq)
    q = torch.randn(B, Nq, H, D, generator=g).half().to(DEV)
    lib = _lib.load()
    refs = []
    variants = (1, 0) if D in (48, 64) else (1,)
    prev = lib.cut3r_attention_variant(-1)
    try:
        for var in variants:
            lib.cut3r_attention_variant(var)
            ref = torch.full((B, Nq, H, D), float("nan"), dtype=F16, device=DEV)
            ops.attention(q, k, v, ref, D ** -0.5)
            refs.append(ref)
    finally:
        lib.cut3r_attention_variant(prev)
    out = torch.full((B, Nq, H, D), float("nan"), dtype=F16, device=DEV)
    ops.attention_one_key(v, out)
    torch.cuda.synchronize()
    want = v.expand(B, Nq, H, D)
    print(f"[one key] B={B} H={H} Nq={Nq} D={D}: differs from v at {int((out.view(torch.int16) != want.contiguous().view(torch.int16)).sum())}, "
          + ", ".join(f"general kernel (variant {var}) differs at {int((r.view(torch.int16) != out.view(torch.int16)).sum())}" for var, r in zip(variants, refs)))
    assert torch.equal(out.view(torch.int16), want.contiguous().view(torch.int16))          # bits (keeps -0 and the subnormals apart)
    for r in refs:          # (as values: 1 * -0 + 0 may be +0 in the general kernel's accumulator)
        assert torch.equal(out, r)


def test_a_strided_output_keeps_its_other_slices():
    B, H, Nq, D = 2, 3, 5, 64
    v = _values(B, H, D, 1)[:, :, 1]
    big = torch.full((B, 3, Nq, H, D), -7.0, dtype=F16, device=DEV)
    ops.attention_one_key(v, big[:, 1])
    torch.cuda.synchronize()
    assert torch.equal(big[:, 1], v.expand(B, Nq, H, D))
    assert bool((big[:, 0] == -7.0).all()) and bool((big[:, 2] == -7.0).all())


def test_refusals_leave_the_output_alone():
    """null pointers, D % 8 != 0, D > 256, B, H, Nq <= 0, misaligned pointers or strides: CUT3R_ERR_ARG (1) before any launch, the
    sentinel-filled output untouched; the same call with none of these is accepted"""
    lib = _lib.load()
    B, H, Nq, D = 2, 3, 5, 64
    kv = _values(B, H, D, 2)
    v = kv[:, :, 1]
    out = torch.full((B * Nq * H * D + 64,), -7.0, dtype=F16, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok = dict(v=v.data_ptr(), o=out.data_ptr(), B=B, H=H, Nq=Nq, D=D, v_sb=v.stride(0), v_sn=v.stride(1), o_sb=Nq * H * D, o_sn=H * D)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cut3r_attention_one_key_f16(C.c_void_p(a["v"]), C.c_void_p(a["o"]), a["B"], a["H"], a["Nq"], a["D"], a["v_sb"], a["v_sn"],
                                               a["o_sb"], a["o_sn"], stream)

    cases = {"null v": dict(v=0), "null out": dict(o=0), "D % 8": dict(D=60), "D > 256": dict(D=264), "D = 0": dict(D=0),
             "B = 0": dict(B=0), "H = 0": dict(H=0), "Nq = 0": dict(Nq=0), "B < 0": dict(B=-1), "H < 0": dict(H=-2), "Nq < 0": dict(Nq=-5),
             "misaligned v": dict(v=v.data_ptr() + 8), "misaligned out": dict(o=out.data_ptr() + 8),
             "v batch stride": dict(v_sb=v.stride(0) + 4), "v key stride": dict(v_sn=v.stride(1) + 4),
             "out batch stride": dict(o_sb=Nq * H * D + 4), "out row stride": dict(o_sn=H * D + 4),
             "out rows overlap": dict(o_sn=H * D - 8), "out batches overlap": dict(o_sb=H * D)}
    for name, kw in cases.items():
        rc = call(**kw)
        torch.cuda.synchronize()
        assert rc == 1, (name, rc)
        assert bool((out == -7.0).all()), name
    with pytest.raises(ValueError):           # ops refuses on the host what it can see there
        ops.attention_one_key(kv[:, :, 1, :, :60], out[:B * Nq * H * 60].view(B, Nq, H, 60))
    with pytest.raises(ValueError):
        ops.attention_one_key(torch.zeros(B, 2, H, D, dtype=F16, device=DEV), out[:B * Nq * H * D].view(B, Nq, H, D))
    assert bool((out == -7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    n = B * Nq * H * D
    assert torch.equal(out[:n].view(B, Nq, H, D), v.expand(B, Nq, H, D)) and bool((out[n:] == -7.0).all())
