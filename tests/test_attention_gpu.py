"""GPU: every instance of the fused attention kernels against an fp64 reference, element by element, at its edges.

The library builds 11 instances (attention.hip): the register-staged attn_kernel<D, 2> and <D, 4> for D = 16, 32, 48, 64, <128, 4>, and
the pipelined attn_pipe_kernel for D = 48 and 64.  Each test here states which one it means to reach and asks the library
(cut3r_attention_kernel_for: 100 * pipelined + waves) whether it does.  tests/attention_oracle.py holds the reference, the derivation
of the per-element bound 3 * 2^-11 * A + 2^-24 (A = sum_j p_j |v_j|), the inputs and the matrix of shapes; tests/test_attention_cpu.py
shows on the CPU that this check separates the kernels' arithmetic (at most 1.53 units of 2^-11 A) from every named defect (at
least 74 x the bound).

Largest err / (2^-11 A) over all shapes of test_every_instance_stays_inside_the_fp64_bound, measured on an MI355X (bound: 3):

    instance           code   worst
    d16-staged-nw2        2   1.531
    d16-staged-nw4        4   1.707
    d32-staged-nw2        2   1.281
    d32-staged-nw4        4   1.617
    d48-pipelined       104   1.486
    d48-staged-nw2        2   1.486
    d48-staged-nw4        4   1.464
    d64-pipelined       104   1.119
    d64-staged-nw2        2   1.119
    d64-staged-nw4        4   1.697
    d128-staged-nw4       4   1.451

(The pipelined and the staged two-wave instance of a head width run the same cases and give the same bits, hence the same figure.  The
CPU emulation of the same arithmetic reaches 1.53: the kernels sit where the derivation puts them, and the third unit, allowed for the
fp32 terms, is not used up at these score magnitudes, |s| <= 35.)
"""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from cut3r_slam_amd import _lib, ops  # noqa: E402
from tests import attention_oracle as AO  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")
SENTINEL = -7.5                            # exact in fp16; no output of these inputs equals it by bits AND position everywhere


@pytest.fixture(autouse=True)
def _library_defaults():
    """the instance each test reaches is the library's own choice, not an environment override"""
    for name in ("CUT3R_ATTN_PIPE", "CUT3R_ATTN_NW4_MIN"):
        assert name not in os.environ, f"{name} is set: the tests would not reach the instances they name"
    lib = _lib.load()
    assert lib.cut3r_attention_variant(-1) == 1, "the pipelined kernel is the default"
    yield
    assert lib.cut3r_attention_variant(-1) == 1


class _variant:
    """run the body with the pipelined (1) or the staged (0) kernel serving the 48- and 64-wide heads; restored on exit"""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        self.lib = _lib.load()
        self.prev = self.lib.cut3r_attention_variant(self.v)
        return self.lib

    def __exit__(self, *exc):
        self.lib.cut3r_attention_variant(self.prev)
        return False


def _bits(t):
    return t.contiguous().view(torch.int16)


def _run(q, k, v, scale):
    """ops.attention on contiguous copies, into a NaN-filled buffer"""
    B, Nq, H, D = q.shape
    o = torch.full((B, Nq, H, D), NAN, dtype=torch.float16, device=DEV)
    ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), o, scale)
    torch.cuda.synchronize()
    return o.cpu()


# ------------------------------------------------------------------------------------------------ (a) reference, per instance
@pytest.mark.parametrize("name,D,pipelined,NW", AO.INSTANCES, ids=[i[0] for i in AO.INSTANCES])
def test_every_instance_stays_inside_the_fp64_bound(name, D, pipelined, NW):
    """Key counts 1, 2, the tile edge (63..66), two tiles and the fold (127..130), three tiles (193) x query counts 1, 33, 129 (128 for
    the 384-head instances); query counts 1, 31..33, 64, 65, 127..129 (idle waves, a clamped last row, a second query block) x key
    counts 65 (fold) and 130 (ragged); each with and without spiked keys; plus one case each at 0.5 and 1.5 times the scale D^-0.5.
    EVERY output element within 3 * 2^-11 * A + 2^-24 of the fp64 reference."""
    big = AO.many_heads(D, pipelined, NW)
    code = 100 * pipelined + NW
    todo = [(nq, nk, spikes, 1.0) for nq, nk in AO.shapes(big) for spikes in (False, True)]
    todo += [(nq, nk, False, mul) for nq, nk, mul in AO.SCALE_CASES]
    worst, worst_at = 0.0, ""
    with _variant(pipelined) as lib:
        for nq, nk, spikes, mul in todo:
            B, H = AO.heads(big, nq, nk)
            c = AO.case(B, H, nq, nk, D, spikes, mul)
            c.check_inputs()                                  # on the reference alone, before any kernel output exists
            assert lib.cut3r_attention_kernel_for(B, H, nq, D) == code, f"{c.name} does not reach {name}"
            got = _run(c.q, c.k, c.v, c.scale)
            u = float(AO.units(got, c.out, c.A).nan_to_num(nan=float("inf")).max())
            if u > worst:
                worst, worst_at = u, c.name
            err = (got.double() - c.out).abs()
            over = ~(err <= AO.bound(c.A))                    # (a NaN is over)
            if bool(over.any()):
                idx = tuple(int(i) for i in over.nonzero()[0])
                raise AssertionError(f"{name} {c.name}: {int(over.sum())}/{over.numel()} elements outside the bound; first at (b,row,h,d) = "
                                     f"{idx}: got {float(got[idx]):.6f} ref {float(c.out[idx]):.6f} bound {float(AO.bound(c.A)[idx]):.2e}; "
                                     f"worst err / (2^-11 A) = {u:.2f}")
    print(f"[attention] {name}: instance code {code}, {len(todo)} cases, worst err / (2^-11 A) = {worst:.3f} at {worst_at}")
    assert worst <= 3.0


# ------------------------------------------------------------------------------------------------ (b) layout
FAMILIES = [(16, 0), (32, 0), (48, 1), (48, 0), (64, 1), (64, 0), (128, 0)]               # (D, pipelined)
FAMILY_IDS = [f"d{D}-{'pipelined' if p else 'staged'}" for D, p in FAMILIES]


def _strided_operands(c):
    """q as [:, 1:Nq+1, :H] of a [B, Nq+2, H+1, D] buffer, k and v as the two halves of ONE [B, Nk+3, 2, H, D] buffer (rows 1:Nk+1);
    every element outside the views is NaN"""
    B, H, Nq, Nk, D = c.shape
    qb = torch.full((B, Nq + 2, H + 1, D), NAN, dtype=torch.float16)
    qb[:, 1:Nq + 1, :H] = c.q
    kvb = torch.full((B, Nk + 3, 2, H, D), NAN, dtype=torch.float16)
    kvb[:, 1:Nk + 1, 0] = c.k
    kvb[:, 1:Nk + 1, 1] = c.v
    qb, kvb = qb.to(DEV), kvb.to(DEV)
    return qb[:, 1:Nq + 1, :H], kvb[:, 1:Nk + 1, 0], kvb[:, 1:Nk + 1, 1]


def _into_sentinel_view(q, k, v, scale, B, H, Nq, D):
    """run into [:, 1:Nq+1, :H] of a sentinel-filled [B, Nq+2, H+1, D] buffer; returns the view's content after checking that every
    sentinel outside it is still there"""
    ob = torch.full((B, Nq + 2, H + 1, D), SENTINEL, dtype=torch.float16, device=DEV)
    ov = ob[:, 1:Nq + 1, :H]
    assert ov.stride(1) != H * D and ov.stride(0) != Nq * ov.stride(1)
    ops.attention(q, k, v, ov, scale)
    torch.cuda.synchronize()
    after = ob.cpu()
    got = after[:, 1:Nq + 1, :H].clone()
    after[:, 1:Nq + 1, :H] = SENTINEL
    touched = int((_bits(after) != _bits(torch.full_like(after, SENTINEL))).sum())
    assert touched == 0, f"{touched} elements outside the output view were written"
    return got


@pytest.mark.parametrize("D,pipelined", FAMILIES, ids=FAMILY_IDS)
@pytest.mark.parametrize("B,H,Nq,Nk", [(3, 5, 129, 65), (3, 5, 33, 130), (3, 5, 65, 65), (3, 5, 130, 130)])
def test_strided_operands_give_the_bits_of_the_contiguous_run_and_touch_nothing_else(B, H, Nq, Nk, D, pipelined):
    """a fold with a one-row query block and idle waves (129 x 65), a ragged tile under a two-wave block (33 x 130), and the two
    self-attention shapes for the [B,N,3,H,D] pack: strided q (token and batch stride), k and v strided separately inside one buffer,
    strided output, NaN everywhere outside the views -- the same bits as the contiguous run (itself inside the fp64 bound), and
    no write outside the output view."""
    c = AO.case(B, H, Nq, Nk, D, True)
    with _variant(pipelined) as lib:
        assert lib.cut3r_attention_kernel_for(B, H, Nq, D) == (104 if pipelined else (4 if D == 128 else 2))
        plain = _run(c.q, c.k, c.v, c.scale)
        assert bool(((plain.double() - c.out).abs() <= AO.bound(c.A)).all())
        q, k, v = _strided_operands(c)
        assert k.stride(0) != Nk * k.stride(1) and q.stride(0) != Nq * q.stride(1) and q.stride(1) != H * D
        got = _into_sentinel_view(q, k, v, c.scale, B, H, Nq, D)
        assert torch.equal(_bits(got), _bits(plain)), f"{int((_bits(got) != _bits(plain)).sum())} elements differ from the contiguous run"
        if Nq == Nk:
            pack = torch.full((B, Nq + 1, 3, H, D), NAN, dtype=torch.float16)
            pack[:, :Nq, 0], pack[:, :Nq, 1], pack[:, :Nq, 2] = c.q, c.k, c.v
            pack = pack.to(DEV)
            got = _into_sentinel_view(pack[:, :Nq, 0], pack[:, :Nq, 1], pack[:, :Nq, 2], c.scale, B, H, Nq, D)
            assert torch.equal(_bits(got), _bits(plain)), "the [B,N,3,H,D] pack differs from the contiguous run"


# ------------------------------------------------------------------------------------------------ (c) head isolation
@pytest.mark.parametrize("D,pipelined", FAMILIES, ids=FAMILY_IDS)
@pytest.mark.parametrize("Nk", [65, 130])
def test_a_head_does_not_depend_on_its_neighbours(Nk, D, pipelined):
    """15 (batch, head) pairs -- not a multiple of the pipelined kernel's XCD group of 8, so its grid is padded -- and two query blocks:
    the output of one pair is the same bits whatever the other 14 hold, NaN included.  First, middle and last pair."""
    B, H, Nq = 3, 5, 129
    c = AO.case(B, H, Nq, Nk, D, True)
    g = torch.Generator().manual_seed(D + Nk)
    with _variant(pipelined) as lib:
        assert lib.cut3r_attention_kernel_for(B, H, Nq, D) == (104 if pipelined else (4 if D == 128 else 2))
        base = _run(c.q, c.k, c.v, c.scale)
        for b, h in ((0, 0), (1, 2), (B - 1, H - 1)):
            # the replacement: fresh draws, NaN in every other pair counted from the chosen one's neighbours, the chosen pair itself kept
            q2, k2, v2 = (torch.randn(t.shape, generator=g).half() for t in (c.q, c.k, c.v))
            for t2, t in ((q2, c.q), (k2, c.k), (v2, c.v)):
                for bb in range(B):
                    for hh in range(H):
                        if (bb, hh) == (b, h):
                            t2[bb, :, hh] = t[bb, :, hh]
                        elif (bb * H + hh - b * H - h) % 2 == 1:
                            t2[bb, :, hh] = NAN
            other = _run(q2, k2, v2, c.scale)
            assert torch.equal(_bits(other[b, :, h]), _bits(base[b, :, h])), f"pair (b={b}, h={h}) changed with its neighbours' data"
            assert torch.isfinite(other[b, :, h]).all()


# ------------------------------------------------------------------------------------------------ (d) repeat launches
@pytest.mark.parametrize("B,H,Nq,Nk,D", [(8, 12, 257, 321, 64), (8, 16, 257, 321, 48)])
def test_pipelined_kernel_repeats_its_bits_over_16_launches(B, H, Nq, Nk, D):
    """the race screen of the LDS-DMA ring (hand-counted vmcnt, one barrier per tile): 16 back-to-back launches into four rotating
    buffers, three query blocks and a fold over five tiles; every result equals the first bit for bit"""
    g = torch.Generator().manual_seed(B + D)
    q = (torch.randn(B, Nq, H, D, generator=g) * 1.5).half().to(DEV)
    k = (torch.randn(B, Nk, H, D, generator=g) * 1.5).half().to(DEV)
    v = torch.randn(B, Nk, H, D, generator=g).half().to(DEV)
    lib = _lib.load()
    assert lib.cut3r_attention_kernel_for(B, H, Nq, D) == 104
    bufs = [torch.full((B, Nq, H, D), NAN, dtype=torch.float16, device=DEV) for _ in range(4)]
    kept = []
    for i in range(16):
        o = bufs[i % 4]
        ops.attention(q, k, v, o, D ** -0.5)
        kept.append(o.clone())                               # (stream-ordered: taken before the buffer's next launch)
    torch.cuda.synchronize()
    first = kept[0]
    assert torch.isfinite(first).all()
    for i, o in enumerate(kept[1:], 1):
        assert torch.equal(_bits(o), _bits(first)), f"launch {i}: {int((_bits(o) != _bits(first)).sum())} elements differ from launch 0"


# ------------------------------------------------------------------------------------------------ (e) refusals
def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    B, H, Nq, Nk, D = 2, 3, 33, 65, 64
    c = AO.case(B, H, Nq, Nk, D, False)
    pad = 64                                                 # spare elements behind every buffer: shifted pointers stay inside them
    def dev(t):
        buf = torch.zeros(t.numel() + pad, dtype=torch.float16, device=DEV)
        buf[:t.numel()] = t.reshape(-1).to(DEV)
        return buf
    q, k, v = dev(c.q), dev(c.k), dev(c.v)
    o = torch.full((B * Nq * H * D + pad,), SENTINEL, dtype=torch.float16, device=DEV)
    sq, sk = (Nq * H * D, H * D), (Nk * H * D, H * D)

    def call(qo=0, oo=0, D_=D, q_sn=sq[1], k_sn=sk[1], o_sn=sq[1], scale=D ** -0.5):
        rc = lib.cut3r_attention_f16(C.c_void_p(q.data_ptr() + qo), C.c_void_p(k.data_ptr()), C.c_void_p(v.data_ptr()),
                                     C.c_void_p(o.data_ptr() + oo), B, H, Nq, Nk, D_, sq[0], q_sn, sk[0], k_sn, sk[0], sk[1], sq[0], o_sn,
                                     C.c_float(scale), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc

    refused = {"q pointer off by 8 bytes": dict(qo=8), "k_sn not a multiple of 8": dict(k_sn=sk[1] + 4), "output pointer off by 4 bytes": dict(oo=4),
               "odd o_sn": dict(o_sn=sq[1] + 1), "D = 24": dict(D_=24), "scale 0": dict(scale=0.0), "scale -1": dict(scale=-1.0),
               "scale NaN": dict(scale=NAN), "scale inf": dict(scale=float("inf"))}
    for what, kw in refused.items():
        assert call(**kw) == 1, what
        assert bool((o == SENTINEL).all()), f"{what}: the output was written"
    assert lib.cut3r_attention_kernel_for(B, H, Nq, 24) == 0
    for bad in (0.0, -1.0, NAN, float("inf")):
        with pytest.raises((ValueError, _lib.Cut3rHipError)):
            ops.attention(c.q.to(DEV), c.k.to(DEV), c.v.to(DEV), torch.empty(B, Nq, H, D, dtype=torch.float16, device=DEV), bad)
    assert call() == 0                                       # the same call with valid arguments runs
    got = o[:B * Nq * H * D].view(B, Nq, H, D).cpu()
    assert bool(((got.double() - c.out).abs() <= AO.bound(c.A)).all())
    assert bool((o[B * Nq * H * D:] == SENTINEL).all())
