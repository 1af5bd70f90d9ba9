"""GPU: the decoder's final norm written where its consumers read it (cut3r_layernorm_tokens / ops.layernorm_tokens).

The launch runs the row bodies of cut3r_layernorm (one device function per body, inlined by both kernels), so its outputs are the bits of
cut3r_layernorm followed by the four strided copies it replaces: every comparison is torch.equal, and the slices of the destinations
that belong to other views keep their sentinel.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from cut3r_slam_amd import _lib, ops  # noqa: E402

DEV = "cuda:0"
F16, F32 = torch.float16, torch.float32
V, VIEW = 3, 1          # the destinations are view VIEW of [Wn, V, ...] tensors
EPS = 1e-6


def _problem(Wn, N, Cc, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(Wn * (N + 1), Cc, generator=g) * torch.logspace(-2, 2, Wn * (N + 1)).view(-1, 1) + 0.3
    gamma, beta = 1 + 0.1 * torch.randn(Cc, generator=g), 0.1 * torch.randn(Cc, generator=g)
    return x.to(DEV), gamma.to(DEV), beta.to(DEV)


def _dests(Wn, N, Cc, with32):
    tok16 = torch.full((Wn, V, N, Cc), -7.0, dtype=F16, device=DEV)
    tok32 = torch.full((Wn, V, N, Cc), -7.0, dtype=F32, device=DEV) if with32 else None
    pose32 = torch.full((Wn, V, Cc), -7.0, dtype=F32, device=DEV)
    pose16 = torch.full((Wn, V, Cc), -7.0, dtype=F16, device=DEV)
    return tok16, tok32, pose32, pose16


@pytest.mark.parametrize("with32", [False, True])
@pytest.mark.parametrize("Cc", [768, 192])          # the fast row body | the generic one
@pytest.mark.parametrize("N", [1, 5])
def test_tokens_equal_layernorm_and_copies_bit_for_bit(N, Cc, with32):
    Wn = 2
    x, gamma, beta = _problem(Wn, N, Cc, 10 * N + Cc)
    # the launch and the copies this one replaces
    dn16 = torch.empty(Wn * (N + 1), Cc, dtype=F16, device=DEV)
    dn32 = torch.empty(Wn * (N + 1), Cc, dtype=F32, device=DEV)
    ops.layernorm(x, gamma, beta, EPS, dn16, dn32)
    r_tok16, r_tok32, r_pose32, r_pose16 = _dests(Wn, N, Cc, with32)
    dn16v, dn32v = dn16.view(Wn, N + 1, Cc), dn32.view(Wn, N + 1, Cc)
    r_tok16[:, VIEW].copy_(dn16v[:, 1:])
    if with32:
        r_tok32[:, VIEW].copy_(dn32v[:, 1:])
    r_pose32[:, VIEW].copy_(dn32v[:, 0])
    r_pose16[:, VIEW].copy_(dn16v[:, 0])
    tok16, tok32, pose32, pose16 = _dests(Wn, N, Cc, with32)
    ops.layernorm_tokens(x, gamma, beta, EPS, pose32[:, VIEW], pose16[:, VIEW], tok16[:, VIEW], tok32[:, VIEW] if with32 else None)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dn32).all()) and float(dn32.abs().max()) > 1.0
    pairs = [("tok16", tok16, r_tok16), ("pose32", pose32, r_pose32), ("pose16", pose16, r_pose16)] + ([("tok32", tok32, r_tok32)] if with32 else [])
    for name, got, ref in pairs:
        print(f"[ln tokens] N={N} C={Cc} tok32={with32} {name}: differs at {int((got != ref).sum())} / {got.numel()}")
    for name, got, ref in pairs:
        assert torch.equal(got, ref), name            # view VIEW: the norm's bits; the other views: the sentinel
        assert bool((got[:, VIEW] != -7.0).any()), name


def test_refusals_leave_the_outputs_alone():
    lib = _lib.load()
    Wn, N, Cc = 2, 5, 192
    x, gamma, beta = _problem(Wn, N, Cc, 3)
    tok16, tok32, pose32, pose16 = _dests(Wn, N, Cc, True)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok = dict(x=x.data_ptr(), ldx=Cc, g=gamma.data_ptr(), b=beta.data_ptr(), eps=EPS, Wn=Wn, N=N, C=Cc,
              p32=pose32[:, VIEW].data_ptr(), p32s=V * Cc, p16=pose16[:, VIEW].data_ptr(), p16s=V * Cc,
              t16=tok16[:, VIEW].data_ptr(), t16s=V * N * Cc, t32=tok32[:, VIEW].data_ptr(), t32s=V * N * Cc)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cut3r_layernorm_tokens(C.c_void_p(a["x"]), a["ldx"], C.c_void_p(a["g"]), C.c_void_p(a["b"]), a["eps"], a["Wn"], a["N"], a["C"],
                                          C.c_void_p(a["p32"]), a["p32s"], C.c_void_p(a["p16"]), a["p16s"], C.c_void_p(a["t16"]), a["t16s"],
                                          C.c_void_p(a["t32"]), a["t32s"], stream)

    cases = {"null x": dict(x=0), "null gamma": dict(g=0), "null beta": dict(b=0), "null pose32": dict(p32=0), "null pose16": dict(p16=0),
             "null tok16": dict(t16=0), "Wn = 0": dict(Wn=0), "N = 0": dict(N=0), "Wn < 0": dict(Wn=-1), "C % 4": dict(C=190), "C > 2048": dict(C=2052),
             "C = 0": dict(C=0), "ldx < C": dict(ldx=Cc - 4), "ldx % 4": dict(ldx=Cc + 2), "eps = 0": dict(eps=0.0), "eps NaN": dict(eps=float("nan")),
             "misaligned x": dict(x=x.data_ptr() + 8), "misaligned gamma": dict(g=gamma.data_ptr() + 4), "misaligned beta": dict(b=beta.data_ptr() + 8),
             "misaligned pose32": dict(p32=ok["p32"] + 8), "misaligned pose16": dict(p16=ok["p16"] + 4), "misaligned tok16": dict(t16=ok["t16"] + 2),
             "misaligned tok32": dict(t32=ok["t32"] + 4), "pose32 stride % 4": dict(p32s=V * Cc + 2), "pose16 stride % 4": dict(p16s=V * Cc + 1),
             "tok16 stride % 4": dict(t16s=V * N * Cc + 2), "tok32 stride % 4": dict(t32s=V * N * Cc + 3),
             "pose32 groups overlap": dict(p32s=Cc - 4), "pose16 groups overlap": dict(p16s=0), "tok16 groups overlap": dict(t16s=(N - 1) * Cc),
             "tok32 groups overlap": dict(t32s=Cc)}
    for name, kw in cases.items():
        rc = call(**kw)
        torch.cuda.synchronize()
        assert rc == 1, (name, rc)
        for t in (tok16, tok32, pose32, pose16):
            assert bool((t == -7.0).all()), name
    # ops.layernorm_tokens refuses on the host what it can see there
    with pytest.raises(ValueError):           # one row short
        ops.layernorm_tokens(x[:-1], gamma, beta, EPS, pose32[:, VIEW], pose16[:, VIEW], tok16[:, VIEW])
    with pytest.raises(ValueError):           # rows of a group not contiguous
        ops.layernorm_tokens(x, gamma, beta, EPS, pose32[:, VIEW], pose16[:, VIEW], torch.zeros(Wn, N, V, Cc, dtype=F16, device=DEV)[:, :, VIEW])
    with pytest.raises(ValueError):           # an fp16 tensor where the fp32 rows go
        ops.layernorm_tokens(x, gamma, beta, EPS, pose16[:, VIEW], pose16[:, VIEW], tok16[:, VIEW])
    for t in (tok16, tok32, pose32, pose16):
        assert bool((t == -7.0).all())
    assert call() == 0
    assert call(t32=0) == 0                   # the fp32 token output is optional
    torch.cuda.synchronize()
    for t in (tok16, tok32, pose32, pose16):
        assert bool((t[:, VIEW] != -7.0).any()) and bool((t[:, 0] == -7.0).all()) and bool((t[:, 2] == -7.0).all())
