"""GPU: one iteration of the fused loop-closure optimiser over sim(3) (csrc/lc.hip: lc_adam_kernel<2> / lc_terms_adam_kernel<2>), element by
element, against its fp64 restatement (tests/lc_sim3_oracle.py; checked on the CPU by tests/test_lc_sim3_cpu.py), under the protocol of
tests/test_lc_step_gpu.py: cut3r_lc_optimize_sim3, cut3r_lc_optimize_terms_sim3, cut3r_transform_submaps and cut3r_scale_planes are called
through _lib.load() with the test's own xi, m, v, T, workspace and loss buffer.

Inputs (lc_sim3_oracle.CASE_TABLE): N in {1, 63, 64, 2047, 2048, 2049, 8*2048+5}, B in {2, 3, 5}, the later-loop term list (P = 6, 7 terms) and
one with ia == ic terms; xi rows with |phi| in {0, 1e-4, 0.29, 0.31, 1, 2.5}, |tau| in {0, 1}, sigma in {0, 1e-4, +-0.05, 0.1, +-0.29, +-0.31,
0.7}, on both sides of both series switches of liemath::sim3_coeffs; residuals planted at >= 1e-3 (5e-2 for three steps).

Bounds:
  workspace rows, loss_out     DERIVED, those of tests/test_lc_step_gpu.py (the accumulate launch is the shared one; the rows of a sim(3) and
                               of an se(3) call on the same inputs at T = identity are bit-equal).
  m', v', xi', T', g           MEASURED: 4 x the worst distance of the fp32 CPU restatement from the fp64 oracle over all one-step cases
                               (the project's factor, from tests/test_lc_step_gpu.py).  Measured (CPU, lc_sim3_oracle.measure_margins):
                               xi 5.9e-8, T 6.6e-7, m 8.8e-8, v 9.5e-8, g 8.8e-7; after three steps from zero state xi 3.4e-10 (2.4e-10
                               on a second host: torch's fp32 sums depend on its thread count), T 1.1e-7.
  transform_submaps            DERIVED: 4 * 2^-24 * (sum_j |T_ij||p_j| + |t_i|) per coordinate, T = [sR | t] with s = 0.5 and 2.
  scale_planes                 EXACT: one fp32 multiply per element, the bits of torch's product.
Worst the kernels showed on an MI355X, as a fraction of the bound (nothing within 3 x of one):
  rows 0.074, loss_out 0.111 one step / 0.047 third step; of 4 x the fp32 distance: xi' 0.250, T' 0.151, m' 0.294, v' 0.265, g 0.294
  (no trend across the series switches); after three steps xi 2.8e-10 = 0.289, T 5.2e-8 = 0.117; transform_submaps with scales 0.5 / 2:
  0.637 (per = 262151); scale_planes bit-equal.
"""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from cut3r_slam_amd import _lib  # noqa: E402
from tests import lc_sim3_oracle as Q  # noqa: E402
from tests import lc_step_oracle as S  # noqa: E402
from tests import test_lc_step_gpu as G  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")
U = S.U
_p, _stream, _same_bits = G._p, G._stream, G._same_bits
ERR_ARG = 1


def _state(cs, zero_state, K):
    z = torch.zeros(cs.P, K)
    m0, v0 = (z, z) if zero_state else (cs.m0, cs.v0)
    xi = cs.xi if cs.xi.shape[1] == K else torch.zeros(cs.P, K)
    assert xi.shape[1] == K and m0.shape[1] == K
    return [x.to(DEV).clone().contiguous() for x in (xi, m0, v0, cs.T)]


def _fn(lib, base, group):
    return getattr(lib, base + ("_sim3" if group == "sim3" else ""))


def run_chain(cs, iters=1, zero_state=False, ws_fill=NAN, group="sim3"):
    lib = _lib.load()
    B, N = cs.P, cs.N
    sub = cs.sub.to(DEV).contiguous()
    n_masked = (B - 1) * N if cs.mask is None else int((cs.mask != 0).sum())
    mask_d = None if cs.mask is None else cs.mask.to(DEV).contiguous()
    assert mask_d is None or (mask_d.dtype == torch.uint8 and mask_d.shape == (B - 1, N))
    cur, cur_lc = cs.cur.to(DEV).contiguous(), cs.cur_lc.to(DEV).contiguous()
    xi, m, v, T = _state(cs, zero_state, 7 if group == "sim3" else 6)
    nws = lib.cut3r_lc_workspace_floats(B, N)
    assert nws == B * S.nblk(N) * S.LC_ROW
    ws = torch.full((nws,), ws_fill, device=DEV)
    loss = torch.full((max(iters, 1),), NAN, device=DEV)
    last = C.c_void_p(sub.data_ptr() + 5 * N * 3 * 4)
    rc = _fn(lib, "cut3r_lc_optimize", group)(_p(sub), last, 6 * N * 3, _p(mask_d), _p(cur), _p(cur_lc), B, N, n_masked, iters, S.LR,
                                              _p(xi), _p(m), _p(v), _p(T), _p(ws), _p(loss), _stream())
    assert rc == 0, f"cut3r_lc_optimize ({group}) returned {rc}"
    return G._out(xi, m, v, T, ws, loss, B)


def _terms_dev(cs):
    N, n = cs.N, len(cs.terms)
    arr = (_lib.LcTerm * n)()
    keep = []
    for t, (a, ia, c, ic, w, mk) in enumerate(cs.terms):
        a, c, mk = a.to(DEV).contiguous(), c.to(DEV).contiguous(), (None if mk is None else mk.to(DEV).contiguous())
        assert a.numel() == 3 * N and c.numel() == 3 * N and (mk is None or mk.numel() == N) and 0 <= ia < cs.P and 0 <= ic < cs.P
        keep.append((a, c, mk))
        arr[t].a, arr[t].c, arr[t].mask = a.data_ptr(), c.data_ptr(), (mk.data_ptr() if mk is not None else None)
        arr[t].ia, arr[t].ic, arr[t].w, arr[t].pad = ia, ic, w, 0
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV), keep


def run_terms(cs, iters=1, zero_state=False, ws_fill=NAN, group="sim3"):
    lib = _lib.load()
    N, n = cs.N, len(cs.terms)
    terms_dev, keep = _terms_dev(cs)
    xi, m, v, T = _state(cs, zero_state, 7 if group == "sim3" else 6)
    nws = lib.cut3r_lc_workspace_floats(n, N)
    assert nws == n * S.nblk(N) * S.LC_ROW
    ws = torch.full((nws,), ws_fill, device=DEV)
    loss = torch.full((max(iters, 1),), NAN, device=DEV)
    rc = _fn(lib, "cut3r_lc_optimize_terms", group)(_p(terms_dev), n, cs.P, N, iters, S.LR, _p(xi), _p(m), _p(v), _p(T), _p(ws), _p(loss),
                                                    _stream())
    assert rc == 0, f"cut3r_lc_optimize_terms ({group}) returned {rc}"
    return G._out(xi, m, v, T, ws, loss, n)


def run(cs, **kw):
    return run_chain(cs, **kw) if cs.kind == "chain" else run_terms(cs, **kw)


def check_state(tag, got, h64, m0):
    w = Q.measure_margins()
    for k in ("xi", "m", "v", "T"):
        assert torch.isfinite(got[k]).all(), f"{tag}: non-finite {k}"
    d = S.scaled_distance(got, h64, m0)
    frac = {k: d[k] / (4 * w[k]) for k in d}
    for k in d:
        print(f"[lc sim3] {tag}: {k} {d[k]:.3e} = {frac[k]:.3f} of 4 x {w[k]:.2e}")
    bad = {k: f"{d[k]:.3e} = {frac[k]:.2f} of 4 x {w[k]:.2e}" for k in d if frac[k] > 1}
    assert not bad, f"{tag}: {bad}"
    return frac


# ------------------------------------------------------------------------------------------------ one step, every element
@pytest.mark.parametrize("name", Q.ONE_STEP)
def test_one_step_per_element(name):
    cs = Q.get_case(name)
    h = Q.reference(name)[0]
    got = run(cs)
    f_rows = G.check_rows(name, got, h["R"])
    f_loss = G.check_loss(name, got, h["R"])
    print(f"\n[lc sim3] {name}: rows {f_rows:.3f} of the bound, loss {f_loss:.3f}")
    check_state(name, got, h, cs.m0)
    G.check_row0(name, cs, got, cs.m0, cs.v0)
    # the same bits from a zero-filled workspace (its padding is never read) and run to run
    _same_bits(got, run(cs, ws_fill=0.0))
    again = run(cs)
    _same_bits(got, again)
    assert torch.equal(got["ws"][:, :, :25].view(torch.int32), again["ws"][:, :, :25].view(torch.int32))


# ------------------------------------------------------------------------------------------------ three steps from zero state
@pytest.mark.parametrize("name", Q.THREE_STEP)
def test_three_steps_from_zero_state(name):
    """pins step + 1 in both bias corrections (the first step from m = v = 0 is lr * sign(g) whatever they are)"""
    cs = Q.get_case(name)
    hist = Q.reference(name)
    w = Q.measure_margins()
    got = run(cs, iters=3, zero_state=True)
    last = hist[-1]
    d_xi = float((got["xi"].double() - last["xi"]).abs().max())
    d_T = float((got["T"].double().reshape(-1, 12) - last["T"].reshape(-1, 12)).abs().max())
    ones = torch.ones(cs.P, 3, 4, dtype=torch.float64)
    f_loss = []
    for k, h in enumerate(hist):
        extra = 4 * w["T3"] * float(S.accum_rows(cs.terms, ones, cs.N).rmag.sum()) if k else 0.0
        f_loss.append(G.check_loss(f"{name} step {k}", got, h["R"], k, extra))
    print(f"\n[lc sim3] {name}: after 3 steps xi {d_xi:.3e} = {d_xi / (4 * w['xi3']):.3f} of 4 x {w['xi3']:.2e}, "
          f"T {d_T:.3e} = {d_T / (4 * w['T3']):.3f} of 4 x {w['T3']:.2e}; loss per step {['%.3f' % f for f in f_loss]} of the bound")
    assert d_xi <= 4 * w["xi3"] and d_T <= 4 * w["T3"], f"{name}: xi {d_xi:.3e} (4 x {w['xi3']:.2e}), T {d_T:.3e} (4 x {w['T3']:.2e})"
    G.check_row0(name, cs, got, torch.zeros(cs.P, 7), torch.zeros(cs.P, 7))
    _same_bits(got, run(cs, iters=3, zero_state=True, ws_fill=0.0))


# ------------------------------------------------------------------------------------------------ the accumulate path is the shared one
@pytest.mark.parametrize("name", ["chain3-N2049-B3", "terms3-later-loop"])
def test_rows_equal_the_se3_calls_at_identity(name):
    cs = Q.get_case(name)
    assert not cs.xi.any()
    a = run(cs, zero_state=True, group="sim3")
    b = run(cs, zero_state=True, group="se3")
    assert torch.equal(a["ws"][:, :, :25].view(torch.int32), b["ws"][:, :, :25].view(torch.int32))
    assert torch.equal(a["loss"].view(torch.int32), b["loss"].view(torch.int32))
    # the first step from zero state is lr * sign(g) up to eps / |g|: the six shared components agree to that
    assert float((a["xi"][:, :6] - b["xi"]).abs().max()) < 1e-3 * S.LR


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors_return_err_arg():
    lib = _lib.load()
    cs = Q.get_case("chain-N63-B3")
    B, N = cs.P, cs.N
    sub = cs.sub.to(DEV).contiguous()
    cur, cur_lc = cs.cur.to(DEV).contiguous(), cs.cur_lc.to(DEV).contiguous()
    xi, m, v, T = _state(cs, False, 7)
    keep0 = [x.clone() for x in (xi, m, v, T)]
    ws = torch.zeros(lib.cut3r_lc_workspace_floats(B, N), device=DEV)
    last = C.c_void_p(sub.data_ptr() + 5 * N * 3 * 4)
    good = [_p(sub), last, 6 * N * 3, _p(None), _p(cur), _p(cur_lc), B, N, (B - 1) * N, 1, S.LR, _p(xi), _p(m), _p(v), _p(T), _p(ws), _p(None),
            _stream()]
    for i in (0, 1, 4, 5, 11, 12, 13, 14, 15):
        bad = list(good)
        bad[i] = _p(None)
        assert lib.cut3r_lc_optimize_sim3(*bad) == ERR_ARG, f"null argument {i}"
    for i, val in ((6, 1), (7, 0), (7, -3), (8, -1), (9, -1)):
        bad = list(good)
        bad[i] = val
        assert lib.cut3r_lc_optimize_sim3(*bad) == ERR_ARG, f"argument {i} = {val}"
    ct = Q.get_case("terms-same-index")
    terms_dev, keep = _terms_dev(ct)
    n = len(ct.terms)
    xt, mt, vt, Tt = _state(ct, False, 7)
    wst = torch.zeros(lib.cut3r_lc_workspace_floats(n, ct.N), device=DEV)
    good_t = [_p(terms_dev), n, ct.P, ct.N, 1, S.LR, _p(xt), _p(mt), _p(vt), _p(Tt), _p(wst), _p(None), _stream()]
    for i in (0, 6, 7, 8, 9, 10):
        bad = list(good_t)
        bad[i] = _p(None)
        assert lib.cut3r_lc_optimize_terms_sim3(*bad) == ERR_ARG, f"terms: null argument {i}"
    for i, val in ((1, 0), (2, 1), (3, 0), (4, -1)):
        bad = list(good_t)
        bad[i] = val
        assert lib.cut3r_lc_optimize_terms_sim3(*bad) == ERR_ARG, f"terms: argument {i} = {val}"
    pl, sc = torch.ones(2, 5, device=DEV), torch.ones(2, device=DEV)
    for args in ((_p(None), _p(sc), 2, 5), (_p(pl), _p(None), 2, 5), (_p(pl), _p(sc), 0, 5), (_p(pl), _p(sc), 2, 0), (_p(pl), _p(sc), 65536, 5)):
        assert lib.cut3r_scale_planes(*args, _stream()) == ERR_ARG
    torch.cuda.synchronize()
    # nothing was launched: the state is untouched
    for a, b in zip((xi, m, v, T), keep0):
        assert torch.equal(a, b)
    assert torch.equal(pl.cpu(), torch.ones(2, 5))
    # iters = 0 is valid and writes nothing
    good[9] = 0
    assert lib.cut3r_lc_optimize_sim3(*good) == 0
    torch.cuda.synchronize()
    for a, b in zip((xi, m, v, T), keep0):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ transform_submaps with a similarity
@pytest.mark.parametrize("per", [257, 262144 + 7])
def test_transform_submaps_with_scales_half_and_two(per):
    lib = _lib.load()
    g = torch.Generator().manual_seed(per)
    B = 3
    xi = torch.zeros(B, 7, dtype=torch.float64)
    for b, (phi_n, tau_n, sig) in enumerate([(2.5, 1.0, math.log(0.5)), (0.0, 0.0, 0.0), (0.29, 1.0, math.log(2.0))]):
        xi[b, :3], xi[b, 3:6], xi[b, 6] = tau_n * S._unit(g), phi_n * S._unit(g), sig
    T64 = Q.matrix7(xi)[:, :3, :]
    T64[1] = torch.eye(4, dtype=torch.float64)[:3]
    assert float((Q.scale_of(T64) - torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)).abs().max()) < 1e-12
    T = T64.float().reshape(B, 12).contiguous()
    pts = torch.stack([S._points(per, g) for _ in range(B)])
    dev = pts.to(DEV).contiguous()
    assert lib.cut3r_transform_submaps(_p(dev), _p(T.to(DEV)), B, per, _stream()) == 0
    torch.cuda.synchronize()
    got = dev.cpu()
    Td, p = T.double().reshape(B, 3, 4), pts.double()
    ref = torch.einsum("bij,bnj->bni", Td[:, :, :3], p) + Td[:, None, :, 3]
    bound = 4 * U * (torch.einsum("bij,bnj->bni", Td[:, :, :3].abs(), p.abs()) + Td[:, None, :, 3].abs())
    frac = float(((got.double() - ref).abs() / bound).max())
    print(f"\n[lc sim3] transform_submaps, scales 0.5 / 1 / 2, per {per}: {frac:.3f} of the bound")
    assert frac <= 1
    assert torch.equal(got[1].view(torch.int32), pts[1].view(torch.int32))


# ------------------------------------------------------------------------------------------------ scale_planes
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("per", [1, 255, 257, 262144 + 7])            # the last: a second pass of the grid-stride loop for a few blocks
def test_scale_planes_is_one_fp32_multiply(n, per):
    lib = _lib.load()
    g = torch.Generator().manual_seed(10 * per + n)
    planes = torch.randn(n + 2, per, generator=g) * 3                 # guard planes before and after
    planes[:, ::7] = 0.0
    planes[:, 3::11] *= 1e-30
    scale = torch.tensor([1.1000001, 1.0, 0.73][:n]) if n > 1 else torch.tensor([0.9090909])
    dev = planes.to(DEV).contiguous()
    view = dev[1:1 + n]
    assert lib.cut3r_scale_planes(_p(view), _p(scale.to(DEV)), n, per, _stream()) == 0
    torch.cuda.synchronize()
    got = dev.cpu()
    ref = planes.clone()
    ref[1:1 + n] = planes[1:1 + n] * scale[:, None]
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
    if n > 1:
        assert torch.equal(got[2].view(torch.int32), planes[2].view(torch.int32))        # a scale of exactly 1
