"""GPU: one iteration of the fused loop-closure optimiser (csrc/lc.hip), element by element, against its fp64 restatement
(tests/lc_step_oracle.py; checked on the CPU by tests/test_lc_step_cpu.py).  cut3r_lc_optimize, cut3r_lc_optimize_terms and
cut3r_transform_submaps are called through _lib.load() with the test's own xi, m, v, T, workspace and loss buffer: ops.lc_optimize* zero the
state and keep m, v and the workspace to themselves.

Inputs (lc_step_oracle.CASE_TABLE): N in {1, 63, 64, 2047, 2048, 2049, 8*2048+5 (nblk 9), 17*2048}, B in {2, 3, 5}, term lists shaped like
the later-loop objective (P = 6, 7 terms), with ia == ic and ia == ic == 0 terms, and with 8 terms x 9 blocks = 72 workspace rows; xi rows
with |phi| in {0, 1e-4, 0.29, 0.31, 1, 2.5} x |tau| in {0, 1}, T = matrix(exp(xi)); residuals planted at >= 1e-3 (5e-2 for three steps) so
that fp32 and fp64 see the same signs, except points planted at exactly 0 where both transforms are the identity.

Bounds, per case family (each test prints its worst error as a fraction of the bound; see them with -s):
  workspace rows [term, block, 0..24] after iters = 1   DERIVED: 2 * 19 * 2^-24 * sum|term| per entry -- 8 sequential adds per thread, 6
      butterfly levels, 3 cross-wave adds, the multiply by w, + 1 for the product; column 24 (sum |r|) + 4 * 2^-24 * w sum(|T||p| + |c'|)
      for the rounding of the residual itself.  One point dropped or doubled at N = 2048 is ~5e-4 * sum|term|, the bound 2.3e-6 * sum|term|.
  loss_out[k]                                           DERIVED: 2 * (ceil(rows / 64) + 6) * 2^-24 * sum|column 24| against the kernel's own
      rows; against the oracle's loss the rows' bounds are added (and, after the first step, the T margin times w sum(|p| + 1)).
  m', v', xi', T', (m' - b1 m) / (1 - b1) = g           MEASURED: 4 x the worst distance of the fp32 CPU restatement from the fp64 oracle over all
      one-step cases (the kernels sum in another order than torch).  m', g per unit of the case's max |g|, v' per max |g|^2, xi', T' absolute.
      Measured (CPU, lc_step_oracle.measure_margins):  xi 5.5e-8, T 4.7e-7, m 9.4e-8, v 7.8e-8, g 9.4e-7; after three steps from zero
      state xi 2.5e-10, T 4.7e-8.
  transform_submaps                                     DERIVED: 4 * 2^-24 * (sum_j |T_ij||p_j| + |t_i|) per coordinate.
Worst the kernels showed on an MI355X, as a fraction of the bound (nothing within 1.6 x of one):
  rows 0.108 (N = 1; 0.003 .. 0.09 elsewhere), loss_out 0.115 one step / 0.117 third step; of 4 x the fp32 distance: xi' 0.250, T' 0.193,
  m' 0.305, v' 0.250, g 0.305 (no trend with |phi|: the closed-form branch of the pull-back at 0.31, 1, 2.5 sits where the series branch does);
  after three steps xi 2.4e-10 = 0.241, T 1.5e-8 = 0.080; n_masked = 0: 0.286; transform_submaps 0.614 (per = 262151, B = 3).
"""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from cut3r_slam_amd import _lib  # noqa: E402
from tests import lc_step_oracle as S  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")
U = S.U
ROW_DEPTH = 8 + 6 + 3 + 1 + 1          # see the docstring


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _state(cs, zero_state):
    z = torch.zeros(cs.P, 6)
    m0, v0 = (z, z) if zero_state else (cs.m0, cs.v0)
    return [x.to(DEV).clone().contiguous() for x in (cs.xi, m0, v0, cs.T)]


def _out(xi, m, v, T, ws, loss, rows):
    torch.cuda.synchronize()
    return dict(xi=xi.cpu(), m=m.cpu(), v=v.cpu(), T=T.cpu(), ws=ws.cpu().reshape(rows, -1, S.LC_ROW), loss=loss.cpu())


def run_chain(cs, iters=1, zero_state=False, mask="case", n_masked=None, ws_fill=NAN, slots=6):
    """cut3r_lc_optimize on the case's maps.  mask: 'case', None or a uint8 [B-1,N] tensor; slots: maps per submap in the store (`last` stays
    at slot 5)."""
    lib = _lib.load()
    B, N = cs.P, cs.N
    if slots == 6:
        sub = cs.sub.to(DEV).contiguous()
    else:
        sub = torch.randn(B, slots, N, 3, generator=torch.Generator().manual_seed(3))
        sub[:, :6] = cs.sub
        sub = sub.to(DEV).contiguous()
    mask = cs.mask if isinstance(mask, str) else mask
    if n_masked is None:
        n_masked = (B - 1) * N if mask is None else int((mask != 0).sum())
    mask_d = None if mask is None else mask.to(DEV).contiguous()
    assert mask_d is None or (mask_d.dtype == torch.uint8 and mask_d.shape == (B - 1, N))
    cur, cur_lc = cs.cur.to(DEV).contiguous(), cs.cur_lc.to(DEV).contiguous()
    xi, m, v, T = _state(cs, zero_state)
    nws = lib.cut3r_lc_workspace_floats(B, N)
    assert nws == B * S.nblk(N) * S.LC_ROW
    ws = torch.full((nws,), ws_fill, device=DEV)
    loss = torch.full((max(iters, 1),), NAN, device=DEV)
    last = C.c_void_p(sub.data_ptr() + 5 * N * 3 * 4)
    rc = lib.cut3r_lc_optimize(_p(sub), last, slots * N * 3, _p(mask_d), _p(cur), _p(cur_lc), B, N, n_masked, iters, S.LR,
                               _p(xi), _p(m), _p(v), _p(T), _p(ws), _p(loss), _stream())
    assert rc == 0, f"cut3r_lc_optimize returned {rc}"
    return _out(xi, m, v, T, ws, loss, B)


def run_terms(cs, iters=1, zero_state=False, ws_fill=NAN):
    lib = _lib.load()
    N, n = cs.N, len(cs.terms)
    arr = (_lib.LcTerm * n)()
    keep = []
    for t, (a, ia, c, ic, w, mk) in enumerate(cs.terms):
        a, c, mk = a.to(DEV).contiguous(), c.to(DEV).contiguous(), (None if mk is None else mk.to(DEV).contiguous())
        assert a.numel() == 3 * N and c.numel() == 3 * N and (mk is None or mk.numel() == N) and 0 <= ia < cs.P and 0 <= ic < cs.P
        keep.append((a, c, mk))
        arr[t].a, arr[t].c, arr[t].mask = a.data_ptr(), c.data_ptr(), (mk.data_ptr() if mk is not None else None)
        arr[t].ia, arr[t].ic, arr[t].w, arr[t].pad = ia, ic, w, 0
    terms_dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    xi, m, v, T = _state(cs, zero_state)
    nws = lib.cut3r_lc_workspace_floats(n, N)
    assert nws == n * S.nblk(N) * S.LC_ROW
    ws = torch.full((nws,), ws_fill, device=DEV)
    loss = torch.full((max(iters, 1),), NAN, device=DEV)
    rc = lib.cut3r_lc_optimize_terms(_p(terms_dev), n, cs.P, N, iters, S.LR, _p(xi), _p(m), _p(v), _p(T), _p(ws), _p(loss), _stream())
    assert rc == 0, f"cut3r_lc_optimize_terms returned {rc}"
    return _out(xi, m, v, T, ws, loss, n)


def run(cs, **kw):
    return run_chain(cs, **kw) if cs.kind == "chain" else run_terms(cs, **kw)


def _same_bits(a, b, keys=("xi", "m", "v", "T", "loss")):
    for k in keys:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{k}: bits differ"


def _row_bounds(R):
    bound = 2 * ROW_DEPTH * U * R.abssum
    bound[:, :, 24] += 4 * U * R.rmag
    return bound


def check_rows(tag, got, R):
    """every workspace entry against the oracle's rows; returns the worst error as a fraction of its bound"""
    ws = got["ws"][:, :, :25].double()
    assert torch.isfinite(ws).all(), f"{tag}: non-finite workspace entries"
    bound = _row_bounds(R)
    err = (ws - R.rows).abs()
    zero = R.abssum == 0
    assert not ws[zero].any(), f"{tag}: entries that nothing is added to are not exactly 0"
    frac = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
    i = torch.nonzero(err > bound)
    assert i.numel() == 0, f"{tag}: {len(i)} workspace entries above the bound, first [term, block, slot] = {i[0].tolist()}: " \
                           f"{float(ws[tuple(i[0])]):.9g} vs {float(R.rows[tuple(i[0])]):.9g} (bound {float(bound[tuple(i[0])]):.3g})"
    return frac


def check_loss(tag, got, R, k=0, extra=0.0):
    """loss_out[k] against the kernel's own column 24 (k = the last iteration only) and against the oracle's loss"""
    rows = R.rows.shape[0] * R.rows.shape[1]
    col = got["ws"][:, :, 24].double()
    lossrow = 2 * (math.ceil(rows / 64) + 6) * U * float(R.abssum[:, :, 24].sum())
    L = float(got["loss"][k])
    frac = 0.0
    if k == len(got["loss"]) - 1:
        frac = abs(L - float(col.sum())) / max(lossrow, 1e-300)
        assert frac <= 1, f"{tag}: loss_out[{k}] {L:.9g} vs the sum of column 24 {float(col.sum()):.9g}: {frac:.2f} of the bound"
    tol = lossrow + float(_row_bounds(R)[:, :, 24].sum()) + extra
    f2 = abs(L - float(R.rows[:, :, 24].sum())) / tol
    assert f2 <= 1, f"{tag}: loss_out[{k}] {L:.9g} vs the oracle's {float(R.rows[:, :, 24].sum()):.9g}: {f2:.2f} of the bound {tol:.3g}"
    return max(frac, f2)


def check_state(tag, cs, got, h64, m0):
    """m', v', xi', T' and the g recovered from m' within 4 x the measured fp32 distance; returns {quantity: fraction of that margin}"""
    w = S.measure_margins()
    for k in ("xi", "m", "v", "T"):
        assert torch.isfinite(got[k]).all(), f"{tag}: non-finite {k}"
    d = S.scaled_distance(got, h64, m0)
    frac = {k: d[k] / (4 * w[k]) for k in d}
    bad = {k: f"{d[k]:.3e} = {frac[k]:.2f} of 4 x {w[k]:.2e}" for k in d if frac[k] > 1}
    assert not bad, f"{tag}: {bad}"
    return frac


def check_row0(tag, cs, got, m0, v0):
    for k, ref in (("xi", cs.xi), ("m", m0), ("v", v0), ("T", cs.T)):
        assert torch.equal(got[k][0].view(torch.int32), ref[0].view(torch.int32)), f"{tag}: row 0 of {k} was written"


# ------------------------------------------------------------------------------------------------ one step, every element
@pytest.mark.parametrize("name", S.ONE_STEP)
def test_one_step_per_element(name):
    cs = S.get_case(name)
    h = S.reference(name)[0]
    got = run(cs)
    f_rows = check_rows(name, got, h["R"])
    f_loss = check_loss(name, got, h["R"])
    f_state = check_state(name, cs, got, h, cs.m0)
    check_row0(name, cs, got, cs.m0, cs.v0)
    print(f"\n[lc step] {name}: rows {f_rows:.3f} of the bound, loss {f_loss:.3f}, of 4 x the fp32 distance: "
          + ", ".join(f"{k} {v:.3f}" for k, v in f_state.items()))
    # the padding of the workspace rows is never read: same bits from a zero-filled workspace
    _same_bits(got, run(cs, ws_fill=0.0))


# ------------------------------------------------------------------------------------------------ three steps from zero state
@pytest.mark.parametrize("name", S.THREE_STEP)
def test_three_steps_from_zero_state(name):
    """pins step + 1 in both bias corrections (the first step from m = v = 0 is lr * sign(g) whatever they are)"""
    cs = S.get_case(name)
    hist = S.reference(name)
    w = S.measure_margins()
    got = run(cs, iters=3, zero_state=True)
    last = hist[-1]
    d_xi = float((got["xi"].double() - last["xi"]).abs().max())
    d_T = float((got["T"].double().reshape(-1, 12) - last["T"].reshape(-1, 12)).abs().max())
    # a T within its margin moves the loss by at most margin * w * sum over points and coordinates of (|p| + 1): rmag at |T| = 1
    ones = torch.ones(cs.P, 3, 4, dtype=torch.float64)
    f_loss = []
    for k, h in enumerate(hist):
        extra = 4 * w["T3"] * float(S.accum_rows(cs.terms, ones, cs.N).rmag.sum()) if k else 0.0
        f_loss.append(check_loss(f"{name} step {k}", got, h["R"], k, extra))
    print(f"\n[lc step] {name}: after 3 steps xi {d_xi:.3e} = {d_xi / (4 * w['xi3']):.3f} of 4 x {w['xi3']:.2e}, "
          f"T {d_T:.3e} = {d_T / (4 * w['T3']):.3f} of 4 x {w['T3']:.2e}; loss per step {['%.3f' % f for f in f_loss]} of the bound")
    assert d_xi <= 4 * w["xi3"] and d_T <= 4 * w["T3"], f"{name}: xi {d_xi:.3e} (4 x {w['xi3']:.2e}), T {d_T:.3e} (4 x {w['T3']:.2e})"
    check_row0(name, cs, got, torch.zeros(cs.P, 6), torch.zeros(cs.P, 6))


# ------------------------------------------------------------------------------------------------ masks and layout
MASK_CASE = "chain-N2049-B5"


def _with_mask(cs, mask):
    terms, n_masked = S.chain_terms(cs.sub[:, 0], cs.sub[:, 5], mask, cs.cur, cs.cur_lc)
    return terms, n_masked, S.oracle_run(cs, terms=terms)[0]


def test_null_mask_equals_all_ones_mask():
    cs = S.get_case("chain-N2048-B3")
    assert cs.mask is None
    a = run_chain(cs)
    b = run_chain(cs, mask=torch.ones(cs.P - 1, cs.N, dtype=torch.uint8))
    _same_bits(a, b)
    assert torch.equal(a["ws"][:, :, :25].view(torch.int32), b["ws"][:, :, :25].view(torch.int32))


def test_pair_with_all_zero_mask_writes_zero_rows():
    cs = S.get_case(MASK_CASE)
    mask = cs.mask.clone()
    mask[1] = 0
    terms, n_masked, h = _with_mask(cs, mask)
    got = run_chain(cs, mask=mask)
    assert not got["ws"][1, :, :25].any()
    f = check_rows("zero pair", got, h["R"])
    fs = check_state("zero pair", cs, got, h, cs.m0)
    print(f"\n[lc step] pair 1 masked out: rows {f:.3f} of the bound, state {max(fs.values()):.3f} of 4 x the fp32 distance")


def test_no_masked_point_at_all_leaves_the_cur_term():
    cs = S.get_case(MASK_CASE)
    mask = torch.zeros_like(cs.mask)
    terms, n_masked, h = _with_mask(cs, mask)
    assert n_masked == 0 and terms[0][4] == 0.0
    got = run_chain(cs, mask=mask)
    assert not got["ws"][:-1, :, :25].any()
    check_rows("n_masked 0", got, h["R"])
    check_loss("n_masked 0", got, h["R"])
    fs = check_state("n_masked 0", cs, got, h, cs.m0)
    print(f"\n[lc step] n_masked = 0: state {max(fs.values()):.3f} of 4 x the fp32 distance")


def test_mask_bytes_other_than_one_count_as_set():
    cs = S.get_case(MASK_CASE)
    ref = run_chain(cs)
    mask = cs.mask.clone()
    mask[:, ::2] *= 2
    mask[:, 1::2] *= 255
    assert set(mask.unique().tolist()) == {0, 2, 255}
    got = run_chain(cs, mask=mask)
    _same_bits(ref, got)
    assert torch.equal(ref["ws"][:, :, :25].view(torch.int32), got["ws"][:, :, :25].view(torch.int32))


def test_seven_slot_store_and_repeatability():
    cs = S.get_case(MASK_CASE)
    ref = run_chain(cs)
    for got in (run_chain(cs, slots=7), run_chain(cs)):
        _same_bits(ref, got)
        assert torch.equal(ref["ws"][:, :, :25].view(torch.int32), got["ws"][:, :, :25].view(torch.int32))
    ct = S.get_case("terms-72-rows")
    a, b = run_terms(ct), run_terms(ct)
    _same_bits(a, b)
    assert torch.equal(a["ws"][:, :, :25].view(torch.int32), b["ws"][:, :, :25].view(torch.int32))


# ------------------------------------------------------------------------------------------------ transform_submaps
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("per", [1, 255, 257, 262144 + 7])            # the last: a second pass of the grid-stride loop for a few blocks
def test_transform_submaps_per_coordinate(B, per):
    lib = _lib.load()
    g = torch.Generator().manual_seed(per + B)
    xi = torch.zeros(B, 6, dtype=torch.float64)
    for b, (phi_n, tau_n) in enumerate([(2.5, 1.0), (0.0, 0.0), (0.29, 1.0)][:B]):
        xi[b, :3], xi[b, 3:] = tau_n * S._unit(g), phi_n * S._unit(g)
    T64 = torch.matrix_exp(S.twist(xi))[:, :3, :]
    if B > 1:
        T64[1] = torch.eye(4, dtype=torch.float64)[:3]
    T = T64.float().reshape(B, 12).contiguous()
    pts = torch.stack([S._points(per, g) for _ in range(B)])                           # [B,per,3]
    dev = pts.to(DEV).contiguous()
    rc = lib.cut3r_transform_submaps(_p(dev), _p(T.to(DEV)), B, per, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    got = dev.cpu()
    Td, p = T.double().reshape(B, 3, 4), pts.double()
    ref = torch.einsum("bij,bnj->bni", Td[:, :, :3], p) + Td[:, None, :, 3]
    bound = 4 * U * (torch.einsum("bij,bnj->bni", Td[:, :, :3].abs(), p.abs()) + Td[:, None, :, 3].abs())
    frac = float(((got.double() - ref).abs() / bound).max())
    print(f"\n[lc step] transform_submaps B {B} per {per}: {frac:.3f} of the bound")
    assert frac <= 1
    if B > 1:
        assert torch.equal(got[1].view(torch.int32), pts[1].view(torch.int32))
