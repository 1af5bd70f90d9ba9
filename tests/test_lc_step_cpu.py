"""CPU: the fp64 restatement of one loop-closure iteration (tests/lc_step_oracle.py) against torch.autograd / torch.optim.Adam on the loss
as oracle/lc_oracle.py writes it, and the conditions the seeded inputs of tests/test_lc_step_gpu.py have to meet (evaluated by the fp64
oracle on the fp32-rounded inputs: conditions on the inputs, not measurements of a kernel)."""
import numpy as np
import pytest
import torch

from oracle import lc_oracle as LO
from tests import lc_step_oracle as S

F64 = torch.float64


def _chain_loss(cs, p, mask):
    """loop_closure_init's loss (oracle/lc_oracle.py), at p instead of 0"""
    sub = cs.sub.to(F64)
    B = sub.shape[0]
    fl = torch.stack([sub[:, 0], sub[:, -1]], 1).reshape(B, 2, -1, 3)
    cur, cur_lc = cs.cur.to(F64).reshape(1, -1, 3), cs.cur_lc.to(F64).reshape(1, -1, 3)
    T = torch.matrix_exp(LO.twist(torch.cat([torch.zeros(1, 6, dtype=F64), p], 0)))
    R, t = T[:, :3, :3], T[:, :3, 3].unsqueeze(1)
    cur_al = torch.matmul(cur, R[-1].unsqueeze(0).transpose(1, 2)) + t[-1].unsqueeze(0)
    l_cur = (cur_al - cur_lc).abs().mean()
    fla = torch.matmul(fl, R.transpose(1, 2).unsqueeze(1)) + t.unsqueeze(1)
    l_fl = (fla[:-1, -1] - fla[1:, 0])[mask].abs().mean()
    return l_fl + l_cur


def _terms_loss(cs, p):
    """loop_closure's loss: a sum of means of |T[ia] a - T[ic] c| (the weight of a term is 1 / (3 * #terms * #points of its mean) here)"""
    T = torch.matrix_exp(LO.twist(torch.cat([torch.zeros(1, 6, dtype=F64), p], 0)))
    loss = 0
    for a, ia, c, ic, w, mk in cs.terms:
        r = a.to(F64) @ T[ia, :3, :3].T + T[ia, :3, 3] - (c.to(F64) @ T[ic, :3, :3].T + T[ic, :3, 3])
        if mk is not None:
            r = r[mk != 0]
        loss = loss + w * r.abs().sum()
    return loss


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("name", S.ONE_STEP)
@pytest.mark.parametrize("masked", [True, False])
def test_rows_gather_pullback_equal_autograd(name, masked):
    """rows -> gather -> pull-back at |phi| up to 2.5 = torch.autograd.grad of the fp64 loss, to 1e-12 relative; the rows' column 24 sums to the
    loss"""
    cs = S.get_case(name)
    if cs.kind == "chain":
        mask = cs.mask if masked and cs.mask is not None else (torch.ones(cs.P - 1, cs.N, dtype=torch.uint8) if masked else None)
        terms, _ = S.chain_terms(cs.sub[:, 0], cs.sub[:, 5], mask, cs.cur, cs.cur_lc)
        bmask = torch.ones(cs.P - 1, cs.N, dtype=torch.bool) if mask is None else mask != 0
        loss_fn = lambda p: _chain_loss(cs, p, bmask)
    else:
        g = torch.Generator().manual_seed(1)
        terms = [(a, ia, c, ic, w, (torch.rand(cs.N, generator=g) > 0.2).to(torch.uint8) if masked else None) for a, ia, c, ic, w, _ in cs.terms]
        cs2 = S.Case()
        cs2.terms = terms
        loss_fn = lambda p: _terms_loss(cs2, p)
    # T = matrix(exp(xi)) exactly here (the case's T is that, rounded to fp32: the signs are the same, |r| >= 1e-3)
    T = torch.matrix_exp(LO.twist(cs.xi.double()))[:, :3, :]
    R = S.accum_rows(terms, T, cs.N)
    _, _, _, _, g = S.adam_step(S.gather(R.rows, terms, cs.P), cs.xi, cs.m0, cs.v0, 0)
    p = cs.xi[1:].double().clone().requires_grad_(True)
    loss = loss_fn(p)
    ref, = torch.autograd.grad(loss, p)
    assert _rel(g[1:], ref) < 1e-12
    assert not g[0].any()
    assert abs(float(R.rows[:, :, 24].sum() - loss.detach())) < 1e-12 * float(loss.detach())
    assert (R.abssum + 1e-300 >= R.rows.abs()).all() and R.rows.shape == (len(terms), S.nblk(cs.N), 25)


@pytest.mark.parametrize("name", ["chain3-N2049-B3", "terms3-later-loop"])
def test_three_steps_from_zero_equal_torch_adam(name):
    """iterate() from xi = m = v = 0 against oracle/lc_oracle.py's own loops (torch.optim.Adam, fp64): xi to 1e-14, the losses to 1e-13"""
    cs = S.get_case(name)
    hist = S.reference(name)
    if cs.kind == "chain":
        xi, T, losses = LO.loop_closure_init(cs.sub.reshape(cs.P, 6, 1, cs.N, 3), cs.mask != 0, cs.cur, cs.cur_lc, 3, lr=S.LR)
    else:
        # (the generator draws independent points for every term, which loop_closure's shared maps cannot hold: its loss, a weighted sum
        # of L1 terms over two families of transforms, is restated on the term list)
        xi, losses = _adam_on_terms(cs, 3)
    np.testing.assert_allclose(hist[-1]["xi"].numpy(), xi.numpy(), rtol=0, atol=1e-14)
    np.testing.assert_allclose([float(h["loss"]) for h in hist], losses, rtol=1e-13)


def _adam_on_terms(cs, iters):
    p = torch.nn.Parameter(torch.zeros(cs.P - 1, 6, dtype=F64))
    opt = torch.optim.Adam([{"params": p, "lr": S.LR}])
    losses = []
    for _ in range(iters):
        opt.zero_grad()
        loss = _terms_loss(cs, p)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return torch.cat([torch.zeros(1, 6, dtype=F64), p.detach()], 0), losses


def test_three_adam_steps_equal_torch_optim_adam():
    """adam_step alone, three times from zero state on seeded gradients G (non-zero xi along the way), against torch.optim.Adam to 1e-14"""
    g = torch.Generator().manual_seed(5)
    P = 4
    Gs = [torch.randn(P, 12, generator=g, dtype=F64) for _ in range(3)]
    p = torch.nn.Parameter(torch.zeros(P - 1, 6, dtype=F64))
    opt = torch.optim.Adam([{"params": p, "lr": S.LR}])
    xi, m, v = torch.zeros(P, 6, dtype=F64), torch.zeros(P, 6, dtype=F64), torch.zeros(P, 6, dtype=F64)
    for k in range(3):
        opt.zero_grad()
        M = torch.matrix_exp(LO.twist(torch.cat([torch.zeros(1, 6, dtype=F64), p], 0)))[:, :3, :]
        (M * Gs[k].reshape(P, 3, 4)).sum().backward()
        opt.step()
        xi, m, v, T, _ = S.adam_step(Gs[k], xi, m, v, k)
        np.testing.assert_allclose(xi[1:].numpy(), p.detach().numpy(), rtol=0, atol=1e-14)
    np.testing.assert_allclose(T.numpy(), torch.matrix_exp(LO.twist(xi))[:, :3, :].numpy(), rtol=0, atol=1e-15)
    assert not xi[0].any() and not m[0].any() and not v[0].any()


def test_case_table_reaches_every_path():
    chain = [S.get_case(n) for n in S.ONE_STEP if n.startswith("chain")]
    terms = [S.get_case(n) for n in S.ONE_STEP if n.startswith("terms")]
    assert {c.N for c in chain} == {1, 63, 64, 2047, 2048, 2049, 8 * 2048 + 5, 17 * 2048} and {c.P for c in chain} == {2, 3, 5}
    for fam in (chain, terms):
        assert {i for c in fam for i in c.combos} == set(range(12)), "every (|phi|, |tau|) under both Adam kernels"
    assert any(len(c.terms) * S.nblk(c.N) > 64 for c in terms)
    assert any(ia == ic and ia > 0 for c in terms for _, ia, _, ic, _, _ in c.terms)
    assert any(ia == 0 and ic == 0 for c in terms for _, ia, _, ic, _, _ in c.terms)
    assert any(S.nblk(c.N) == 9 for c in chain) and any(S.nblk(c.N) == 17 for c in chain)
    # |phi| of every row is what the table says, on either side of the series switch
    for c in chain + terms:
        for b, cid in enumerate(c.combos, 1):
            assert abs(float(c.xi[b, 3:].double().norm()) - S.COMBOS[cid][0]) < 1e-6 * max(S.COMBOS[cid][0], 1e-3)
            assert abs(float(c.xi[b, :3].double().norm()) - S.COMBOS[cid][1]) < 1e-6


@pytest.mark.parametrize("name", S.CASE_NAMES)
def test_inputs_meet_their_conditions(name):
    cs = S.get_case(name)
    hist = S.reference(name)
    assert len(hist) == cs.iters
    # the minimum |r| is the planted margin (less the rounding of c to fp32, ~1e-6); exact zeros are the planted ones and nothing else;
    # over the iterations of a multi-step case no residual changes sign, and none comes closer to 0 than a fifth of the margin
    assert hist[0]["min_r"] >= 0.999 * cs.margin, (hist[0]["min_r"], cs.margin)
    for h in hist:
        assert h["same_signs"] and h["min_r"] >= 0.2 * cs.margin, h["min_r"]
    assert hist[0]["R"].n_zero == cs.planted
    if cs.name in ("chain-N2049-B5", "terms-same-index"):
        assert cs.planted > 0
    # T is matrix(exp(xi)) rounded to fp32; row 0 is the identity
    T = torch.matrix_exp(LO.twist(cs.xi.double()))[:, :3, :].reshape(cs.P, 12)
    assert float((cs.T.double() - T).abs().max()) <= 2.0 ** -24 * float(T.abs().max())
    assert torch.equal(cs.T[0], torch.eye(4)[:3].reshape(12)) and not cs.xi[0].any()
    # the fp32 restatement sees the same signs (so its distance from the oracle is rounding, not another objective)
    h32 = S.oracle_run(cs, torch.float32)
    for a, b in zip(h32, hist):
        assert all(torch.equal(x, y) for x, y in zip(a["R"].signs, b["R"].signs))
    # no component of a gradient that the first step from zero state normalises to +-lr is small enough to change sign in fp32
    if cs.iters > 1:
        for h in hist:
            g = h["g"][1:]
            assert float(g.abs().min()) > 1e-3 * float(g.abs().max())
    else:
        assert cs.m0[1:].abs().min() > 0 and cs.v0[1:].min() > 0


def test_measured_margins_print():
    """the fp32-vs-fp64 distances the GPU file's Adam margins rest on (4 x these); printed with -s, recorded in its docstring"""
    w = S.measure_margins()
    print("\n[lc step] fp32 CPU restatement vs fp64 oracle, worst over the cases: " + ", ".join(f"{k} {d:.2e}" for k, d in w.items()))
    assert set(w) == {"xi", "T", "m", "v", "g_from_m", "xi3", "T3"}
    # rounding-sized: a restatement this far from the oracle would make the margins meaningless
    assert all(0 < d < 1e-3 for d in w.values())
