"""CPU: the fp64 restatement of the sim(3) loop-closure iteration (tests/lc_sim3_oracle.py) -- its analytic structure, its gradient, its
reduction to the se(3) oracle -- the conditions the seeded inputs of tests/test_lc_sim3_gpu.py have to meet, the condition under which the
mode is worth having (a planted scale drift is recovered where the rigid optimiser cannot), and the host pose rewrite.

Convergence scenario (lc_sim3_oracle.drift_scenario: B = 5, N = 257, noise 5 mm, 2000 iterations, lr 5e-4), measured with the seeded inputs:
  planted scale 1.1 at the loop: final loss sim(3) 0.0106 = 0.070 x the se(3) run's 0.1514 (cap 0.25 x); recovered scales within 1.7e-4
  relative of 1 / scale(A_p) (cap 2e-3);  no planted scale drift: sim(3) final loss 0.0111 = 1.000 x the se(3) one (cap 1.02 x), scales
  within 1.8e-4 of 1."""
import functools
import math

import numpy as np
import pytest
import torch

from cut3r_slam_amd import geom_host as gh
from oracle import lc_oracle as LO
from tests import lc_sim3_oracle as Q
from tests import lc_step_oracle as S

F64 = torch.float64


def _rand_xi(n, seed, sig=0.5):
    g = torch.Generator().manual_seed(seed)
    xi = torch.randn(n, 7, generator=g, dtype=F64)
    xi[:, 6] *= sig
    return xi


def test_matrix_exp_of_the_generator_is_sR_Wtau():
    """T = [e^sigma R | W tau]: the 3x3 block over e^sigma is orthonormal with det +1 and equals exp([phi]x); the translation is W tau with
    W = integral_0^1 exp(u (sigma I + [phi]x)) du (here: by 64-point Gauss-Legendre, exact to fp64 for these arguments)"""
    xi = _rand_xi(9, 0)
    xi[0, 3:6] = 0                       # pure scale
    xi[1, 6] = 0                         # rigid
    T = Q.matrix7(xi)
    s = torch.exp(xi[:, 6])
    R = T[:, :3, :3] / s[:, None, None]
    assert float((R @ R.transpose(1, 2) - torch.eye(3, dtype=F64)).abs().max()) < 1e-13
    assert float((torch.linalg.det(R) - 1).abs().max()) < 1e-13
    z = torch.zeros(9, 6, dtype=F64)
    z[:, 3:] = xi[:, 3:6]
    assert float((R - torch.matrix_exp(LO.twist(z))[:, :3, :3]).abs().max()) < 1e-13
    assert float((Q.scale_of(T) - s).abs().max()) < 1e-13
    assert float((T[:, 3] - torch.tensor([0, 0, 0, 1.0], dtype=F64)).abs().max()) == 0
    u, w = np.polynomial.legendre.leggauss(64)
    u, w = torch.from_numpy(0.5 * (u + 1)), torch.from_numpy(0.5 * w)
    gen = Q.twist7(xi)[:, :3, :3]
    W = (torch.matrix_exp(u[None, :, None, None] * gen[:, None]) * w[None, :, None, None]).sum(1)
    assert float((T[:, :3, 3] - (W @ xi[:, :3, None])[:, :, 0]).abs().max()) < 1e-12


def test_gradient_against_central_differences():
    g = torch.Generator().manual_seed(3)
    P = 5
    xi = _rand_xi(P, 4)
    G = torch.randn(P, 12, generator=g, dtype=F64)
    z = torch.zeros(P, 7, dtype=F64)
    grad = Q.adam_step7(G, xi, z, z, 0)[4]
    f = lambda x: float((Q.matrix7(x)[:, :3, :] * G.reshape(P, 3, 4)).sum())
    h = 1e-6
    for b in range(1, P):
        for k in range(7):
            d = torch.zeros(P, 7, dtype=F64)
            d[b, k] = h
            fd = (f(xi + d) - f(xi - d)) / (2 * h)
            assert abs(fd - float(grad[b, k])) < 1e-7 * max(1.0, abs(fd)), (b, k, fd, float(grad[b, k]))
    assert not grad[0].any()


def test_sigma_pinned_reproduces_the_se3_step():
    """sigma = 0 and a G whose sigma-gradient is 0 (the component of G along dT/dsigma removed): the first six columns are
    lc_step_oracle.adam_step's, the seventh stays 0"""
    g = torch.Generator().manual_seed(6)
    P = 4
    xi6 = torch.randn(P, 6, generator=g, dtype=F64)
    xi6[0] = 0
    xi7 = torch.cat([xi6, torch.zeros(P, 1, dtype=F64)], 1)
    G = torch.randn(P, 12, generator=g, dtype=F64)
    x = xi7.clone().requires_grad_(True)
    M = Q.matrix7(x)[:, :3, :]
    D = torch.stack([torch.autograd.grad(M[b].reshape(12)[k], x, retain_graph=True)[0][b, 6] for b in range(P) for k in range(12)]).reshape(P, 12)
    G = G - (G * D).sum(1, keepdim=True) / (D * D).sum(1, keepdim=True) * D
    m6, v6 = torch.randn(P, 6, generator=g, dtype=F64) * 0.1, torch.rand(P, 6, generator=g, dtype=F64) * 0.01
    z1 = torch.zeros(P, 1, dtype=F64)
    a = S.adam_step(G, xi6, m6, v6, 2)
    b = Q.adam_step7(G, xi7, torch.cat([m6, z1], 1), torch.cat([v6, z1], 1), 2)
    assert float(b[4][:, 6].abs().max()) < 1e-14
    for k, tol in ((0, 1e-14), (1, 1e-15), (2, 1e-15), (4, 1e-13)):
        assert float((b[k][:, :6] - a[k]).abs().max()) < tol, k
    assert float(b[0][:, 6].abs().max()) < 1e-9          # 0 / (0 + eps)
    assert float((b[3] - a[3]).abs().max()) < 1e-8


def test_case_table_covers_every_value_and_both_switches():
    chain = [Q.get_case(n) for n in Q.ONE_STEP if n.startswith("chain")]
    terms = [Q.get_case(n) for n in Q.ONE_STEP if n.startswith("terms")]
    assert {c.N for c in chain} == {1, 63, 64, 2047, 2048, 2049, 8 * 2048 + 5} and {c.P for c in chain} == {2, 3, 5}
    assert any(len(c.terms) == 7 and c.P == 6 for c in terms)
    assert any(ia == ic and ia > 0 for c in terms for _, ia, _, ic, _, _ in c.terms)
    need_sigma = {0.0, 1e-4, 0.05, -0.05, 0.29, -0.29, 0.31, -0.31, 0.7}
    for fam in (chain, terms):
        rows = [Q.ROWS[i] for c in fam for i in c.rows]
        assert {r[0] for r in rows} == set(Q.PHI) == {0.0, 1e-4, 0.29, 0.31, 1.0, 2.5}
        assert {r[1] for r in rows} == set(Q.TAU) == {0.0, 1.0}
        assert {r[2] for r in rows} >= need_sigma and {r[2] for r in rows} == set(Q.SIGMA)
        # both switches of sim3_coeffs (0.09) from each side, close to it
        sg2 = sorted(r[2] ** 2 for r in rows)
        c2 = sorted(r[0] ** 2 + r[2] ** 2 for r in rows)
        for v in (sg2, c2):
            assert any(0.08 < x < 0.09 for x in v) and any(0.09 < x < 0.1 for x in v)
    # the rows are what the table says
    for c in chain + terms:
        for b, rid in enumerate(c.rows, 1):
            phi, tau, sig = Q.ROWS[rid]
            assert abs(float(c.xi[b, 3:6].double().norm()) - phi) < 1e-6 * max(phi, 1e-3)
            assert abs(float(c.xi[b, :3].double().norm()) - tau) < 1e-6 and abs(float(c.xi[b, 6]) - sig) < 1e-7


@pytest.mark.parametrize("name", Q.CASE_NAMES)
def test_inputs_meet_their_conditions(name):
    cs = Q.get_case(name)
    hist = Q.reference(name)
    assert len(hist) == cs.iters
    assert hist[0]["min_r"] >= 0.99 * cs.margin, (hist[0]["min_r"], cs.margin)
    for h in hist:
        assert h["same_signs"] and h["min_r"] >= 0.2 * cs.margin, h["min_r"]
    assert hist[0]["R"].n_zero == 0
    T = Q.matrix7(cs.xi.double())[:, :3, :].reshape(cs.P, 12)
    assert float((cs.T.double() - T).abs().max()) <= 2.0 ** -24 * float(T.abs().max())
    assert torch.equal(cs.T[0], torch.eye(4)[:3].reshape(12)) and not cs.xi[0].any()
    h32 = Q.oracle_run(cs, torch.float32)
    for a, b in zip(h32, hist):
        assert all(torch.equal(x, y) for x, y in zip(a["R"].signs, b["R"].signs))
    if cs.iters > 1:
        for h in hist:
            g = h["g"][1:]
            assert float(g.abs().min()) > 1e-3 * float(g.abs().max())
    else:
        assert cs.m0[1:].abs().min() > 0 and cs.v0[1:].min() > 0


def test_rows_gather_pullback_equal_autograd():
    """rows -> gather -> sim(3) pull-back = torch.autograd.grad of the fp64 loss written out directly"""
    for name in ("chain-N64-B5", "terms-same-index"):
        cs = Q.get_case(name)
        T = Q.matrix7(cs.xi.double())[:, :3, :]
        R = S.accum_rows(cs.terms, T, cs.N)
        g = Q.adam_step7(S.gather(R.rows, cs.terms, cs.P), cs.xi, cs.m0, cs.v0, 0)[4]
        p = cs.xi[1:].double().clone().requires_grad_(True)
        Tp = Q.matrix7(torch.cat([torch.zeros(1, 7, dtype=F64), p], 0))
        loss = 0
        for a, ia, c, ic, w, mk in cs.terms:
            cp = c.to(F64) if ic is None else Q._apply(Tp[ic], c.to(F64))
            r = Q._apply(Tp[ia], a.to(F64)) - cp
            if mk is not None:
                r = r[mk != 0]
            loss = loss + w * r.abs().sum()
        ref, = torch.autograd.grad(loss, p)
        assert float((g[1:] - ref).abs().max()) < 1e-12 * float(ref.abs().max())


def test_measured_margins_print():
    w = Q.measure_margins()
    print("\n[lc sim3] fp32 CPU restatement vs fp64 oracle, worst over the cases: " + ", ".join(f"{k} {d:.2e}" for k, d in w.items()))
    assert set(w) == {"xi", "T", "m", "v", "g_from_m", "xi3", "T3"}
    assert all(0 < d < 1e-3 for d in w.values())


def test_k6_restatement_equals_the_se3_oracle():
    """the K = 6 form of this file's whole-optimisation restatement gives oracle/lc_oracle.loop_closure_init's numbers"""
    sub, mask, cur, cur_lc, _ = Q.drift_scenario(B=3, N=65, seed=2)
    a = LO.loop_closure_init(sub, mask, cur, cur_lc, 20)
    b = Q.loop_closure_init(sub, mask, cur, cur_lc, 20, K=6)
    assert float((a[0] - b[0]).abs().max()) < 1e-12
    np.testing.assert_allclose(a[2], b[2], rtol=1e-12)


# ------------------------------------------------------------------------------------------------ the condition the mode exists for
@functools.lru_cache(maxsize=None)
def _converged(total_scale):
    sub, mask, cur, cur_lc, sA = Q.drift_scenario(total_scale=total_scale)
    sim = Q.loop_closure_init(sub, mask, cur, cur_lc, 2000, K=7)
    se = Q.loop_closure_init(sub, mask, cur, cur_lc, 2000, K=6)
    return sim, se, sA


def test_sim3_recovers_a_planted_scale_drift_where_se3_cannot():
    (xi, T, l7), (_, _, l6), sA = _converged(1.1)
    s = Q.scale_of(T)
    rel = float((s * sA - 1).abs().max())
    print(f"\n[lc sim3] planted scale 1.1: final loss sim3 {l7[-1]:.4f} = {l7[-1] / l6[-1]:.3f} x se3 {l6[-1]:.4f}; scales within {rel:.2e}")
    assert l7[-1] <= 0.25 * l6[-1]
    assert rel <= 2e-3
    assert float((torch.exp(xi[:, 6]) - s).abs().max()) < 1e-12


def test_sim3_equals_se3_without_scale_drift():
    (_, T, l7), (_, _, l6), _ = _converged(1.0)
    print(f"\n[lc sim3] no planted scale: final loss sim3 {l7[-1]:.4f} = {l7[-1] / l6[-1]:.3f} x se3 {l6[-1]:.4f}; "
          f"scales within {float((Q.scale_of(T) - 1).abs().max()):.2e} of 1")
    assert l7[-1] <= 1.02 * l6[-1]


# ------------------------------------------------------------------------------------------------ host pose rewrite
def _poses(n, seed):
    g = np.random.default_rng(seed)
    p = g.standard_normal((n, 7)).astype(np.float32)
    p[:, 3:] /= np.linalg.norm(p[:, 3:], axis=1, keepdims=True)
    return gh.pose_vec_to_matrix(p)


@pytest.mark.parametrize("s", [1.0, 0.8, 1.25])
def test_similarity_on_poses_is_rigid_with_the_scaled_centre(s):
    n = 11
    c2w = _poses(n, 1)
    xi = _rand_xi(n, 8)
    xi[:, 6] = math.log(s)
    Sm = Q.matrix7(xi)[:, :3, :].numpy()
    out, sc = gh.similarity_on_poses(Sm.astype(np.float32), c2w)
    assert out.dtype == np.float32 and out.shape == (n, 4, 4)
    np.testing.assert_allclose(sc, s, rtol=1e-6)
    R = out[:, :3, :3].astype(np.float64)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-6 and np.abs(np.linalg.det(R) - 1).max() < 1e-6
    centre = np.einsum("nij,nj->ni", Sm[:, :, :3], c2w[:, :3, 3].astype(np.float64)) + Sm[:, :, 3]
    np.testing.assert_allclose(out[:, :3, 3], centre, rtol=0, atol=4 * 2.0 ** -24 * (np.abs(centre).max() + 1))
    np.testing.assert_allclose(R, (Sm[:, :, :3] / s) @ c2w[:, :3, :3], atol=1e-6)
    assert np.array_equal(out[:, 3], np.tile(np.array([0, 0, 0, 1], np.float32), (n, 1)))
    if s == 1.0:
        # what TrackBackend._rewrite computes in se(3) mode: the fp32 product Ts @ c2w
        Ts = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
        Ts[:, :3, :] = Sm.astype(np.float32)
        old = np.stack([Ts[j] @ c2w[j] for j in range(n)])
        bound = 8 * 2.0 ** -24 * (np.abs(Ts) @ np.abs(c2w)).max()
        assert np.abs(out - old).max() <= bound
    one, s1 = gh.similarity_on_poses(Sm.astype(np.float32)[0], c2w)       # one similarity for all
    assert np.allclose(s1, s) and np.array_equal(one[0], out[0])
