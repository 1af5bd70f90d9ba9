"""TEST INFRASTRUCTURE ONLY -- fp64 restatement of ONE iteration of the fused loop-closure optimiser over sim(3) (csrc/lc.hip:
lc_adam_kernel<2> / lc_terms_adam_kernel<2> behind cut3r_lc_optimize_sim3 / cut3r_lc_optimize_terms_sim3), the seeded inputs the per-element
tests run on, and the fp64 restatement of whole closures in that mode.  Plain torch on the CPU; no import of the extension.  This mode has
no counterpart in the reference: the restatement here is its only oracle.

The accumulate and gather stages are those of tests/lc_step_oracle.py (imported: they take any 3x4 T).  What differs is the pull-back:
  xi = [tau(3), phi(3), sigma],  T = matrix(exp(xi)) = [e^sigma R | W tau] = the top three rows of torch.matrix_exp of the 4x4 generator
  [[sigma I + [phi]x, tau], [0, 0]]  (Sophus / lietorch Sim3.exp);  g = fp64 autograd through it;  Adam as in lc_step_oracle.adam_step."""
import functools
import math

import torch

from oracle import lc_oracle as LO
from tests import lc_step_oracle as S

B1, B2, EPS, LR = S.B1, S.B2, S.EPS, S.LR
F64 = torch.float64


def twist7(xi):
    """[P,7] -> [P,4,4]: [[sigma I + [phi]x, tau], [0, 0]]"""
    M = LO.twist(xi[:, :6])
    D = torch.zeros(4, 4, dtype=xi.dtype)
    D[0, 0] = D[1, 1] = D[2, 2] = 1
    return M + xi[:, 6, None, None] * D


def matrix7(xi):
    return torch.matrix_exp(twist7(xi))


def adam_step7(G, xi, m, v, step, lr=LR, dtype=F64):
    """G [P,12] (or [P,3,4]); xi, m, v [P,7]; step counted from 0.  Returns (xi', m', v', T' [P,3,4], g [P,7]); row 0 of xi, m, v is returned
    as given."""
    xi, m, v = xi.to(dtype), m.to(dtype), v.to(dtype)
    x = xi.clone().requires_grad_(True)
    M = matrix7(x)[:, :3, :]
    (M * G.reshape(-1, 3, 4).to(dtype)).sum().backward()
    g = x.grad.clone()
    g[0] = 0
    m1 = B1 * m + (1 - B1) * g
    v1 = B2 * v + (1 - B2) * g * g
    bc1, bc2 = 1 - B1 ** (step + 1), 1 - B2 ** (step + 1)
    x1 = xi - (lr / bc1) * m1 / (v1.sqrt() / math.sqrt(bc2) + EPS)
    x1[0], m1[0], v1[0] = xi[0], m[0], v[0]
    T1 = matrix7(x1)[:, :3, :]
    return x1, m1, v1, T1, g


def iterate(terms, P, N, xi, m, v, T, k, lr=LR, dtype=F64):
    """lc_step_oracle.iterate with the sim(3) step"""
    hist, sign0 = [], None
    T = T.reshape(-1, 3, 4).to(dtype)
    for it in range(k):
        R = S.accum_rows(terms, T, N, dtype)
        if sign0 is None:
            sign0 = R.signs
        same = all(torch.equal(a, b) for a, b in zip(R.signs, sign0))
        xi, m, v, T, g = adam_step7(S.gather(R.rows, terms, P), xi, m, v, it, lr, dtype)
        hist.append(dict(R=R, loss=R.rows[:, :, 24].sum(), min_r=R.min_r, same_signs=same, g=g, xi=xi, m=m, v=v, T=T))
    return hist


# ------------------------------------------------------------------------------------------------ seeded inputs
PHI = (0.0, 1e-4, 0.29, 0.31, 1.0, 2.5)
TAU = (0.0, 1.0)
SIGMA = (0.0, 1e-4, 0.05, -0.05, 0.29, -0.29, 0.31, -0.31, 0.7, 0.1)      # 0.1: with |phi| = 0.29 just past theta^2 + sigma^2 = 0.09
# (|phi|, |tau|, sigma) of a row.  Rows 0..9 hold every value of PHI, TAU and SIGMA; liemath::sim3_coeffs switches its C at sigma^2 = 0.09
# (rows 2 | 3, 5 | 6 on either side) and its A, B at theta^2 + sigma^2 = 0.09 (rows 0 | 1 through sigma, 11 | 10 through theta).
ROWS = [
    (0.29, 1.0, 0.05), (0.29, 0.0, 0.1), (0.0, 1.0, 0.29), (1e-4, 1.0, 0.31), (0.31, 0.0, -0.05),
    (1.0, 1.0, -0.29), (2.5, 1.0, -0.31), (0.0, 0.0, 0.7), (1e-4, 0.0, 1e-4), (1.0, 1.0, 0.0),
    (0.31, 1.0, 0.0), (0.29, 1.0, 0.0), (2.5, 0.0, 0.7), (1.0, 0.0, -0.31), (0.0, 1.0, -0.05), (1e-4, 1.0, 0.05),
]
ZERO = -1                                       # row id of the zero vector (three-step cases)
MARGIN_1, MARGIN_3 = S.MARGIN_1, S.MARGIN_3


def _partner(a, Ta, Tc, margin, N, g):
    """c = Tc^-1 (Ta a + e) in fp64, rounded; |e_k| uniform in [margin, 4 margin], random sign (Tc a similarity: a general inverse)"""
    e = (margin * (1 + 3 * torch.rand(N, 3, generator=g, dtype=F64)) * (torch.randint(0, 2, (N, 3), generator=g).double() * 2 - 1))
    y = a.double() @ Ta[:3, :3].T + Ta[:3, 3] + e
    return ((y - Tc[:3, 3]) @ torch.inverse(Tc[:3, :3]).T).float()


def make_case(name, kind, N, P, rows, spec=None, iters=1, seed=0, mask="rand"):
    """as lc_step_oracle.make_case, with xi [P,7] drawn from ROWS (no residual is planted at exactly 0: sign(0) belongs to the accumulate
    kernels, which the se(3) file covers)"""
    g = torch.Generator().manual_seed(seed)
    cs = S.Case()
    cs.name, cs.kind, cs.N, cs.P, cs.iters, cs.rows = name, kind, N, P, iters, list(rows)
    cs.margin = MARGIN_1 if iters == 1 else MARGIN_3
    assert len(rows) == P - 1
    xi = torch.zeros(P, 7, dtype=F64)
    for b, rid in enumerate(rows, 1):
        if rid == ZERO:
            continue
        phi_n, tau_n, sig = ROWS[rid]
        xi[b, :3], xi[b, 3:6], xi[b, 6] = tau_n * S._unit(g), phi_n * S._unit(g), sig
    if iters > 1:
        assert not xi.any(), "multi-step cases start from the zero state"
    cs.xi = xi.float()
    T64 = matrix7(cs.xi.double())
    for b in range(P):
        if not bool(cs.xi[b].any()):
            T64[b] = torch.eye(4, dtype=F64)
    cs.T = T64[:, :3, :].float().reshape(P, 12).contiguous()
    cs.planted = 0

    def rand_mask():
        return (torch.rand(N, generator=g) > 0.1).to(torch.uint8)

    if kind == "chain":
        B = P
        sub = torch.stack([torch.stack([S._points(N, g) for _ in range(6)]) for _ in range(B)])
        cs.mask = torch.stack([rand_mask() for _ in range(B - 1)]) if mask == "rand" else None
        for p in range(B - 1):
            sub[p + 1, 0] = _partner(sub[p, 5], T64[p], T64[p + 1], cs.margin, N, g)
        cs.sub = sub.contiguous()
        cs.cur = S._points(N, g)
        cs.cur_lc = _partner(cs.cur, T64[B - 1], torch.eye(4, dtype=F64), cs.margin, N, g)
        cs.terms, cs.n_masked = S.chain_terms(cs.sub[:, 0], cs.sub[:, 5], cs.mask, cs.cur, cs.cur_lc)
    else:
        cs.terms = []
        for ia, ic, masked in spec:
            a = S._points(N, g)
            c = _partner(a, T64[ia], T64[ic], cs.margin, N, g)
            mk = rand_mask() if masked else None
            n_set = N if mk is None else int(mk.sum())
            w = float(torch.tensor(1.0 / (3.0 * len(spec) * max(n_set, 1))).float())
            cs.terms.append((a, ia, c, ic, w, mk))
    cs.m0, cs.v0 = torch.zeros(P, 7), torch.zeros(P, 7)
    if iters == 1:
        g64 = oracle_run(cs, zero_state=True)[0]["g"]
        mag = torch.maximum(g64.abs(), 0.05 * g64.abs().max().clamp_min(1e-3)).expand(P, 7)
        cs.m0 = (mag * (0.5 + torch.rand(P, 7, generator=g).double()) * (torch.randint(0, 2, (P, 7), generator=g).double() * 2 - 1)).float()
        cs.v0 = ((mag * (0.5 + torch.rand(P, 7, generator=g).double())) ** 2).float()
    return cs


def oracle_run(cs, dtype=F64, zero_state=False, terms=None):
    z = torch.zeros(cs.P, 7)
    m, v = (z, z) if zero_state else (cs.m0, cs.v0)
    return iterate(cs.terms if terms is None else terms, cs.P, cs.N, cs.xi, m, v, cs.T, cs.iters, LR, dtype)


_LATER = S._LATER                                                                                        # B = 4, Bc = 2, P = 6, 7 terms
_SAME = [(1, 1, False), (1, 2, False), (0, 0, False), (2, 0, True), (3, 3, False), (4, 5, True), (5, 3, False)]
CASE_TABLE = [
    ("chain-N1-B2", "chain", 1, 2, [0], None, 1, None),
    ("chain-N63-B3", "chain", 63, 3, [1, 2], None, 1, "rand"),
    ("chain-N64-B5", "chain", 64, 5, [3, 4, 5, 6], None, 1, "rand"),
    ("chain-N2047-B2", "chain", 2047, 2, [7], None, 1, "rand"),
    ("chain-N2048-B3", "chain", 2048, 3, [8, 9], None, 1, None),
    ("chain-N2049-B5", "chain", 2049, 5, [10, 11, 12, 13], None, 1, "rand"),
    ("chain-N16389-B3", "chain", 8 * 2048 + 5, 3, [14, 15], None, 1, "rand"),
    ("terms-later-loop", "terms", 2049, 6, [0, 1, 2, 3, 4], _LATER, 1, None),
    ("terms-same-index", "terms", 2047, 6, [5, 6, 7, 8, 9], _SAME, 1, None),
    ("chain3-N2049-B3", "chain", 2049, 3, [ZERO, ZERO], None, 3, "rand"),
    ("chain3-N16389-B2", "chain", 8 * 2048 + 5, 2, [ZERO], None, 3, None),
    ("terms3-later-loop", "terms", 2049, 6, [ZERO] * 5, _LATER, 3, None),
]
# seeds chosen so that the inputs meet test_lc_sim3_cpu.test_inputs_meet_their_conditions (no gradient component of a three-step case within
# 1e-3 of 0 relative to the largest: the first step from zero state normalises each to +-lr, and fp32 must see the same sign)
SEEDS = {"terms3-later-loop": 715}
CASE_NAMES = [c[0] for c in CASE_TABLE]
ONE_STEP = [c[0] for c in CASE_TABLE if c[6] == 1]
THREE_STEP = [c[0] for c in CASE_TABLE if c[6] == 3]


@functools.lru_cache(maxsize=None)
def get_case(name):
    i = CASE_NAMES.index(name)
    _, kind, N, P, rows, spec, iters, mask = CASE_TABLE[i]
    return make_case(name, kind, N, P, rows, spec, iters, seed=SEEDS.get(name, 700 + i), mask=mask)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the fp64 oracle's run of a case, computed once and shared (treat as read-only)"""
    return oracle_run(get_case(name))


@functools.lru_cache(maxsize=None)
def measure_margins():
    """fp32 restatement vs fp64 oracle over every one-step case, worst distance per quantity (lc_step_oracle.scaled_distance), and xi, T after
    the third step of every three-step case ('xi3', 'T3').  The GPU tests allow 4 x these."""
    worst = {}
    for name in ONE_STEP:
        cs = get_case(name)
        h32 = oracle_run(cs, torch.float32)[0]
        for k, d in S.scaled_distance(h32, reference(name)[0], cs.m0).items():
            worst[k] = max(worst.get(k, 0.0), d)
    for name in THREE_STEP:
        cs = get_case(name)
        h32, h64 = oracle_run(cs, torch.float32)[-1], reference(name)[-1]
        worst["xi3"] = max(worst.get("xi3", 0.0), float((h32["xi"].double() - h64["xi"]).abs().max()))
        worst["T3"] = max(worst.get("T3", 0.0), float((h32["T"].double() - h64["T"]).abs().max()))
    return worst


# ------------------------------------------------------------------------------------------------ whole optimisations, fp64
def _adam_terms(term_fn, shapes, iters, lr, dtype, K):
    """torch.optim.Adam over zero-initialised parameter blocks of width K; term_fn(params) -> loss"""
    ps = [torch.nn.Parameter(torch.zeros(n, K, dtype=dtype)) for n in shapes]
    opt = torch.optim.Adam([{"params": p, "lr": lr} for p in ps])
    losses = []
    for _ in range(iters):
        opt.zero_grad()
        loss = term_fn(ps)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return [p.detach() for p in ps], losses


def _mat(xi, K):
    return matrix7(xi) if K == 7 else torch.matrix_exp(LO.twist(xi))


def _apply(T, p):
    """T [...,4,4] on p [...,N,3]"""
    return p @ T[..., :3, :3].transpose(-1, -2) + T[..., None, :3, 3]


def loop_closure_init(submaps, mask, cur, cur_lc, iters, lr=LR, dtype=F64, K=7):
    """oracle/lc_oracle.loop_closure_init's objective over K = 7 (sim(3)) or K = 6 (se(3): the same numbers as the original) parameters
    per submap.  Returns (xi [B,K], T [B,4,4], losses)."""
    sub = submaps.to(dtype)
    B = sub.shape[0]
    first, last = sub[:, 0].reshape(B, -1, 3), sub[:, -1].reshape(B, -1, 3)
    cur, cur_lc = cur.to(dtype).reshape(-1, 3), cur_lc.to(dtype).reshape(-1, 3)
    z = torch.zeros(1, K, dtype=dtype)

    def loss_fn(ps):
        T = _mat(torch.cat([z, ps[0]], 0), K)
        l_cur = (_apply(T[-1], cur) - cur_lc).abs().mean()
        return (_apply(T[:-1], last[:-1]) - _apply(T[1:], first[1:]))[mask].abs().mean() + l_cur

    (p,), losses = _adam_terms(loss_fn, [B - 1], iters, lr, dtype, K)
    xi = torch.cat([z, p], 0)
    return xi, _mat(xi, K), losses


def loop_closure(submaps, lc_all, pm_cur, sub_cur_all, sub_matched_all, iters, lr=LR, dtype=F64, K=7):
    """oracle/lc_oracle.loop_closure's objective over K parameters per transform.  Returns (xi [B,K], T, xi_m [Bc,K], Tm, losses)."""
    sub, lc, cur = submaps.to(dtype), lc_all.to(dtype), pm_cur.to(dtype)
    B, Bc = sub.shape[0], lc.shape[0]
    first, last = sub[:, 0].reshape(B, -1, 3), sub[:, -1].reshape(B, -1, 3)
    lc_first, lc_last = lc[:, 0].reshape(Bc, -1, 3), lc[:, -1].reshape(Bc, -1, 3)
    cur = cur.reshape(Bc, -1, 3)
    sc, sm = torch.as_tensor(sub_cur_all, dtype=torch.long), torch.as_tensor(sub_matched_all, dtype=torch.long)
    z = torch.zeros(1, K, dtype=dtype)

    def loss_fn(ps):
        T, Tm = _mat(torch.cat([z, ps[0]], 0), K), _mat(ps[1], K)
        fl_loss = (_apply(T[:-1], last[:-1]) - _apply(T[1:], first[1:])).abs().mean()
        matched = (_apply(Tm, lc_first) - _apply(T[sm], first[sm])).abs().mean()
        current = (_apply(T[sc], cur) - _apply(Tm, lc_last)).abs().mean()
        return fl_loss + current + matched

    (a, mm), losses = _adam_terms(loss_fn, [B - 1, Bc], iters, lr, dtype, K)
    xi = torch.cat([z, a], 0)
    return xi, _mat(xi, K), mm, _mat(mm, K), losses


def scale_of(T):
    """cube root of det of the 3x3 block, fp64"""
    d = torch.linalg.det(T[..., :3, :3].double())
    return d.sign() * d.abs() ** (1.0 / 3.0)


class LoopCloserSim3(LO.LoopCloser):
    """oracle/lc_oracle.LoopCloser in sim(3) mode: the optimisers above with K = 7; the rewrite moves the pointmaps by the similarity, keeps
    the poses rigid (rotation R R0, centre s R c + t) and multiplies the depth map of every rewritten keyframe by its submap's scale.
    `depth` [K,H,W] is updated in place like the other stores."""

    def __init__(self, submaps, conf_ds, pose, depth, iters, dtype=F64):
        super().__init__(submaps, conf_ds, pose, iters, dtype)
        self.depth = depth.double()

    def _rewrite(self, sub1, T):
        from scipy.spatial.transform import Rotation
        B = sub1 + 1
        self.sub[:B] = torch.einsum("bij,bshwj->bshwi", T[:, :3, :3], self.sub[:B]) + T[:, :3, 3].reshape(B, 1, 1, 1, 3)
        s = scale_of(T)
        for i in range(B * 5 + 1):
            b = min(i // 5, B - 1)
            P0 = self._pose_mat(self.pose[i])
            Rn = (T[b, :3, :3] / s[b]) @ P0[:3, :3]
            c = T[b, :3, :3] @ P0[:3, 3] + T[b, :3, 3]
            self.pose[i] = torch.cat([c, torch.from_numpy(Rotation.from_matrix(Rn.numpy()).as_quat())])
            self.depth[i] = self.depth[i] * s[b]

    def close(self, pm_lc, idx_matched, idx_current):
        sub1 = idx_current // 5
        pm_lc = pm_lc.double()
        if not self.initialized:
            B = sub1 + 1
            mask = (self.conf[:sub1, 5] > 0).reshape(B - 1, -1)
            cur = self.sub[sub1, idx_current % 5].reshape(-1, 3)
            xi, T, losses = loop_closure_init(self.sub[:B], mask, cur, pm_lc[-1].reshape(-1, 3), self.iters, dtype=self.dtype)
            T = T.double()
            self._rewrite(sub1, T)
            self.initialized = True
            stored = pm_lc
        else:
            prev_cur = self.closed["idx_current"]
            lc_all = torch.stack(self.closed["pointmaps_lc"] + [pm_lc], 0)
            pm_cur = torch.stack([self.sub[c // 5, c % 5] for c in prev_cur] + [self.sub[sub1, idx_current % 5]], 0)
            sc = [c // 5 for c in prev_cur] + [sub1]
            sm = [m // 5 for m in self.closed["idx_matched"]] + [idx_matched // 5]
            xi, T, xi_m, Tm, losses = loop_closure(self.sub[:sub1 + 1], lc_all, pm_cur, sc, sm, self.iters, dtype=self.dtype)
            T, Tm = T.double(), Tm.double()
            self._rewrite(sub1, T)
            lc_al = torch.einsum("kij,kshwj->kshwi", Tm[:, :3, :3], lc_all) + Tm[:, :3, 3].reshape(-1, 1, 1, 1, 3)
            for i in range(len(prev_cur)):
                self.closed["pointmaps_lc"][i] = lc_al[i]
            stored = lc_al[-1]
        self.closed["idx_current"].append(idx_current)
        self.closed["idx_matched"].append(idx_matched)
        self.closed["pointmaps_lc"].append(stored)
        self.losses.append(losses)
        self.T_last = T
        return xi


# ------------------------------------------------------------------------------------------------ the scale-drift scenario
def drift_scenario(B=5, N=257, noise=5e-3, total_scale=1.1, seed=0):
    """A chain of B submaps over a closed loop whose stored frames carry a cumulative similarity drift A_p (per-step log-scale
    log(total_scale) / (B - 1), small rotation / translation growing with p; A_0 = identity):  first_p = A_p(bound_p), last_p =
    A_p(bound_{p+1}), both + noise;  cur = last_{B-1},  cur_lc = bound_B + noise (the loop's far end seen without drift).  The similarity
    that undoes the drift of submap p is A_p^-1: scale 1 / scale(A_p).  Returns (submaps [B,6,1,N,3], mask, cur, cur_lc, scales of A_p)."""
    g = torch.Generator().manual_seed(seed)
    bound = [torch.randn(N, 3, generator=g, dtype=F64) * 1.5 + torch.tensor([0.0, 0.0, 3.0], dtype=F64) for _ in range(B + 1)]
    xi = torch.zeros(B, 7, dtype=F64)
    for p in range(1, B):
        xi[p, :3] = 0.02 * p * S._unit(g)
        xi[p, 3:6] = 0.01 * p * S._unit(g)
        xi[p, 6] = math.log(total_scale) * p / (B - 1)
    A = matrix7(xi)
    n = lambda: noise * torch.randn(N, 3, generator=g, dtype=F64)
    sub = torch.randn(B, 6, 1, N, 3, generator=g, dtype=F64)
    for p in range(B):
        sub[p, 0, 0] = _apply(A[p], bound[p]) + n()
        sub[p, 5, 0] = _apply(A[p], bound[p + 1]) + n()
    cur = sub[B - 1, 5, 0].clone()
    cur_lc = bound[B] + n()
    mask = torch.ones(B - 1, N, dtype=torch.bool)
    return sub.float(), mask, cur.float(), cur_lc.float(), scale_of(A)
