"""TEST INFRASTRUCTURE ONLY -- fp64 restatement of ONE iteration of the fused loop-closure optimiser (csrc/lc.hip: lc_accum / lc_adam and
their term-list forms), element for element, plus the seeded inputs the per-element tests run on.  Plain torch on the CPU; no import of
the extension.

One iteration, as lc.hip and include/cut3r_hip.h document it:
  accumulate : for every term  w * sum_n | T[ia] a_n - T[ic] c_n |_1  and every block of LC_POINTS = 2048 consecutive points, one row of
               25 numbers: the 12 sums of sign(r) [a;1] (gradient to the 3x4 matrix T[ia], row-major), the 12 sums of -sign(r) [c;1]
               (to T[ic]; zero where c is fixed, the `cur` pair of the chain form), and sum |r|; each times w.  Masked-out points add
               nothing, sign(0) = 0.
  gather     : G[b] = sum, over the terms that use transform b, of the 'a' (and / or 'c') halves of their rows.  Row 0 is the fixed identity.
  adam       : g = pull-back of G through matrix(exp(xi)) (here: fp64 autograd through torch.matrix_exp of the twist), then
               torch.optim.Adam:  m' = b1 m + (1-b1) g,  v' = b2 v + (1-b2) g^2,  xi' = xi - lr/(1-b1^t) m' / (sqrt(v')/sqrt(1-b2^t) + eps),
               t = step + 1 with `step` counted from 0 in every call;  T' = matrix(exp(xi')).

Every function takes `dtype`: float64 is the oracle, float32 is the same statement in the arithmetic of the kernels (summed in torch's order),
used only to MEASURE how far two correct fp32 evaluations may sit from the fp64 one (measure_margins)."""
import functools
import math
from typing import NamedTuple

import torch
import torch.nn.functional as F

from oracle.lc_oracle import twist

LC_POINTS = 2048                 # LC_BLOCK * LC_PPT: points per workspace row
LC_ROW = 28                      # floats per workspace row (25 used)
B1, B2, EPS = 0.9, 0.999, 1e-8   # torch.optim.Adam defaults, as the kernels hard-code them
LR = 5e-4
U = 2.0 ** -24                   # fp32 unit roundoff


def nblk(N):
    return (N + LC_POINTS - 1) // LC_POINTS


class Rows(NamedTuple):
    rows: torch.Tensor           # [terms, nblk, 25]
    abssum: torch.Tensor         # [terms, nblk, 25]  sum of |what was added| per entry (times |w|)
    rmag: torch.Tensor           # [terms, nblk]      w * sum over points and coordinates of |T[ia]| |[a;1]| + |T[ic]| |[c;1]|
    min_r: float                 # smallest non-zero |r| over unmasked points and coordinates
    n_zero: int                  # number of unmasked coordinates whose residual is exactly 0
    signs: list                  # per term int8 [N,3]: sign(r), 0 where masked out


def chain_terms(first, last, mask, cur, cur_lc):
    """The chain form as a term list.  first/last [B,N,3], mask [B-1,N] (any non-zero byte = set) or None, cur/cur_lc [N,3].
    A term is (a, ia, c, ic, w, mask); ic = None marks a fixed c (no transform, no gradient).  Returns (terms, n_masked)."""
    B, N = first.shape[0], first.shape[1]
    n_masked = (B - 1) * N if mask is None else int((mask != 0).sum())
    w_fl = 1.0 / (3.0 * n_masked) if n_masked > 0 else 0.0
    terms = [(last[p], p, first[p + 1], p + 1, w_fl, None if mask is None else mask[p]) for p in range(B - 1)]
    terms.append((cur, B - 1, cur_lc, None, 1.0 / (3.0 * N), None))
    return terms, n_masked


def accum_rows(terms, T, N, dtype=torch.float64):
    T = T.reshape(-1, 3, 4).to(dtype)
    nb = nblk(N)
    pad = nb * LC_POINTS - N
    blk = lambda x: F.pad(x, (0, 0, 0, pad)).reshape(nb, LC_POINTS, -1)
    one = torch.ones(N, 1, dtype=dtype)
    rows, abss, rmag, signs = [], [], [], []
    min_r, n_zero = math.inf, 0
    for a, ia, c, ic, w, mask in terms:
        a, c = a.reshape(N, 3).to(dtype), c.reshape(N, 3).to(dtype)
        a1, c1 = torch.cat([a, one], 1), torch.cat([c, one], 1)
        cp = c if ic is None else c1 @ T[ic].T
        r = a1 @ T[ia].T - cp
        s = torch.sign(r)
        keep = torch.ones(N, dtype=torch.bool) if mask is None else mask.reshape(N) != 0
        ta = (s[:, :, None] * a1[:, None, :]).reshape(N, 12)
        tc = torch.zeros(N, 12, dtype=dtype) if ic is None else (-s[:, :, None] * c1[:, None, :]).reshape(N, 12)
        t = torch.cat([ta, tc, r.abs().sum(1, keepdim=True)], 1) * keep[:, None].to(dtype) * w
        mag = (a1.abs() @ T[ia].abs().T).sum(1) + (c.abs().sum(1) if ic is None else (c1.abs() @ T[ic].abs().T).sum(1))
        rows.append(blk(t).sum(1))
        abss.append(blk(t.abs()).sum(1))
        rmag.append(blk((mag * keep.to(dtype) * abs(w))[:, None]).sum(1)[:, 0])
        rk = r.abs()[keep]
        n_zero += int((rk == 0).sum())
        if (rk > 0).any():
            min_r = min(min_r, float(rk[rk > 0].min()))
        signs.append((s * keep[:, None].to(dtype)).to(torch.int8))
    return Rows(torch.stack(rows), torch.stack(abss), torch.stack(rmag), min_r, n_zero, signs)


def gather(rows, terms, P):
    """G [P,12]: per transform the sum of the row halves of the terms that reference it, in term order; row 0 (fixed) stays 0"""
    G = torch.zeros(P, 12, dtype=rows.dtype)
    for t, (_, ia, _, ic, _, _) in enumerate(terms):
        if ia > 0:
            G[ia] += rows[t, :, 0:12].sum(0)
        if ic is not None and ic > 0:
            G[ic] += rows[t, :, 12:24].sum(0)
    return G


def adam_step(G, xi, m, v, step, lr=LR, dtype=torch.float64):
    """G [P,12] (or [P,3,4]); xi, m, v [P,6]; step counted from 0.  Returns (xi', m', v', T' [P,3,4], g [P,6]); row 0 of xi, m, v is
    returned as given."""
    xi, m, v = xi.to(dtype), m.to(dtype), v.to(dtype)
    x = xi.clone().requires_grad_(True)
    M = torch.matrix_exp(twist(x))[:, :3, :]
    (M * G.reshape(-1, 3, 4).to(dtype)).sum().backward()
    g = x.grad.clone()
    g[0] = 0
    m1 = B1 * m + (1 - B1) * g
    v1 = B2 * v + (1 - B2) * g * g
    bc1, bc2 = 1 - B1 ** (step + 1), 1 - B2 ** (step + 1)
    x1 = xi - (lr / bc1) * m1 / (v1.sqrt() / math.sqrt(bc2) + EPS)
    x1[0], m1[0], v1[0] = xi[0], m[0], v[0]
    T1 = torch.matrix_exp(twist(x1))[:, :3, :]
    return x1, m1, v1, T1, g


def iterate(terms, P, N, xi, m, v, T, k, lr=LR, dtype=torch.float64):
    """k iterations in sequence from the caller's state (T is used as given for the first one).  Returns one dict per iteration: the rows at
    the iteration's T, its loss and minimum |r|, whether every sign equals iteration 0's, g, and the state after the step."""
    hist, sign0 = [], None
    T = T.reshape(-1, 3, 4).to(dtype)
    for it in range(k):
        R = accum_rows(terms, T, N, dtype)
        if sign0 is None:
            sign0 = R.signs
        same = all(torch.equal(a, b) for a, b in zip(R.signs, sign0))
        xi, m, v, T, g = adam_step(gather(R.rows, terms, P), xi, m, v, it, lr, dtype)
        hist.append(dict(R=R, loss=R.rows[:, :, 24].sum(), min_r=R.min_r, same_signs=same, g=g, xi=xi, m=m, v=v, T=T))
    return hist


# ------------------------------------------------------------------------------------------------ seeded inputs
PHI = (0.0, 1e-4, 0.29, 0.31, 1.0, 2.5)        # crosses liemath's SERIES_X2 = 0.09 (|phi| = 0.3) and so3_exp's EPS
TAU = (0.0, 1.0)
COMBOS = [(p, t) for p in PHI for t in TAU]    # id = 2 * index(phi) + index(tau); id 0 is the identity
MARGIN_1, MARGIN_3 = 1e-3, 5e-2
ZERO_IDX = range(2, 40, 3)                      # points that get e = 0 where both transforms of a term are the identity


class Case:
    """name, kind ('chain' | 'terms'), N, P, iters, margin, combos (one id per optimised row), xi [P,6] / T [P,12] fp32 with
    T = matrix(exp(xi)) rounded, terms (fp32 operands; oracle form), planted (coordinates planted at exactly 0), m0 / v0 [P,6] fp32.
    chain only: sub [B,6,N,3], mask uint8 [B-1,N] | None, cur, cur_lc, n_masked."""


def _unit(g):
    x = torch.randn(3, generator=g, dtype=torch.float64)
    return x / x.norm()


def _points(N, g):
    return (torch.randn(N, 3, generator=g, dtype=torch.float64) * 1.5 + torch.tensor([0.0, 0.0, 3.0], dtype=torch.float64)).float()


def _partner(a, Ta, Tc, ident, margin, N, g):
    """c = Tc^-1 (Ta a + e) in fp64, rounded; |e_k| uniform in [margin, 4 margin], random sign; e = 0 at ZERO_IDX iff `ident`.
    Returns (c fp32, number of planted points)"""
    e = (margin * (1 + 3 * torch.rand(N, 3, generator=g, dtype=torch.float64))
         * (torch.randint(0, 2, (N, 3), generator=g).double() * 2 - 1))
    a = a.double()
    idx = [i for i in ZERO_IDX if i < N] if ident else []
    if ident:
        e[idx] = 0
        return (a + e).float(), idx
    y = a @ Ta[:3, :3].T + Ta[:3, 3] + e
    return ((y - Tc[:3, 3]) @ Tc[:3, :3]).float(), idx


def make_case(name, kind, N, P, combos, spec=None, iters=1, seed=0, mask="rand"):
    """spec (terms form): list of (ia, ic, masked).  chain form: P = B, pairs (p, p+1) and the cur pair; mask 'rand' (90 % set) or None."""
    g = torch.Generator().manual_seed(seed)
    cs = Case()
    cs.name, cs.kind, cs.N, cs.P, cs.iters, cs.combos = name, kind, N, P, iters, list(combos)
    cs.margin = MARGIN_1 if iters == 1 else MARGIN_3
    assert len(combos) == P - 1
    xi = torch.zeros(P, 6, dtype=torch.float64)
    for b, cid in enumerate(combos, 1):
        phi_n, tau_n = COMBOS[cid]
        xi[b, :3], xi[b, 3:] = tau_n * _unit(g), phi_n * _unit(g)
    if iters > 1:
        assert not xi.any(), "multi-step cases start from the zero state"
    cs.xi = xi.float()
    T64 = torch.matrix_exp(twist(cs.xi.double()))
    is_id = [not bool(cs.xi[b].any()) for b in range(P)]
    for b in range(P):
        if is_id[b]:
            T64[b] = torch.eye(4, dtype=torch.float64)
    cs.T = T64[:, :3, :].float().reshape(P, 12).contiguous()
    plant = iters == 1                                   # a planted zero would change sign at the first step
    cs.planted = 0

    def rand_mask():
        return (torch.rand(N, generator=g) > 0.1).to(torch.uint8)

    if kind == "chain":
        B = P
        sub = torch.stack([torch.stack([_points(N, g) for _ in range(6)]) for _ in range(B)])          # [B,6,N,3]
        cs.mask = torch.stack([rand_mask() for _ in range(B - 1)]) if mask == "rand" else None
        for p in range(B - 1):
            c, idx = _partner(sub[p, 5], T64[p], T64[p + 1], plant and is_id[p] and is_id[p + 1], cs.margin, N, g)
            sub[p + 1, 0] = c
            cs.planted += 3 * sum(1 for i in idx if cs.mask is None or cs.mask[p, i])
        cs.sub = sub.contiguous()
        cs.cur = _points(N, g)
        cs.cur_lc, idx = _partner(cs.cur, T64[B - 1], torch.eye(4, dtype=torch.float64), plant and is_id[B - 1], cs.margin, N, g)
        cs.planted += 3 * len(idx)
        cs.terms, cs.n_masked = chain_terms(cs.sub[:, 0], cs.sub[:, 5], cs.mask, cs.cur, cs.cur_lc)
    else:
        cs.terms = []
        for ia, ic, masked in spec:
            a = _points(N, g)
            c, idx = _partner(a, T64[ia], T64[ic], plant and is_id[ia] and is_id[ic], cs.margin, N, g)
            mk = rand_mask() if masked else None
            n_set = N if mk is None else int(mk.sum())
            w = float(torch.tensor(1.0 / (3.0 * len(spec) * max(n_set, 1))).float())                   # the weight is an fp32 input
            cs.terms.append((a, ia, c, ic, w, mk))
            cs.planted += 3 * sum(1 for i in idx if mk is None or mk[i])
    # seeded Adam state: |m| and sqrt(v) around the oracle's |g| for the one-step cases, zero for the multi-step ones
    cs.m0, cs.v0 = torch.zeros(P, 6), torch.zeros(P, 6)
    if iters == 1:
        g64 = oracle_run(cs, zero_state=True)[0]["g"]
        mag = torch.maximum(g64.abs(), 0.05 * g64.abs().max().clamp_min(1e-3)).expand(P, 6)
        cs.m0 = (mag * (0.5 + torch.rand(P, 6, generator=g).double()) * (torch.randint(0, 2, (P, 6), generator=g).double() * 2 - 1)).float()
        cs.v0 = ((mag * (0.5 + torch.rand(P, 6, generator=g).double())) ** 2).float()
    return cs


def oracle_run(cs, dtype=torch.float64, zero_state=False, terms=None):
    """the case's iterations from its own state (or from m = v = 0); `terms` overrides the term list (mask / layout variants)"""
    z = torch.zeros(cs.P, 6)
    m, v = (z, z) if zero_state else (cs.m0, cs.v0)
    return iterate(cs.terms if terms is None else terms, cs.P, cs.N, cs.xi, m, v, cs.T, cs.iters, LR, dtype)


# (name, kind, N, P, combo ids of rows 1..P-1, spec, iters, mask).  N: 1, one short of / exactly / one past a wave and a block, nblk = 9
# (one full eight-row gather group + a ragged one, ragged last block), nblk = 17 (two full groups + one).  Every combo id appears among the
# one-step chain cases and among the one-step term cases (test_lc_step_cpu checks it).
_LATER = [(0, 1, False), (1, 2, False), (2, 3, False), (4, 0, False), (5, 1, False), (2, 4, False), (3, 5, False)]      # B = 4, Bc = 2, P = 6
CASE_TABLE = [
    ("chain-N1-B2", "chain", 1, 2, [2], None, 1, None),
    ("chain-N63-B3", "chain", 63, 3, [3, 4], None, 1, "rand"),
    ("chain-N64-B5", "chain", 64, 5, [5, 6, 7, 8], None, 1, "rand"),
    ("chain-N2047-B2", "chain", 2047, 2, [9], None, 1, "rand"),
    ("chain-N2048-B3", "chain", 2048, 3, [10, 11], None, 1, None),
    ("chain-N2049-B5", "chain", 2049, 5, [0, 1, 2, 3], None, 1, "rand"),                  # row 1 = identity: pair 0 carries planted zeros
    ("chain-N16389-B3", "chain", 8 * 2048 + 5, 3, [4, 5], None, 1, "rand"),
    ("chain-N34816-B2", "chain", 17 * 2048, 2, [6], None, 1, "rand"),
    ("terms-later-loop", "terms", 2049, 6, [7, 8, 9, 10, 11], _LATER, 1, None),
    ("terms-same-index", "terms", 2047, 3, [0, 3], [(1, 1, False), (1, 2, False), (0, 0, False), (2, 0, True)], 1, None),
    ("terms-72-rows", "terms", 8 * 2048 + 5, 6, [1, 2, 4, 5, 6],                          # 8 terms x 9 blocks > 64 rows: the loss row's strided loop
     [(0, 1, False), (1, 2, True), (2, 3, False), (3, 4, False), (4, 5, True), (5, 0, False), (2, 2, False), (1, 3, False)], 1, None),
    ("chain3-N2049-B3", "chain", 2049, 3, [0, 0], None, 3, "rand"),
    ("chain3-N16389-B2", "chain", 8 * 2048 + 5, 2, [0], None, 3, None),
    ("terms3-later-loop", "terms", 2049, 6, [0, 0, 0, 0, 0], _LATER, 3, None),
]
CASE_NAMES = [c[0] for c in CASE_TABLE]
ONE_STEP = [c[0] for c in CASE_TABLE if c[6] == 1]
THREE_STEP = [c[0] for c in CASE_TABLE if c[6] == 3]


@functools.lru_cache(maxsize=None)
def get_case(name):
    i = CASE_NAMES.index(name)
    _, kind, N, P, combos, spec, iters, mask = CASE_TABLE[i]
    return make_case(name, kind, N, P, combos, spec, iters, seed=100 + i, mask=mask)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the fp64 oracle's run of a case, computed once and shared (treat as read-only)"""
    return oracle_run(get_case(name))


# ------------------------------------------------------------------------------------------------ measured margins
def scaled_distance(got, h64, m0):
    """{quantity: max |got - fp64|} of what the per-element tests compare after a step, in the units they compare it in: m', the g recovered
    from it as (m' - b1 m) / (1 - b1), and v' per unit of the fp64 run's max |g| (|g|^2 for v'); xi' and T' absolute"""
    gs = float(h64["g"].abs().max())

    def q(h):
        m1 = h["m"].double()
        return {"xi": h["xi"].double(), "T": h["T"].double().reshape(-1, 12), "m": m1 / gs, "v": h["v"].double() / gs ** 2,
                "g_from_m": (m1 - B1 * m0.double()) / (1 - B1) / gs}
    a, b = q(got), q(h64)
    return {k: float((a[k] - b[k]).abs().max()) for k in b}


@functools.lru_cache(maxsize=None)
def measure_margins():
    """fp32 restatement vs fp64 oracle over every one-step case, worst distance per quantity; and the same for xi, T after the third step
    of every three-step case ('xi3', 'T3').  The GPU tests allow 4 x these (the kernels sum in another order than torch does)."""
    worst = {}
    for name in ONE_STEP:
        cs = get_case(name)
        h32 = oracle_run(cs, torch.float32)[0]
        for k, d in scaled_distance(h32, reference(name)[0], cs.m0).items():
            worst[k] = max(worst.get(k, 0.0), d)
    for name in THREE_STEP:
        cs = get_case(name)
        h32, h64 = oracle_run(cs, torch.float32)[-1], reference(name)[-1]
        worst["xi3"] = max(worst.get("xi3", 0.0), float((h32["xi"].double() - h64["xi"]).abs().max()))
        worst["T3"] = max(worst.get("T3", 0.0), float((h32["T"].double() - h64["T"]).abs().max()))
    return worst
