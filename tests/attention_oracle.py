"""CPU oracle of the fused attention kernels (cut3r_slam_amd/csrc/attention.hip): an fp64 reference with a derived
per-element bound, inputs that make every key count, an emulation of the kernels' arithmetic that can be broken on purpose,
and the matrix of kernel instances and shapes that tests/test_attention_gpu.py runs.  torch and numpy only, no GPU.

The bound.  out[r, d] = sum_j p_j v[j, d] with p = softmax(scale * q k^T).  The kernels compute the scores and the row
sum in fp32, round each p_j (relative to the running maximum, so p_j <= 1) to fp16 for the PV product, accumulate that
product in fp32 and round the quotient to fp16.  With A[r, d] = sum_j p_j |v[j, d]| (>= |out[r, d]|):

  * fp16 rounding of P:       each p_j moves by at most 2^-11 p_j, the row sum uses the unrounded p  -> 2^-11 A
  * fp16 rounding of out:     2^-11 |out| <= 2^-11 A; below the normal range half a subnormal step    -> 2^-11 A + 2^-25
  * everything in fp32:       a score s = scale_log2 * (q . k) carries a few 2^-24 |s| of rounding (fp32 accumulation of
    exact fp16 products, one fma), the hardware exp2 is good to about 1 ulp, and p_j moves by ln2 * ds * p_j: with
    |s| <= 40 nats (58 in log2 units) that is ~3 * 58 * 0.69 * 2^-24 = 2^-17.1 p_j, the fp32 sums of at most a few hundred
    terms add 2^-16 at worst.  Together well under one unit of 2^-11 A; one unit is allowed                   -> 2^-11 A

so |kernel - reference| <= 3 * 2^-11 * A + 2^-24 element by element, on the condition |scaled score| <= 40.  The 3 is this
sum of terms, not a fit: `emulate` (the same arithmetic in torch) stays below 1.6 units on the inputs of `make_inputs`.
"""
import functools
import math

import torch

KT = 64                                   # keys per tile of both kernels
UNIT = 2.0 ** -11
S_MAX = 40.0                              # the bound's condition on |scaled score|
COVER_MIN = 0.25                          # every key index gets at least this probability from some row


def reference(q, k, v, scale):
    """fp64 softmax attention on fp16 (B,N,H,D) operands.  Returns out [B,Nq,H,D], the probabilities p [B,H,Nq,Nk],
    A = sum_j p_j |v_j| [B,Nq,H,D] (all fp64) and the largest |scaled score|."""
    qd, kd, vd = (t.double().permute(0, 2, 1, 3) for t in (q, k, v))          # [B,H,N,D]
    s = torch.matmul(qd, kd.transpose(-1, -2)) * float(scale)
    smax = float(s.abs().max())
    p = torch.softmax(s, dim=-1)
    out = torch.matmul(p, vd).permute(0, 2, 1, 3).contiguous()
    A = torch.matmul(p, vd.abs()).permute(0, 2, 1, 3).contiguous()
    return out, p, A, smax


def bound(A):
    return 3.0 * UNIT * A + 2.0 ** -24


def units(got, out, A):
    """err / (2^-11 A) per element -- the figure the tests print (the 2^-24 floor keeps it finite where A is tiny)."""
    return (got.double() - out).abs() / (UNIT * A + 2.0 ** -24 / 3.0)


def make_inputs(B, H, Nq, Nk, D, seed, spikes=False):
    """fp16 q [B,Nq,H,D], k, v [B,Nk,H,D] in which every key matters to some row: N(0,1) draws, q scaled by 0.7, and row r of head
    (b,h) pulled towards key t = (r + Nq (b H + h)) % Nk by 8 sqrt(D) k_t / |k_t|^2 (its score rises by 8 nats at scale
    D^-0.5).  With `spikes` one channel each of key 0, key min(64, Nk-1) and key Nk-1 is multiplied by 4 after the pull: an early and
    a late running maximum.  The caller picks B so that B H Nq >= Nk (every key index is some row's target)."""
    assert B * H * Nq >= Nk
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Nq, H, D, generator=g).double() * 0.7
    k = torch.randn(B, Nk, H, D, generator=g).double()
    v = torch.randn(B, Nk, H, D, generator=g)
    bh = torch.arange(B)[:, None] * H + torch.arange(H)[None, :]                            # [B,H]
    t = (torch.arange(Nq)[None, :, None] + Nq * bh[:, None, :]) % Nk                        # [B,Nq,H]
    kt = torch.gather(k, 1, t[..., None].expand(B, Nq, H, D))
    q = q + 8.0 * math.sqrt(D) * kt / (kt * kt).sum(-1, keepdim=True)
    if spikes:
        for i, j in enumerate(sorted({0, min(KT, Nk - 1), Nk - 1})):
            k[:, j, :, (3 + 5 * i) % D] *= 4.0
    return q.half(), k.half(), v.half()


def coverage(p):
    """per key index: the largest probability any row of any head gives it."""
    return p.amax(dim=(0, 1, 2))


# ------------------------------------------------------------------------------------------------ emulation
def _partner(j, Nk, extra):
    """a key in the same 64-key tile as key j (the folded key 0 has no tile: its neighbour)."""
    if extra and j == 0:
        return 1
    t = (j - extra) // KT
    lo, hi = extra + t * KT, min(extra + (t + 1) * KT, Nk) - 1
    return j + 1 if j + 1 <= hi else (j - 1 if j - 1 >= lo else j)


def emulate(q, k, v, scale, mutate=None):
    """The kernels' arithmetic in torch: fp32 raw scores, 64-key tiles with a running maximum taken on the raw scores and scaled
    afterwards, p = exp2(s * scale_log2 - m), fp32 row sum of the unrounded p, P rounded to fp16 for the PV product (fp32
    accumulation), key 0 folded in first when Nk > 64 and Nk % 64 == 1, fp16 output.

    mutate names ONE defect: ("drop", j) key j contributes nothing; ("twice", j) key j is counted twice; ("swap_v", j) the V rows
    of key j and of a neighbour in its tile are exchanged; ("no_rescale",) O is not rescaled when the running maximum grows;
    ("fold_twice",) key 0 is folded in AND left in tile 0 (only a defect where the fold applies)."""
    kind, j = (mutate[0], mutate[1] if len(mutate) > 1 else None) if mutate else (None, None)
    assert kind in (None, "drop", "twice", "swap_v", "no_rescale", "fold_twice")
    B, Nq, H, D = q.shape
    Nk = k.shape[1]
    sl2 = torch.tensor(float(scale), dtype=torch.float32) * torch.tensor(1.44269504088896340736, dtype=torch.float32)
    qf, kf, vf = (t.float().permute(0, 2, 1, 3).contiguous() for t in (q, k, v))            # [B,H,N,D]
    extra = 1 if (Nk > KT and Nk % KT == 1) else 0
    if kind == "swap_v":
        j2 = _partner(j, Nk, extra)
        vf = vf.clone()
        vf[:, :, [j, j2]] = vf[:, :, [j2, j]]
    w = torch.ones(Nk, dtype=torch.float32)          # how often a key is counted
    if kind == "drop":
        w[j] = 0.0
    if kind == "twice":
        w[j] = 2.0
    s_all = torch.matmul(qf, kf.transpose(-1, -2))                                          # raw fp32 scores [B,H,Nq,Nk]
    m_run = torch.full((B, H, Nq), -math.inf, dtype=torch.float32)
    l_run = torch.zeros(B, H, Nq, dtype=torch.float32)
    O = torch.zeros(B, H, Nq, D, dtype=torch.float32)
    if extra and w[0] > 0:
        m_run = s_all[..., 0] * sl2
        l_run = torch.full_like(l_run, float(w[0]))
        O = vf[:, :, 0:1, :].expand(B, H, Nq, D) * w[0]
    first = 0 if (kind == "fold_twice" and extra) else extra
    for k0 in range(first, Nk, KT):
        k1 = min(k0 + KT, Nk)
        s = s_all[..., k0:k1]
        wt = w[k0:k1]
        live = wt > 0
        if not bool(live.any()):
            continue
        mloc = s[..., live].amax(-1) * sl2
        m_new = torch.maximum(m_run, mloc)
        alpha = torch.exp2(m_run - m_new)
        m_run = m_new
        p = torch.where(live, torch.exp2(s * sl2 - m_new[..., None]), torch.zeros(())) * wt
        l_run = l_run * alpha + p.sum(-1)
        if kind != "no_rescale":
            O = O * alpha[..., None]
        O = O + torch.matmul(p.half().float(), vf[:, :, k0:k1])
    out = (O * (1.0 / l_run)[..., None]).half()
    return out.permute(0, 2, 1, 3).contiguous()


# ------------------------------------------------------------------------------------------------ the GPU matrix
# (id, D, pipelined, NW): every kernel instance the library builds; the code cut3r_attention_kernel_for returns is 100 * pipelined + NW
INSTANCES = [("d16-staged-nw2", 16, 0, 2), ("d16-staged-nw4", 16, 0, 4), ("d32-staged-nw2", 32, 0, 2), ("d32-staged-nw4", 32, 0, 4),
             ("d48-pipelined", 48, 1, 4), ("d48-staged-nw2", 48, 0, 2), ("d48-staged-nw4", 48, 0, 4),
             ("d64-pipelined", 64, 1, 4), ("d64-staged-nw2", 64, 0, 2), ("d64-staged-nw4", 64, 0, 4), ("d128-staged-nw4", 128, 0, 4)]
NK_EDGES = (1, 2, 63, 64, 65, 66, 127, 128, 129, 130, 193)      # one key, the tile edge, the fold (65, 129, 193), two and three tiles
NQ_EDGES = (1, 31, 32, 33, 64, 65, 127, 128, 129)               # idle waves, a clamped last row, a second query block
BIG_HEADS = (48, 8)                                             # B, H with B H = 384: attn_kernel<D, 4> for D < 128


def many_heads(D, pipelined, NW):
    """whether the instance is reached only with 384 (batch, head) pairs: the staged four-wave kernel of the head widths below 128."""
    return (not pipelined) and NW == 4 and D < 128


def shapes(big):
    """(Nq, Nk) pairs of the reference test; the 384-head instances use query counts 1, 33, 128 (128: B H ceil(Nq/128) stays 384)."""
    nqs = (1, 33, 128) if big else (1, 33, 129)
    out = [(nq, nk) for nk in NK_EDGES for nq in nqs]
    for nq in (nqs if big else NQ_EDGES):
        for nk in (65, 130):
            if (nq, nk) not in out:
                out.append((nq, nk))
    return out


def heads(big, Nq, Nk):
    """B, H of a case: 384 pairs for the four-wave instances; else 3 heads and enough batches that every key index is the target of
    four rows (at least 2 batches), but fewer than 384 workgroups' worth, so the two-wave instance still serves it."""
    if big:
        return BIG_HEADS
    return min(127, max(2, -(-4 * Nk // (3 * Nq)))), 3


def seed_of(Nq, Nk, D, spikes, attempt=0):
    return 1000 * Nq + 7 * Nk + D + (500000 if spikes else 0) + 1000000 * attempt


ATTEMPTS = 24


class Case:
    """inputs and fp64 reference of one case: made once, read by every test that needs it, never written.

    The two input conditions -- |scaled score| <= 40 (the bound's own condition) and, at the scale D^-0.5 the pull is sized for, every
    key index with probability >= 0.25 in some row (so a wrong key cannot hide) -- are properties of the draw and of the fp64 reference
    alone.  Where a key index is the target of one or two rows only (one query row, 16-wide heads: the other keys' scores then spread by
    2 nats) a draw can miss the second one, so the draw is repeated with the next seed until both hold (two cases of the matrix, both
    16-wide with one query row and 193 keys, take a later seed); no kernel output is involved in that choice.  `check_inputs` asserts them."""

    def __init__(self, B, H, Nq, Nk, D, spikes, scale_mul=1.0):
        self.shape = (B, H, Nq, Nk, D)
        self.scale = scale_mul * D ** -0.5
        self.need_cover = scale_mul == 1.0
        self.name = f"B{B} H{H} Nq{Nq} Nk{Nk} D{D}{' spikes' if spikes else ''}" + (f" scale x{scale_mul}" if scale_mul != 1.0 else "")
        for self.attempt in range(ATTEMPTS):
            self.q, self.k, self.v = make_inputs(B, H, Nq, Nk, D, seed_of(Nq, Nk, D, spikes, self.attempt), spikes)
            self.out, p, self.A, self.smax = reference(self.q, self.k, self.v, self.scale)
            self.cover = float(coverage(p).min())
            if self.smax <= S_MAX and (self.cover >= COVER_MIN or not self.need_cover):
                break

    def check_inputs(self):
        assert self.smax <= S_MAX, f"{self.name}: largest |scaled score| {self.smax:.1f} > {S_MAX}"
        assert self.cover >= COVER_MIN or not self.need_cover, f"{self.name}: some key index gets at most p = {self.cover:.3f} from any row"


@functools.lru_cache(maxsize=1024)
def _small_case(B, H, Nq, Nk, D, spikes, scale_mul):
    return Case(B, H, Nq, Nk, D, spikes, scale_mul)


def case(B, H, Nq, Nk, D, spikes, scale_mul=1.0):
    """the few-head cases are shared (the pipelined and the staged two-wave instance run the same ones); the 384-head ones are large
    and each is used once"""
    if B * H >= 384:
        return Case(B, H, Nq, Nk, D, spikes, scale_mul)
    return _small_case(B, H, Nq, Nk, D, spikes, scale_mul)


SCALE_CASES = ((33, 130, 0.5), (33, 130, 1.5))                 # (Nq, Nk, multiple of D^-0.5): no spikes, so |s| stays inside 40
