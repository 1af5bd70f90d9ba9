"""CPU: the attention oracle (tests/attention_oracle.py) can tell a right kernel from a wrong one -- before any kernel runs.

  * the inputs of EVERY case of the GPU matrix (tests/test_attention_gpu.py) meet the two conditions the check rests on: scaled
    scores inside the bound's |s| <= 40, and every key index with probability >= 0.25 in some row;
  * the clean emulation of the kernels' arithmetic stays inside the per-element bound 3 * 2^-11 * A + 2^-24 (measured here: at most
    1.53 units of 2^-11 A, see the printed lines), so the bound is not tighter than the arithmetic it allows;
  * every named defect -- a dropped key, a key counted twice, two V rows of a tile exchanged, a missing rescale of O, key 0 folded in
    and also left in tile 0 -- at key 0, 63, 64, Nk-1 and mid-range, leaves some element outside the bound by a factor of at least 20
    (measured: 74 at the least), so the bound is not looser than the defects it must catch.
"""
import pytest
import torch

from tests import attention_oracle as AO

CONFIGS = [(D, big) for D in (16, 32, 48, 64, 128) for big in (False, True) if not (big and D == 128)]


def _cases(D, big, scales=True):
    for nq, nk in AO.shapes(big):
        for spikes in (False, True):
            yield AO.case(*AO.heads(big, nq, nk), nq, nk, D, spikes)
    if scales:
        for nq, nk, mul in AO.SCALE_CASES:
            yield AO.case(*AO.heads(big, nq, nk), nq, nk, D, False, mul)


def test_the_matrix_names_every_instance_once_and_reaches_the_four_wave_ones_with_384_heads():
    assert len(AO.INSTANCES) == 11 and len({i[0] for i in AO.INSTANCES}) == 11
    assert {(D, p, nw) for _, D, p, nw in AO.INSTANCES} == (
        {(D, 0, nw) for D in (16, 32, 48, 64) for nw in (2, 4)} | {(48, 1, 4), (64, 1, 4), (128, 0, 4)})
    for big in (False, True):
        sh = AO.shapes(big)
        assert len(sh) == len(set(sh))
        for nq, nk in sh:
            B, H = AO.heads(big, nq, nk)
            assert B * H * nq >= nk
            assert (B * H * ((nq + 127) // 128) >= 384) == big          # the launcher's rule for four waves below D = 128
    nqs = {nq for nq, _ in AO.shapes(False)}
    assert nqs == set(AO.NQ_EDGES) and {nk for _, nk in AO.shapes(False)} == set(AO.NK_EDGES)
    assert all((nq, nk) in AO.shapes(False) for nq in AO.NQ_EDGES for nk in (65, 130))
    assert all((nq, nk) in AO.shapes(False) for nq in (1, 33, 129) for nk in AO.NK_EDGES)
    assert all((nq, nk) in AO.shapes(True) for nq in (1, 33, 128) for nk in AO.NK_EDGES)


@pytest.mark.parametrize("D,big", CONFIGS)
def test_inputs_of_every_gpu_case_meet_the_two_conditions(D, big):
    cover, smax, n = 1.0, 0.0, 0
    for c in _cases(D, big):
        c.check_inputs()
        if c.need_cover:
            cover = min(cover, c.cover)
        smax, n = max(smax, c.smax), n + 1
    print(f"[attention] inputs D={D} heads={'384' if big else 'few'}: {n} cases, smallest coverage {cover:.3f}, largest |s| {smax:.1f}")


def test_reference_is_softmax_attention():
    """the oracle against a second statement of the operation (per-row loops in numpy), one key and a fold shape"""
    import numpy as np
    for B, H, Nq, Nk, D in ((2, 3, 5, 1, 16), (6, 4, 3, 65, 32)):
        q, k, v = AO.make_inputs(B, H, Nq, Nk, D, 3, spikes=True)
        out, p, A, smax = AO.reference(q, k, v, D ** -0.5)
        qn, kn, vn = (t.double().numpy() for t in (q, k, v))
        for b in range(B):
            for h in range(H):
                s = qn[b, :, h] @ kn[b, :, h].T * D ** -0.5
                e = np.exp(s - s.max(-1, keepdims=True))
                pr = e / e.sum(-1, keepdims=True)
                assert np.allclose(p[b, h].numpy(), pr, rtol=1e-12, atol=1e-300)
                assert np.allclose(out[b, :, h].numpy(), pr @ vn[b, :, h], rtol=1e-12, atol=1e-15)
                assert np.allclose(A[b, :, h].numpy(), pr @ np.abs(vn[b, :, h]), rtol=1e-12, atol=1e-15)
                assert smax >= np.abs(s).max() - 1e-9
        assert torch.allclose(p.sum(-1), torch.ones(B, H, Nq, dtype=torch.float64), atol=1e-12)


@pytest.mark.parametrize("D", (16, 32, 48, 64, 128))
def test_clean_emulation_stays_inside_the_bound(D):
    worst = 0.0
    for c in _cases(D, False):
        got = AO.emulate(c.q, c.k, c.v, c.scale)
        err = (got.double() - c.out).abs()
        worst = max(worst, float(AO.units(got, c.out, c.A).max()))
        over = err > AO.bound(c.A)
        assert not bool(over.any()), f"{c.name}: {int(over.sum())} elements of the clean emulation outside the bound"
    print(f"[attention] emulation D={D}: worst err / (2^-11 A) = {worst:.3f}")
    assert worst <= 3.0


def _defects(Nk):
    fold = Nk > AO.KT and Nk % AO.KT == 1
    js = sorted({j for j in (0, 63, 64, Nk - 1, Nk // 2) if j < Nk})
    out = [(kind, j) for kind in ("drop", "twice", "swap_v") for j in js]
    out.append(("no_rescale",))
    if fold:
        out.append(("fold_twice",))
    return out


@pytest.mark.parametrize("D", (16, 32, 48, 64, 128))
def test_every_defect_leaves_the_bound_by_a_factor_of_20(D):
    smallest = float("inf")
    for nq, nk, spikes in ((33, 65, True), (33, 129, False), (33, 130, True), (129, 193, False), (1, 130, False)):
        c = AO.case(*AO.heads(False, nq, nk), nq, nk, D, spikes)
        c.check_inputs()
        for mut in _defects(nk):
            got = AO.emulate(c.q, c.k, c.v, c.scale, mutate=mut)
            ratio = float(((got.double() - c.out).abs() / AO.bound(c.A)).nan_to_num(nan=float("inf")).max())
            smallest = min(smallest, ratio)
            assert ratio >= 20.0, f"{c.name}: defect {mut} stays within {ratio:.1f} x the bound -- the GPU test would not see it"
    print(f"[attention] defects D={D}: smallest worst-element err / bound = {smallest:.0f}")


def test_emulation_refuses_an_unknown_defect():
    q, k, v = AO.make_inputs(1, 1, 2, 2, 16, 0)
    with pytest.raises(AssertionError):
        AO.emulate(q, k, v, 0.25, mutate=("typo", 0))
