"""CPU: the references of tests/geom_oracle.py against the reference's own outputs and hand-worked examples, and the proof that every
case of tests/geom_cases.py meets the conditions the GPU tests (tests/test_geom_gpu.py) rely on."""
import os

import numpy as np
import pytest

from oracle import geom as G
from tests import geom_cases as GC
from tests import geom_oracle as GO

GOLD = os.path.join(os.path.dirname(__file__), "golden")


# ------------------------------------------------------------------------------------------------ the references
def test_row_maxima_and_ratio_reproduce_the_reference_outputs():
    f = np.load(os.path.join(GOLD, "graph.npz"))
    Nv = f["feat0"].shape[0] - 1
    for k, ref in enumerate(f["patch_ratios"]):
        mx = GO.row_maxima64(f["feat0"], f[f"feat1_{k}"])
        assert mx.shape == (Nv,)
        count = int((mx > 0.7).sum())
        assert abs(count / Nv - ref) < 1e-6 and abs(GO.ratio_of(count, Nv) - ref) < 1e-6, (k, count, ref)


def test_normalised_rows_drop_row_zero_and_floor_the_norm():
    x = np.array([[9, 9], [3, 4], [0, 0], [0, -2e-13]], np.float32)
    n = GO.normalised_rows64(x)
    assert n.shape == (3, 2)
    np.testing.assert_allclose(n[0], [0.6, 0.8], rtol=1e-15)
    assert (n[1] == 0).all()
    np.testing.assert_allclose(n[2], [0, np.float64(np.float32(-2e-13)) / 1e-12], rtol=1e-15)     # below the floor: divided by 1e-12


def test_chain_scan_without_decisions_is_b_independent_ratios():
    case = GC.chain_case("mixed", 33, 8)
    scan = GO.chain_scan(case["feat_last"], case["feats"], 0.7, -1.0, None)
    assert scan["state"] == -1 and not scan["decisions"].any() and scan["against"] == [-1] * len(case["feats"])
    for i, f in enumerate(case["feats"]):
        assert scan["counts"][i] == int((GO.row_maxima64(case["feat_last"], f) > 0.7).sum())


def test_chain_scan_on_a_hand_made_example():
    """Nv = 4, C = 8, exact axes.  last = (e0, e0, e1, e1).  A = (e0, e2, e2, e2): 2 of 4 rows of `last` match, ratio 0.5 < 0.6:
    taken.  B = (e2, e2, e2, e1) against A: 3 of 4, 0.75: skipped.  X = (e3, e3, e3, e3) is forced: count 0, taken.
    D = (e3, e1, e1, e1) against X: 4 of 4: skipped (against `last` it would be 2 of 4 and taken; against A, 0 of 4)."""
    e = np.eye(8, dtype=np.float32)
    mk = lambda idx: np.concatenate([np.full((1, 8), 3.0, np.float32), e[list(idx)]])
    last, A, B, X, D = mk((0, 0, 1, 1)), mk((0, 2, 2, 2)), mk((2, 2, 2, 1)), mk((3, 3, 3, 3)), mk((3, 1, 1, 1))
    scan = GO.chain_scan(last, [A, B, X, D], 0.7, 0.6, [0, 0, 1, 0])
    assert scan["counts"].tolist() == [2, 3, 0, 4] and scan["decisions"].tolist() == [1, 0, 1, 0]
    assert scan["state"] == 2 and scan["against"] == [-1, 0, 0, 2] and scan["dist"][2] is None
    np.testing.assert_allclose(scan["dist"][0], [0.3, 0.3, 0.7, 0.7], atol=1e-12)


def test_the_two_ties_come_out_as_stated():
    assert GO.ratio_of(63, 70) < 0.9 and not (63 / 70 < 0.9)                 # fp32 quotient widened: taken; plain fp64: not
    assert GO.ratio_of(16, 32) == 0.5 and not (GO.ratio_of(16, 32) < 0.5)
    for C in (8, 64):
        t70, t32 = GC.chain_case("tie70", 70, C), GC.chain_case("tie32", 32, C)
        s70 = GO.chain_scan(t70["feat_last"], t70["feats"], 0.7, 0.9, None)
        s32 = GO.chain_scan(t32["feat_last"], t32["feats"], 0.7, 0.5, None)
        assert s70["counts"][0] == 63 and s70["decisions"][0] == 1
        assert s32["counts"][:2].tolist() == [16, 16] and s32["decisions"][:2].tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("N,C", GC.OVERLAP_SHAPES)
@pytest.mark.parametrize("variant", GC.OVERLAP_VARIANTS)
def test_overlap_cases_keep_clear_of_the_threshold_and_hold_their_planted_rows(N, C, variant):
    case = GC.overlap_case(N, C, variant)
    Nv = N - 1
    mx = GO.row_maxima64(case["feat0"], case["feat1"])
    assert np.abs(mx - case["thr"]).min() > GO.max_bound(C)
    n0, n1 = GO.normalised_rows64(case["feat0"]), GO.normalised_rows64(case["feat1"])
    p = case["planted"]
    if variant == "zero":
        assert (n0[p["zero0"]] == 0).all() and mx[p["zero0"]] == 0
        if Nv >= 2:
            assert (n1[p["zero1"]] == 0).all()
    elif variant == "negative":
        assert mx[p["negative"]] < -0.1                                      # far beyond any rounding: the clamp must act
    else:
        assert all(abs(mx[r] - 1.0) < 1e-12 for r in p["duplicate"])
    if Nv >= 30:
        count = int((mx > case["thr"]).sum())
        assert 0 < count < Nv


@pytest.mark.parametrize("name,Nv,C", GC.CHAIN_CASES)
def test_chain_cases_meet_their_conditions(name, Nv, C):
    case = GC.chain_case(name, Nv, C)
    feats, last, forced = case["feats"], case["feat_last"], case["forced"]
    B = len(feats)
    assert 5 <= B <= 7
    scan = GO.chain_scan(last, feats, case["thr_sim"], case["thr_ratio"], forced)
    assert scan["decisions"].tolist() == case["decisions"]
    assert 0 < sum(case["decisions"]) < B
    # planted: every row maximum of every step is a match (> 0.8) or not (< 0.5), and the count is the number of rows whose type
    # occurs in the candidate -- so no row is anywhere near the band of (2C + 6) u around thr_sim
    assert GO.min_distance(scan) > GO.max_bound(C)
    for i in range(B):
        if scan["dist"][i] is None:
            assert scan["counts"][i] == 0 and scan["decisions"][i] == 1
            continue
        k = scan["against"][i]
        mx = GO.row_maxima64(last if k < 0 else feats[k], feats[i])
        assert ((mx > GC.MATCHED_ABOVE) | (mx < GC.UNMATCHED_BELOW)).all()
        assert scan["counts"][i] == GC.expected_count(case["types_last"] if k < 0 else case["types"][k], case["types"][i])
    if name == "mixed":
        # >= 2 candidates whose count AND decision differ from the scan against feat_last and from the scan against the
        # immediately preceding candidate: a kernel that ignored the state, or used the previous candidate, fails
        telling = 0
        for i in range(1, B):
            c_last = int((GO.row_maxima64(last, feats[i]) > case["thr_sim"]).sum())
            c_prev = int((GO.row_maxima64(feats[i - 1], feats[i]) > case["thr_sim"]).sum())
            d_last, d_prev = (int(GO.ratio_of(c, Nv) < case["thr_ratio"]) for c in (c_last, c_prev))
            c, d = scan["counts"][i], scan["decisions"][i]
            telling += int(c != c_last and c != c_prev and d != d_last and d != d_prev)
        assert telling >= 2
    if name == "forced_mid":
        i = forced.index(1)
        assert 0 < i < B - 1 and scan["against"][i + 1] == i
        unforced = GO.chain_scan(last, feats, case["thr_sim"], case["thr_ratio"], None)
        assert unforced["decisions"][i] == 0                                  # forcing changes the decision ...
        assert unforced["counts"][i + 1] != scan["counts"][i + 1] and unforced["decisions"][i + 1] != scan["decisions"][i + 1]     # ... and what follows
    if name == "forced_first":
        assert forced[0] == 1 and np.array_equal(last, feats[0])
    if name in ("tie70", "tie32"):
        # the other outcome of the tie would change a later count: the tie is visible beyond its own decision
        other = np.nextafter(0.5, 1.0) if name == "tie32" else GO.ratio_of(63, 70)      # the nearest threshold that decides the other way
        flipped = GO.chain_scan(last, feats, case["thr_sim"], other, None)
        assert flipped["decisions"][0] != scan["decisions"][0] and (flipped["counts"] != scan["counts"]).any()


@pytest.mark.parametrize("B,N,has_align,clamp_z", GC.FWD_CASES)
def test_forward_cases_are_not_vacuous_in_any_camera_chunk(B, N, has_align, clamp_z):
    case = GC.fwd_case(B, N, has_align)
    assert case["pm"].shape == (N, 3) and case["w2c"].shape == (B, 12)
    assert GC.chunks_not_vacuous(GC.fwd_reference(case, clamp_z), N)


def test_aligning_through_the_oracle_equals_aligning_an_image():
    """fwd_reference aligns the N points as an N x 1 image: the same per-point chain as the 24 x 32 image"""
    case = GC.fwd_case(65, 768, True)
    a = G.align_view(case["pm"].reshape(24, 32, 3), np.ones((24, 32), np.float32), case["P12"], case["s"], 1)[0].reshape(-1, 3)
    b = G.align_view(case["pm"].reshape(-1, 1, 3), np.ones((768, 1), np.float32), case["P12"], case["s"], 1)[0].reshape(-1, 3)
    np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("name", ["stride", "slots", "one"])
def test_backward_cases(name):
    case = GC.bwd_case(name)
    N, B = case["N"], case["B"]
    assert N % 4 == 0
    slots = [GO.slot_of(b, case["grp"], case["grp_stride"]) for b in range(B)]
    ref = G.overlap_bwd(case["store"][slots], case["w2c"], case["K4"], case["W"], case["H"])
    assert ((ref > 0) & (ref < N)).all()
    if name == "stride":
        assert N > 64 * 256 * 4                                              # beyond one pass of the capped grid
        tail = G.overlap_bwd(case["store"][:, 65536:], case["w2c"], case["K4"], case["W"], case["H"])
        assert ((tail > 0) & (tail < N - 65536)).all()                       # the second pass changes every count
    if name == "slots":
        unused = G.overlap_bwd(case["store"][5:6], case["w2c"], case["K4"], case["W"], case["H"])[0]
        assert unused == N and slots == [0, 1, 2, 3, 4, 6, 7]
        plain = G.overlap_bwd(case["store"][:B], case["w2c"], case["K4"], case["W"], case["H"])
        assert plain[5] != ref[5] and plain[6] != ref[6]                     # slot = b would be seen


def _window_ref(case):
    v = GC.window_views(case)
    return GO.window_reference(case["pts"], case["conf"], case["P"], case["s"], case["ds"], v["store"], v["dst_slot"], v["w2c"], v["t0"],
                               case["first"], case["K4"], case["ldc"], w2c_new=v["w2c"][v["t0"]:v["t0"] + case["V"]] if case["has_w2c"] else None)


@pytest.mark.parametrize("name", sorted(GC.WINDOW_CASES))
def test_window_cases_count_something_but_not_everything(name):
    case = GC.window_case(name)
    ref = _window_ref(case)
    t0, V, counts = GC.window_views(case)["t0"], case["V"], ref["counts"]
    assert counts.shape == (V, 2, case["ldc"]) and case["ldc"] >= t0 + V
    if case["first"] > t0 + V:
        assert not counts.any()
        return
    assert GC.counted_rows_not_vacuous(case, counts)
    for v in range(V):
        kfi = t0 + v
        assert not counts[v, :, kfi:].any()
        if kfi < case["first"]:
            assert not counts[v].any()
    if name == "two_chunks":
        assert t0 > 64 and all(counts[v, 0, 64:t0 + v].any() for v in range(V))          # the second chunk contributes to every view
    if name == "chunk_boundary":
        assert t0 + V - 1 == 65 and counts[V - 1, 0, 64] > 0 and counts[V - 2, 0, 63] > 0     # kfi = 65 sees camera 64; kfi = 64 ends at 63
    if name == "warm_up":
        assert not counts[:3].any() and counts[3, 0, :3].all()


def test_window_reference_agrees_with_direct_oracle_calls_on_the_existing_configuration():
    """V = 6, t0 = 10, first = 3 (the configuration of test_window_update_matches_per_keyframe_calls): the counts of the last and of
    a middle view, assembled by hand from G.align_view / G.overlap_fwd / G.overlap_bwd"""
    case = GC.window_case("no_lsum_reset")
    assert (case["t0"], case["V"], case["first"], case["ds"]) == (10, 6, 3, 2)
    ref = _window_ref(case)
    H, W, K4 = case["H"], case["W"], case["K4"]
    store = case["store"].copy()
    for v in range(6):
        store[2, v] = G.align_view(case["pts"][v], case["conf"][v], case["P"][v], case["s"], 2)[0]
    np.testing.assert_array_equal(ref["store"].reshape(store.shape), store)
    for v in (2, 5):
        kfi = 10 + v
        full = G.align_view(case["pts"][v], case["conf"][v], case["P"][v], case["s"], 1)[0]
        np.testing.assert_array_equal(ref["counts"][v, 0, :kfi], G.overlap_fwd(full, case["w2c"][:kfi], K4, W, H))
        maps = np.stack([store[b // 5, b % 5] for b in range(kfi)])
        np.testing.assert_array_equal(ref["counts"][v, 1, :kfi], G.overlap_bwd(maps, case["w2c"][kfi], K4, W // 2, H // 2))
        assert not ref["counts"][v, :, kfi:].any()
    d = G.align_view(case["pts"][3], case["conf"][3], case["P"][3], case["s"], 2)
    np.testing.assert_array_equal(ref["conf_ds"][3], d[1])
    np.testing.assert_array_equal(ref["depth"][3], d[2])


def test_logdepth_marked_case_sums_to_minus_four_log_two():
    prev, pts = GC.logdepth_marked()
    assert prev.shape == (GC.LOGDEPTH_N,) and GC.LOGDEPTH_N > 512 * 256 and (pts[:, 2] == 2.0).sum() == 4
    assert abs(G.logdepth_sum(prev, pts) + 4 * float(np.log(np.float32(2.0)))) < 1e-6
