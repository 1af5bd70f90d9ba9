"""CPU: the preconditions that the dense-BA shape tests (tests/test_ba_shapes_gpu.py) rely on, checked with the oracle alone -- a GPU
case that is meant to reach a sparse source set or the depth mask must not pass because its scene quietly stopped reaching it."""
import numpy as np
import torch

from cut3r_slam_amd.ba import edge_structure
from oracle import ba_oracle as BO
from tests import ba_scenes as SC


def test_default_scene_is_the_dense_band_with_every_frame_a_source():
    poses, disps, intr, ii, jj, tgt, wgt, eta = SC.scene(4, 6, 8, 4)
    assert sorted(zip(ii.tolist(), jj.tolist())) == sorted((i, j) for i in range(4) for j in range(4) if i != j and abs(i - j) <= 2)
    assert np.array_equal(np.unique(ii), np.arange(4)) and eta.shape == (4, 6, 8)
    assert disps.min() >= 0.3 and disps.max() <= 0.6
    # the keywords leave the arrays drawn before them alone: same poses in y, z and rotation, same disparities outside the patch
    p2, d2, *_ = SC.scene(4, 6, 8, 4, patch=(1, 1, 3, 2, 5))
    assert np.array_equal(p2, poses)
    keep = np.ones_like(disps, bool)
    keep[1, 1:3, 2:5] = False
    assert np.array_equal(d2[keep], disps[keep]) and d2[~keep].min() >= 3.5 and d2[~keep].max() <= 5.0


def test_case_sizes_reach_the_blocks_and_waves_they_are_named_for():
    want = {"two_blocks": (323, 18), "three_blocks": (667, 18), "block_exact": (256, 18), "block_plus_two": (258, 18), "free_gauge": (48, 24),
            "two_waves": (48, 72), "three_waves": (24, 132), "limit_33": (24, 192), "limit_34": (24, 192), "sparse_sources": (323, 24),
            "masked": (323, 18)}
    assert set(want) == set(SC.CASES)
    for name, (P, ht, wd, seed, fixedp, kw) in SC.CASES.items():
        assert (ht * wd, 6 * (P - fixedp)) == want[name], name
    P, ht, wd, seed, fixedp, kw = SC.BEYOND
    assert 6 * (P - fixedp) == 198


def test_sparse_source_scene_has_three_sources_and_a_duplicate_edge():
    P, ht, wd, seed, fixedp, kw = SC.CASES["sparse_sources"]
    assert (P, ht, wd, seed, kw["step"]) == (5, 17, 19, 5, 0.15)
    poses, disps, intr, ii, jj, tgt, wgt, eta = SC.case_scene("sparse_sources")
    kx, kk, order, src_ptr, present = edge_structure(torch.from_numpy(ii), torch.from_numpy(jj), P, fixedp)
    assert kx.tolist() == [1, 3, 4] and eta.shape == (3, ht, wd)                    # M = 3 < P, kx != arange
    edges = list(zip(ii.tolist(), jj.tolist()))
    assert len(edges) == 10 and len(set(edges)) == 9 and edges.count((3, 2)) == 2   # one duplicated edge
    assert 0 not in ii and 2 not in ii and 0 in jj and 2 in jj                      # frame 0 (fixed) and frame 2 (free) are only targets
    assert src_ptr.tolist() == [0, 3, 7, 10]
    assert [ii[e] for e in order] == [1, 1, 1, 3, 3, 3, 3, 4, 4, 4]                 # the CSR walk groups the edges by source
    # E blocks [Pf, M]: free pose 2 - 1 = 1 is never a source but is a target of every source; source 4 never meets pose 1 - 1 = 0
    assert present.tolist() == [[1, 1, 0], [1, 1, 1], [1, 1, 1], [0, 1, 1]]
    dx, dz, kx_o = SC.case_reference("sparse_sources")
    assert kx_o.tolist() == [1, 3, 4] and dx.shape == (4, 6) and dz.shape == (3, ht * wd)
    assert float(dx.abs().max()) > 1e-3 and float(dz.abs().max()) > 1e-3            # the step is not trivially zero


def test_masked_scene_masks_a_few_percent_and_keeps_clear_of_the_thresholds():
    P, ht, wd, seed, fixedp, kw = SC.CASES["masked"]
    assert (P, ht, wd, seed, kw) == (4, 17, 19, 4, dict(step=0.15, back=2, patch=(1, 3, 9, 4, 12)))
    poses, disps, intr, ii, jj, tgt, wgt, eta = SC.case_scene("masked")
    Z = SC.edge_depths(poses, disps, intr, ii, jj)
    assert Z.shape == (len(ii), ht * wd)
    share = float((Z <= 0.2).double().mean())
    near = float(torch.minimum((Z - 0.1).abs(), (Z - 0.2).abs()).min())
    print(f"[masked scene] share of (edge, pixel) pairs with Z <= 0.2: {share:.4f}; nearest Z to a threshold: {near:.4f}")
    assert 0.01 <= share <= 0.10
    assert near >= 0.01
    assert bool((Z < 0.1).any()) and bool((Z > 0.2).any())                          # both branches of the depth mask
    # the oracle's own mask agrees with Z, edge by edge
    G = BO.se3_matrix(poses)
    for e in range(len(ii)):
        _, valid = BO.project(G[jj[e]] @ torch.linalg.inv(G[ii[e]]), torch.from_numpy(disps[ii[e]]), intr[ii[e]], intr[jj[e]], ht, wd)
        assert torch.equal(valid > 0, Z[e] > 0.2)
    # the other scenes never mask anything: that is the gap this scene closes
    p0, d0, i0, ii0, jj0, *_ = SC.case_scene("two_blocks")
    assert float(SC.edge_depths(p0, d0, i0, ii0, jj0).min()) > 0.2


def test_ba_dense_returns_the_system_it_solved():
    poses, disps, intr, ii, jj, tgt, wgt, eta = SC.case_scene("free_gauge")
    dx, dz, kx, H, g = SC.case_reference("free_gauge", True)
    dx0, dz0, kx0 = SC.case_reference("free_gauge")
    assert torch.equal(dx, dx0) and torch.equal(dz, dz0)
    sol = torch.cat([dx.reshape(-1), dz.reshape(-1)])
    assert H.shape == (sol.numel(), sol.numel()) and torch.allclose(H, H.T, rtol=0, atol=1e-12 * float(H.abs().max()))
    assert float((H @ sol - g).abs().max()) <= 1e-9 * float(g.abs().max())
