"""GPU: the dense-BA kernels of csrc/ba.hip at the sizes where they change behaviour -- several pixel blocks of 256 (the Hpart layout, the
edge fold, the k += 256 strides, the workspace offsets), Cholesky rows in a second and third wave (n = 6 (P - fixedp) up to the limit of
192, where a missing barrier shows), source sets with M < P and kx != arange (everything indexed by source slot m, not by frame), the depth
mask, the solve alone through the C ABI, the mono-prior solve at n = 65, 66, 192, and cut3r_ba_step inside a guarded workspace.
References: oracle/ba_oracle.py (fp64, numerical Jacobians, un-reduced dense solve) and fp64 torch on the CPU; the scenes and their
preconditions are tests/ba_scenes.py and tests/test_ba_scenes_cpu.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cut3r_slam_amd import _lib  # noqa: E402
from cut3r_slam_amd import ba as B  # noqa: E402
from cut3r_slam_amd import droid_backends as db  # noqa: E402
from cut3r_slam_amd.lietorch import SE3  # noqa: E402
from oracle import ba_oracle as BO  # noqa: E402
from oracle import lie_oracle as LO  # noqa: E402
from tests import ba_scenes as SC  # noqa: E402

DEV = "cuda:0"


def _f(a):
    return torch.from_numpy(np.asarray(a)).float().to(DEV)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ba_args(scene):
    poses, disps, intr, ii, jj, tgt, wgt, eta = scene
    return (_f(tgt)[None], _f(wgt)[None], _f(eta), SE3(_f(poses)[None]), _f(disps)[None], _f(intr)[None], torch.from_numpy(ii), torch.from_numpy(jj))


@functools.lru_cache(maxsize=None)
def _ba(name):
    """ba.BA on a named case, once per process: (new_poses matrices, new_disps, dx, dz, failed) on the CPU"""
    fixedp = SC.CASES[name][4]
    new_poses, new_disps, info = B.BA(*_ba_args(SC.case_scene(name)), fixedp=fixedp)
    torch.cuda.synchronize()
    return new_poses.matrix()[0].cpu().double(), new_disps[0].cpu().double(), info["dx"].cpu(), info["dz"].cpu(), int(info["failed"].item())


def _f32_cpu_error(name):
    """the un-reduced system of the oracle solved once in float32 on the CPU: (error of dx, error of dz), each relative to the largest
    component of the fp64 solution -- what the conditioning of the case costs ANY float32 solver"""
    dx_ref, dz_ref, kx, H, g = SC.case_reference(name, True)
    sol = torch.linalg.solve(H.float(), g.float()).double()
    nx = dx_ref.numel()
    return (float((sol[:nx] - dx_ref.reshape(-1)).abs().max() / dx_ref.abs().max()),
            float((sol[nx:] - dz_ref.reshape(-1)).abs().max() / dz_ref.abs().max()))


def _check_step(name, dx, dz, rel=(5e-3, 5e-3)):
    """dx, dz against BO.ba_dense with the bound of test_ba_step_matches_unreduced_dense_solve: rel * largest reference component + 1e-6"""
    dx_ref, dz_ref, kx = SC.case_reference(name)
    dx, dz = dx.cpu().double(), dz.cpu().double()
    assert dx.shape == dx_ref.shape and dz.shape == dz_ref.shape
    sx, sz = dx_ref.abs().max().item(), dz_ref.abs().max().item()
    ex, ez = (dx - dx_ref).abs().max().item(), (dz - dz_ref).abs().max().item()
    print(f"[ba step {name}] dx err {ex / sx:.2e} (bound {rel[0]:.2e}), dz err {ez / sz:.2e} (bound {rel[1]:.2e}) of the largest component")
    assert sx > 1e-3 and sz > 1e-3                                  # the step is not trivially zero
    assert ex <= rel[0] * sx + 1e-6, (name, ex / sx)
    assert ez <= rel[1] * sz + 1e-6, (name, ez / sz)


def _check_update(name, Mnew, nd):
    """retracted poses and clamped disparities, as test_ba_step_matches_unreduced_dense_solve checks them"""
    P, ht, wd, seed, fixedp, kw = SC.CASES[name]
    poses, disps = SC.case_scene(name)[:2]
    dx_ref, dz_ref, kx = SC.case_reference(name)
    sz = dz_ref.abs().max().item()
    G = BO.se3_matrix(poses)
    for p in range(P):
        ref = G[p] if p < fixedp else torch.from_numpy(LO.exp_matrix(1, dx_ref[p - fixedp].numpy())) @ G[p]
        np.testing.assert_allclose(Mnew[p].numpy(), ref.numpy(), atol=5e-4)
    ref_d = torch.from_numpy(disps).clone()
    ref_d[torch.from_numpy(kx)] += dz_ref.reshape(-1, ht, wd)
    ref_d = torch.where(ref_d > 10, torch.zeros_like(ref_d), ref_d).clamp(min=0.001)
    np.testing.assert_allclose(nd.numpy(), ref_d.numpy(), atol=5e-3 * sz + 1e-5)
    frames = np.setdiff1d(np.arange(P), kx)                          # a frame that is no source keeps its disparities exactly
    assert np.array_equal(nd.numpy()[frames], torch.from_numpy(disps).float().double().numpy()[frames])


# ------------------------------------------------------------------------------------------------ 2. the BA step against BO.ba_dense
@pytest.mark.parametrize("name", ["two_blocks", "three_blocks", "block_exact", "block_plus_two", "sparse_sources", "masked", "free_gauge",
                                  "two_waves", "three_waves", "limit_33", "limit_34"])
def test_ba_step_at_block_and_wave_boundaries_matches_unreduced_dense_solve(name):
    """ba.BA against the fp64 un-reduced solve with the bound of test_ba_step_matches_unreduced_dense_solve (5e-3 of the largest reference
    component + 1e-6) at HW = 256, 258, 323, 667 (one to three pixel blocks), n = 72, 132, 192 (two and three waves of Cholesky rows), no
    fixed pose, three sources out of five frames with a duplicated edge, and 1.5 % of the (edge, pixel) pairs behind the depth mask."""
    Mnew, nd, dx, dz, failed = _ba(name)
    assert failed == 0
    if SC.CASES[name][0] - SC.CASES[name][4] >= 22:                  # n >= 132: print what float32 costs on the CPU (not used as a bound)
        e32 = _f32_cpu_error(name)
        print(f"[ba step {name}] CPU float32 solve of the un-reduced system: dx err {e32[0]:.2e}, dz err {e32[1]:.2e}")
    _check_step(name, dx, dz)
    _check_update(name, Mnew, nd)


def test_ba_beyond_the_cholesky_limit_is_refused_with_nothing_written():
    """n = 198 > 192: ba.BA raises, and cut3r_ba_step returns the argument error before its first launch -- workspace, dx, dz, flag untouched"""
    P, ht, wd, seed, fixedp, kw = SC.BEYOND
    scene = SC.scene(P, ht, wd, seed, **kw)
    with pytest.raises(_lib.Cut3rHipError, match="bad argument"):
        B.BA(*_ba_args(scene), fixedp=fixedp)
    rc, big, nws, dx, dz, flag = _call_ba_step(scene, fixedp, n_out=6 * (P - fixedp))
    torch.cuda.synchronize()
    assert rc == 1
    for t in (big, dx, dz):
        assert bool((t.view(torch.int32) == GUARD_BITS).all())
    assert int(flag.item()) == FLAG_SENTINEL


# ------------------------------------------------------------------------------------------------ the other operators on >1 block, M < P
@pytest.mark.parametrize("name", ["two_blocks", "sparse_sources"])
def test_moba_on_two_pixel_blocks_and_sparse_sources(name):
    """test_moba_matches_dense_pose_only_solve (same oracle, same tolerance) with HW = 323 and with three sources out of five frames"""
    P, ht, wd, seed, fixedp, kw = SC.CASES[name]
    poses, disps, intr, ii, jj, tgt, wgt, eta = SC.case_scene(name)
    dx_ref = BO.moba_dense(torch.from_numpy(tgt), torch.from_numpy(wgt), poses, torch.from_numpy(disps), intr, ii, jj, fixedp)
    new_poses = B.MoBA(*_ba_args(SC.case_scene(name)), fixedp=fixedp)
    torch.cuda.synchronize()
    Mnew = new_poses.matrix()[0].cpu().double()
    G = BO.se3_matrix(poses)
    for p in range(P):
        ref = G[p] if p < fixedp else torch.from_numpy(LO.exp_matrix(1, dx_ref[p - fixedp].numpy())) @ G[p]
        np.testing.assert_allclose(Mnew[p].numpy(), ref.numpy(), atol=5e-4)
    assert dx_ref.abs().max() > 1e-3


@functools.lru_cache(maxsize=None)
def _proj_trans_ref(name):
    poses, disps, intr, ii, jj, tgt, wgt, eta = SC.case_scene(name)
    return BO.proj_trans_dense(torch.from_numpy(tgt), torch.from_numpy(wgt), poses, torch.from_numpy(disps), intr, ii, jj)


@pytest.mark.parametrize("name", ["two_blocks", "sparse_sources"])
def test_proj_trans_on_two_pixel_blocks_and_sparse_sources(name):
    """the proj_trans half of test_proj_trans_and_bi_inter_match_their_restatements (same oracle, same tolerances): C, w [M, HW] by source slot"""
    poses, disps, intr, ii, jj, tgt, wgt, eta = SC.case_scene(name)
    C_ref, w_ref, kx = _proj_trans_ref(name)
    Cm, w = db.proj_trans(_f(poses), _f(disps), _f(intr[0]), _f(tgt)[None], _f(wgt)[None], torch.from_numpy(ii), torch.from_numpy(jj))
    torch.cuda.synchronize()
    assert Cm.shape == C_ref.shape == (len(kx), disps.shape[1] * disps.shape[2])
    np.testing.assert_allclose(Cm.cpu().numpy(), C_ref.numpy(), rtol=2e-3, atol=1e-6 * float(C_ref.abs().max()) + 1e-9)
    np.testing.assert_allclose(w.cpu().numpy(), w_ref.numpy(), rtol=2e-3, atol=2e-3 * float(w_ref.abs().max()))


@pytest.mark.parametrize("name", ["two_blocks", "sparse_sources"])
def test_jdsa_on_two_pixel_blocks_and_sparse_sources(name):
    """test_jdsa_matches_unreduced_dense_solve (same oracle, same tolerances) with HW = 323 -- jdsa_blocks_kernel's p += 256 loop runs twice
    -- and with prior / scales / disparities gathered by kx = [1, 3, 4]"""
    P, ht, wd, seed, fixedp, kw = SC.CASES[name]
    hs, ws, alpha = 2, 3, 0.05
    poses, disps, intr, ii, jj, tgt, wgt, eta = SC.case_scene(name)
    g = np.random.default_rng(2)
    prior = disps * g.uniform(0.8, 1.2, disps.shape)
    prior[:, :2, :3] = 0.0                                          # pixels without a prior fall back to eta
    prior[:, -1, -4:] = 0.0                                         # ... in the second pixel block too
    scales = g.uniform(0.9, 1.1, (P, hs, ws))
    C_ref, w_ref, kx = _proj_trans_ref(name)
    dz_ref, dso_ref = BO.jdsa_dense(C_ref, w_ref, torch.from_numpy(eta), torch.from_numpy(disps[kx]), torch.from_numpy(prior[kx]),
                                    torch.from_numpy(scales[kx]), alpha)
    dsc = _f(scales).clone()
    args = _ba_args(SC.case_scene(name))
    new_disps, new_scales, dzcov = B.JDSA(*args[:6], _f(prior), dsc, args[6], args[7], alpha)
    torch.cuda.synchronize()
    ref_d = torch.from_numpy(disps).clone()
    ref_d[torch.from_numpy(kx)] += dz_ref.reshape(-1, ht, wd)
    ref_d = torch.where(ref_d > 10, torch.zeros_like(ref_d), ref_d).clamp(min=0.001)
    sz, ss = float(dz_ref.abs().max()), float(dso_ref.abs().max())
    assert sz > 1e-4 and ss > 1e-4
    np.testing.assert_allclose(new_disps[0].cpu().numpy(), ref_d.numpy(), atol=1e-2 * sz + 1e-6)
    moved = new_scales.cpu().double() - torch.from_numpy(scales)
    np.testing.assert_allclose(moved[torch.from_numpy(kx)].reshape(len(kx), -1).numpy(), dso_ref.numpy(), atol=1e-2 * ss + 1e-6)
    rest = torch.from_numpy(np.setdiff1d(np.arange(P), kx))
    assert torch.equal(new_scales.cpu()[rest], torch.from_numpy(scales).float()[rest])         # scale grids of non-sources stay
    assert dzcov.shape == (len(kx), ht * wd) and bool((dzcov > 0).all())


@pytest.mark.parametrize("name", ["two_blocks", "sparse_sources"])
def test_edge_sharded_ba_sums_to_the_full_system_on_two_blocks_and_an_uneven_split(name):
    """test_edge_sharded_ba_sums_to_the_full_system (same assertions, same tolerances) with two ranks on HW = 323; the sparse scene deals its
    M = 3 sources [1, 3, 4] as two and one"""
    fixedp = SC.CASES[name][4]
    ii = SC.case_scene(name)[3]
    args = _ba_args(SC.case_scene(name))
    p_full, d_full, info = B.BA(*args, fixedp=fixedp)
    masks = [B.shard_edges_by_source(torch.from_numpy(ii), 2, r) for r in range(2)]
    assert bool((masks[0] ^ masks[1]).all()) and set(ii[masks[0].numpy()]).isdisjoint(set(ii[masks[1].numpy()]))
    if name == "sparse_sources":
        assert sorted(len(set(ii[m.numpy()])) for m in masks) == [1, 2]
    parts = [B.BA(*args, fixedp=fixedp, edge_mask=m) for m in masks]
    S = parts[0][2]["S"] + parts[1][2]["S"]
    vS = parts[0][2]["vS"] + parts[1][2]["vS"]
    torch.cuda.synchronize()
    sc = float(info["S"].abs().max())
    np.testing.assert_allclose(S.cpu().numpy(), info["S"].cpu().numpy(), atol=2e-5 * sc)
    np.testing.assert_allclose(vS.cpu().numpy(), info["vS"].cpu().numpy(), atol=2e-5 * float(info["vS"].abs().max()))


# ------------------------------------------------------------------------------------------------ 3. the Cholesky alone
def _solve_inputs(n):
    g = torch.Generator().manual_seed(100 + n)
    A = torch.randn(n, n, generator=g, dtype=torch.float64)
    S = (A @ A.T / n + torch.eye(n, dtype=torch.float64)).float()   # well conditioned by construction
    vS = torch.randn(n, generator=g, dtype=torch.float64).float()
    return S.contiguous(), vS.contiguous(), torch.diagonal(S).clone().contiguous()


def _call_solve(S, vS, hd, n, ep=0.1, lm=1e-4, rows=None):
    """cut3r_ba_solve through the C ABI with the test's own buffers; dx (max(rows, n, 1) floats) and flag start from sentinels"""
    rows = max(n, 1) if rows is None else rows
    dx = torch.full((rows,), float("nan"), device=DEV)
    flag = torch.full((1,), FLAG_SENTINEL, dtype=torch.int32, device=DEV)
    scratch = torch.empty(max(rows * rows, 1), device=DEV)
    rc = _lib.load().cut3r_ba_solve(_p(S), _p(vS), _p(hd), n, ep, lm, _p(scratch), _p(dx), _p(flag), _stream())
    torch.cuda.synchronize()
    return rc, dx.cpu(), int(flag.item())


@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 64, 65, 72, 127, 128, 129, 185, 192])
def test_chol_solve_alone_matches_fp64_cholesky(n):
    """cut3r_ba_solve (damping + in-LDS Cholesky + two triangular solves, one thread per row) on S = A A^T / n + I against fp64 torch from the
    same float32 inputs.  Bound: max(8 e32, 2e-6) with e32 the error of torch's float32 cholesky / cholesky_solve on the CPU on the same
    inputs (the 8 covers another equally stable summation order -- panels of 8 with fma -- not a wrong entry); both numbers are printed."""
    S, vS, hd = _solve_inputs(n)
    ep, lm = 0.1, 1e-4
    Sd = S.double() + torch.diag(ep + lm * hd.double())
    ref = torch.cholesky_solve(vS.double()[:, None], torch.linalg.cholesky(Sd))[:, 0]
    Sd32 = S + torch.diag(ep + lm * hd)
    x32 = torch.cholesky_solve(vS[:, None], torch.linalg.cholesky(Sd32))[:, 0]
    e32 = float((x32.double() - ref).abs().max() / ref.abs().max())
    rc, dx, flag = _call_solve(S.to(DEV), vS.to(DEV), hd.to(DEV), n)
    assert rc == 0 and flag == 0
    err = float((dx.double() - ref).abs().max() / ref.abs().max())
    print(f"[cut3r_ba_solve n = {n}] CPU float32 e32 = {e32:.2e}, kernel {err:.2e}, bound {max(8 * e32, 2e-6):.2e}")
    assert err <= max(8 * e32, 2e-6), (n, err, e32)


@pytest.mark.parametrize("row", [3, 70, 150])
def test_chol_solve_alone_fails_cleanly_on_a_bad_pivot_in_each_wave(row):
    """a diagonal entry of -1 (damped: about -0.9) in the first, second and third wave of rows: flag = 1 and dx exactly zero"""
    n = 185
    S, vS, hd = _solve_inputs(n)
    S[row, row] = -1.0
    hd = torch.diagonal(S).clone().contiguous()
    rc, dx, flag = _call_solve(S.to(DEV), vS.to(DEV), hd.to(DEV), n)
    assert rc == 0 and flag == 1
    assert dx.shape == (n,) and bool((dx == 0).all())


@pytest.mark.parametrize("n", [193, 0])
def test_chol_solve_alone_refuses_sizes_outside_its_range(n):
    S, vS, hd = _solve_inputs(193)
    rc, dx, flag = _call_solve(S.to(DEV), vS.to(DEV), hd.to(DEV), n, rows=193)
    assert rc == 1 and flag == FLAG_SENTINEL and bool(torch.isnan(dx).all())       # refused, nothing written


def _rel(got, want):
    return float((got.cpu().double() - want.double()).abs().max() / want.double().abs().max())


@pytest.mark.parametrize("M,D,HW", [(11, 6, 40), (13, 5, 21), (32, 6, 9), (33, 6, 9)])
def test_schur_solve_mono_prior_in_other_waves_and_ragged_chunks(M, D, HW):
    """schur_solve_mono_prior(dzcov=True) at n = M D = 66, 65, 192 (Cholesky rows in a second and third wave, n no multiple of 8 or 16) and
    cols = M HW = 440, 273, 288 (two mp_backsub workgroups, a ragged last 64-column chunk in mp_reduce), and at n = 198 the dense-tensor
    fallback, against the fp64 restatement of geom/chol.py:80-107 (tests/ba_scenes.mono_prior_ref).  Bound per output: the larger of the
    2e-4 of test_schur_solve_mono_prior_matches_fp64_restatement_including_the_covariance and 8 x the error of the same restatement
    evaluated in float32 on the CPU; both numbers are printed."""
    inputs = SC.mono_prior_inputs(M, D, HW, seed=M, ridge=None)
    want = SC.mono_prior_ref(*inputs)
    cpu32 = SC.mono_prior_ref(*(t.float() for t in inputs))
    assert (M * D > B.CHOL_MAXN) == (M == 33)
    got = B.schur_solve_mono_prior(*(t.float().to(DEV) for t in inputs), dzcov=True)
    torch.cuda.synchronize()
    for g_, w_, c_, nm in zip(got, want, cpu32, ("dso", "dz", "dzcov")):
        assert g_.shape == w_.shape
        e32, err = _rel(c_, w_), _rel(g_, w_)
        print(f"[schur_solve_mono_prior M = {M}, D = {D}, HW = {HW}] {nm}: CPU float32 {e32:.2e}, GPU {err:.2e}, bound {max(2e-4, 8 * e32):.2e}")
        assert err <= max(2e-4, 8 * e32), (nm, err, e32)


# ------------------------------------------------------------------------------------------------ 4. cut3r_ba_step in a guarded workspace
GUARD = 256                                   # floats on each side of the workspace
GUARD_BITS = 0x7FC0BEEF                       # a quiet NaN with a payload nothing computes
FLAG_SENTINEL = -12345


def _call_ba_step(scene, fixedp, ep=0.1, lm=1e-4, n_out=None):
    """cut3r_ba_step through the C ABI: index tables from ba._prepare, the workspace a slice of a larger tensor with GUARD floats on each side;
    guards, workspace, dx and dz start as GUARD_BITS.  Returns (rc, the whole tensor, workspace floats, dx, dz, flag)."""
    lib = _lib.load()
    args = _ba_args(scene)
    c = B._prepare(*args, fixedp)
    P, ht, wd, N, M = c["P"], c["ht"], c["wd"], c["N"], c["M"]
    nws = int(lib.cut3r_ba_workspace_floats(P, ht, wd, N, M, fixedp))
    fill = lambda k: torch.full((k,), GUARD_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    big = fill(GUARD + nws + GUARD)
    ws = big[GUARD:GUARD + nws]
    dx, dz = fill((P - fixedp) * 6 if n_out is None else n_out), fill(M * c["HW"])
    flag = torch.full((1,), FLAG_SENTINEL, dtype=torch.int32, device=DEV)
    rc = lib.cut3r_ba_step(_p(c["Gij"]), _p(c["dsp"]), _p(c["intr"]), _p(c["tgt"]), _p(c["wgt"]), _p(c["eta"]), _p(c["ii"]), _p(c["jj"]),
                           _p(c["src_ptr"]), _p(c["order"]), _p(c["kx_d"]), _p(c["present"]), P, ht, wd, N, M, fixedp, ep, lm, _p(ws), _p(dx),
                           _p(dz), _p(flag), _stream())
    return rc, big, nws, dx, dz, flag


@pytest.mark.parametrize("name", ["two_blocks", "sparse_sources", "two_waves", "limit_33"])
def test_ba_step_entry_point_stays_inside_its_workspace_and_equals_the_staged_step(name):
    """cut3r_ba_step, the one-GPU composition of assemble / solve / backsub, with the workspace sized by cut3r_ba_workspace_floats and 256
    guard floats on each side (more than the 128 floats by which the entry point used to overrun at n = 192: it kept diag(H) in the first n
    floats of a region reserved as n^2 + 64 and damped into the n^2 floats behind it, so for n > 64 the last n - 64 damped entries landed
    behind the workspace).  Both guards keep their bits; dx, dz and flag equal ba.BA's bit for bit (same kernels in the same order, all
    reductions in fixed order); and the step agrees with the oracle as in the tests above."""
    P, ht, wd, seed, fixedp, kw = SC.CASES[name]
    rc, big, nws, dx, dz, flag = _call_ba_step(SC.case_scene(name), fixedp)
    torch.cuda.synchronize()
    assert rc == 0
    bits = big.view(torch.int32).cpu()
    assert bool((bits[:GUARD] == GUARD_BITS).all()), "cut3r_ba_step wrote in front of its workspace"
    over = (bits[GUARD + nws:] != GUARD_BITS).nonzero().reshape(-1)
    assert over.numel() == 0, f"cut3r_ba_step wrote {int(over.max()) + 1} floats behind its workspace (n = {6 * (P - fixedp)})"
    Mnew, nd, dx_ba, dz_ba, failed = _ba(name)
    assert int(flag.item()) == failed == 0
    M = dz_ba.shape[0]
    assert torch.equal(dx.cpu().view(torch.int32), dx_ba.reshape(-1).view(torch.int32))
    assert torch.equal(dz.cpu().view(torch.int32), dz_ba.reshape(-1).view(torch.int32))
    _check_step(name, dx.reshape(P - fixedp, 6), dz.reshape(M, ht * wd))
