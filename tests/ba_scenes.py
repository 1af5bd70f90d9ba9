"""TEST INFRASTRUCTURE ONLY -- the synthetic dense-BA scenes of tests/test_ba_gpu.py, tests/test_ba_shapes_gpu.py and
tests/test_ba_scenes_cpu.py, the named cases of the shape tests with their fp64 references (oracle/ba_oracle.py, computed once per
process and shared), and the fp64 restatement of geom/chol.py:80-107 that the mono-prior solve is compared with."""
import functools

import numpy as np
import torch

from oracle import ba_oracle as BO
from oracle import lie_oracle as LO


def scene(P, ht, wd, seed, step=None, edges=None, back=None, patch=None):
    """P frames moving sideways, inverse depths ~ 0.4, targets = the projections under perturbed geometry + noise.
    step: x-baseline per frame (default 0.6 / (P - 1));  edges: explicit list of (i, j) (default: every |i - j| <= 2, both directions);
    back: a frame whose pose tangent gets -0.3 added in z;  patch = (frame, y0, y1, x0, x1): disparities there are drawn from U(3.5, 5.0).
    With the defaults the random stream, and so every array, is the one the suite has always used."""
    g = np.random.default_rng(seed)
    fx = fy = 0.8 * wd
    intr = np.tile(np.array([fx, fy, wd / 2 - 0.5, ht / 2 - 0.5]), (P, 1))
    # world->camera poses near identity, moving sideways; inverse depths ~ 0.4
    tang = np.zeros((P, 6))
    tang[:, 0] = (np.linspace(0, 0.6, P) if step is None else step * np.arange(P)) + g.normal(0, 0.02, P)
    tang[:, 1:3] = g.normal(0, 0.03, (P, 2))
    tang[:, 3:] = g.normal(0, 0.03, (P, 3))
    if back is not None:
        tang[back, 2] += -0.3
    poses = np.stack([LO.matrix_to_data(1, LO.exp_matrix(1, a)) for a in tang])
    disps = g.uniform(0.3, 0.6, (P, ht, wd))
    if patch is not None:
        f, y0, y1, x0, x1 = patch
        disps[f, y0:y1, x0:x1] = g.uniform(3.5, 5.0, (y1 - y0, x1 - x0))
    ii, jj = [], []
    if edges is None:
        for i in range(P):
            for j in range(P):
                if i != j and abs(i - j) <= 2:
                    ii.append(i); jj.append(j)
    else:
        for i, j in edges:
            ii.append(i); jj.append(j)
    ii, jj = np.array(ii), np.array(jj)
    N = len(ii)
    # targets: the true projections under perturbed geometry (so the residual is small but non-zero)
    G = BO.se3_matrix(poses)
    tgt = np.zeros((N, ht, wd, 2))
    for e in range(N):
        c, _ = BO.project(G[jj[e]] @ torch.linalg.inv(G[ii[e]]), torch.from_numpy(disps[ii[e]] * 1.05), intr[ii[e]], intr[jj[e]], ht, wd)
        tgt[e] = c.reshape(ht, wd, 2).numpy() + g.normal(0, 0.3, (ht, wd, 2))
    wgt = g.uniform(0.2, 1.0, (N, ht, wd, 2))
    eta = g.uniform(1e-3, 1e-2, (len(np.unique(ii)), ht, wd))
    return poses, disps, intr, ii, jj, tgt, wgt, eta


SPARSE_EDGES = [(1, 0), (1, 2), (3, 2), (3, 4), (4, 2), (4, 3), (1, 3), (3, 1), (4, 0), (3, 2)]

# name -> (P, ht, wd, seed, fixedp, scene keywords).  n = 6 (P - fixedp) rows in the Cholesky, HW = ht * wd pixels in blocks of 256.
# The seed is P, as in test_ba_step_matches_unreduced_dense_solve, unless the case states its own.
CASES = {
    "two_blocks": (4, 17, 19, 4, 1, {}),                                   # HW = 323: block 1 holds 67 pixels = one full wave + 3 lanes
    "three_blocks": (5, 23, 29, 5, 2, {}),                                 # HW = 667
    "block_exact": (4, 16, 16, 4, 1, {}),                                  # HW = 256 exactly
    "block_plus_two": (4, 3, 86, 4, 1, {}),                                # HW = 258: two pixels in block 1
    "sparse_sources": (5, 17, 19, 5, 1, dict(step=0.15, edges=SPARSE_EDGES)),
    "masked": (4, 17, 19, 4, 1, dict(step=0.15, back=2, patch=(1, 3, 9, 4, 12))),
    "free_gauge": (4, 6, 8, 4, 0, {}),
    "two_waves": (13, 6, 8, 13, 1, dict(step=0.15)),                       # n = 72
    "three_waves": (23, 4, 6, 23, 1, {}),                                  # n = 132
    "limit_33": (33, 4, 6, 33, 1, {}),                                     # n = 192
    "limit_34": (34, 4, 6, 34, 2, {}),                                     # n = 192, two fixed poses
}
BEYOND = (34, 4, 6, 34, 1, {})                                             # n = 198: refused


@functools.lru_cache(maxsize=None)
def case_scene(name):
    P, ht, wd, seed, fixedp, kw = CASES[name]
    return scene(P, ht, wd, seed, **kw)


@functools.lru_cache(maxsize=None)
def case_reference(name, system=False):
    """(dx_ref, dz_ref, kx[, H, g]) of BO.ba_dense for a named case; read-only for the tests that share it"""
    P, ht, wd, seed, fixedp, kw = CASES[name]
    poses, disps, intr, ii, jj, tgt, wgt, eta = case_scene(name)
    return BO.ba_dense(torch.from_numpy(tgt), torch.from_numpy(wgt), torch.from_numpy(eta), poses, torch.from_numpy(disps), intr, ii, jj,
                       fixedp, return_system=system)


def edge_depths(poses, disps, intr, ii, jj):
    """Z of every (edge, pixel) pair in the target camera, fp64: [N, HW] -- what the depth mask of ba_edge_kernel looks at"""
    P, ht, wd = disps.shape
    G = BO.se3_matrix(poses)
    y, x = torch.meshgrid(torch.arange(ht, dtype=BO.DT), torch.arange(wd, dtype=BO.DT), indexing="ij")
    out = []
    for e in range(len(ii)):
        fx, fy, cx, cy = [float(v) for v in intr[ii[e]]]
        X0 = torch.stack([(x - cx) / fx, (y - cy) / fy, torch.ones_like(x), torch.from_numpy(disps[ii[e]])], -1).reshape(-1, 4)
        out.append((X0 @ (G[jj[e]] @ torch.linalg.inv(G[ii[e]])).T)[:, 2])
    return torch.stack(out)


def mono_prior_ref(C, w, Hs, Es, vs, ep=0.1, lm=1e-4):
    """geom/chol.py:80-107 in plain torch, in the dtype of its arguments: C, w [1,M,HW]; Hs [1,M,M,D,D]; Es [1,M,M,D,HW]; vs [1,M,D]
    -> (dso [1,M,D], dz [1,M,HW], dzcov [M,HW])"""
    D = Hs.shape[-1]
    _, M, HW = C.shape
    Q = (1.0 / C).view(1, M * HW, 1)
    wv = w.reshape(1, M * HW, 1)
    H = Hs.permute(0, 1, 3, 2, 4).reshape(1, M * D, M * D)
    E = Es.permute(0, 1, 3, 2, 4).reshape(1, M * D, M * HW)
    v = vs.reshape(1, M * D, 1)
    H = H + (ep + lm * H) * torch.eye(M * D, dtype=H.dtype)
    Et = E.transpose(1, 2)
    S = H - E @ (Q * Et)
    v = v - E @ (Q * wv)
    L = torch.linalg.cholesky(S)
    dso = torch.cholesky_solve(v, L)
    dz = Q * (wv - Et @ dso)
    Fm = torch.linalg.solve_triangular(L, E * Q[..., 0][:, None], upper=False)
    cov = (Fm ** 2).sum(1) + Q[..., 0]
    return dso.reshape(1, M, D), dz.reshape(1, M, HW), cov.reshape(M, HW)


def mono_prior_inputs(M, D, HW, seed, ridge=4.0):
    """a general (not block diagonal) mono-prior system in fp64: H = A A^T + ridge I.  ridge = None: 4 + the largest eigenvalue of
    E C^-1 E^T, so that the reduced system S = H + damping - E C^-1 E^T is positive definite at every size (with the fixed 4.0 it is
    only while M * HW stays small: the eigenvalues of E C^-1 E^T grow with the number of columns)"""
    g = torch.Generator().manual_seed(seed)
    Es = torch.randn(1, M, M, D, HW, generator=g, dtype=torch.float64) * 0.3
    A = torch.randn(M * D, M * D, generator=g, dtype=torch.float64)
    vs = torch.randn(1, M, D, generator=g, dtype=torch.float64)
    C = torch.rand(1, M, HW, generator=g, dtype=torch.float64) * 2 + 6.0
    w = torch.randn(1, M, HW, generator=g, dtype=torch.float64)
    if ridge is None:
        E = Es.permute(0, 1, 3, 2, 4).reshape(M * D, M * HW)
        ridge = 4.0 + float(torch.linalg.eigvalsh((E / C.reshape(1, -1)) @ E.T)[-1])
    Hfull = A @ A.T + ridge * torch.eye(M * D, dtype=torch.float64)
    Hs = Hfull.reshape(M, D, M, D).permute(0, 2, 1, 3)[None].contiguous()
    return C, w, Hs, Es, vs
