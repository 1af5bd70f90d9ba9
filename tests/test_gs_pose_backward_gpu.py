"""cut3r_gs_pose_backward (csrc/gs.hip): the backward pass of a pose-only iteration against a frozen map, dgeom -> the 16 pose sums
M (9) | s (3) | r (4) of csrc/gs_train.hip's header in one kernel + a fixed-order finish, against the chain it replaces
(cut3r_gs_preprocess_backward + cut3r_gs_activate_backward with gtheta = NULL) and an fp64 summation of that chain's per-Gaussian terms.

Scene: a 32 x 48 image, random Gaussians in front of the camera with some behind it or far off-screen (culled), a non-identity pose with a
non-zero increment, random cotangents on every output image through the existing forward and cut3r_gs_render_backward."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pytestmark = pytest.mark.gpu

from cut3r_slam_amd import _lib  # noqa: E402
from cut3r_slam_amd import gaussian_rasterizer as GR  # noqa: E402
from cut3r_slam_amd import gs_mapper as GM  # noqa: E402
from oracle import gs_oracle as GO  # noqa: E402

DEV = "cuda:0"
H, W, FX, FY, CX, CY = 32, 48, 40.0, 40.0, 24.0, 16.0
SIZES = (1, 63, 64, 65, 256, 257, 1000)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _arr(vals):
    return (C.c_float * len(vals))(*[float(v) for v in vals])


IDENTITY16 = _arr([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1])


def _camera():
    return GM.Camera(0, torch.zeros(3, H, W), torch.zeros(H, W), torch.eye(4), FX, FY, CX, CY, device=DEV)


def _pose_state():
    """world->camera (t, q_xyzw) away from the identity, and a non-zero increment (tau, phi)"""
    ps = torch.zeros(32)
    q = torch.tensor([0.03, -0.02, 0.015, 1.0])
    ps[0:3] = torch.tensor([0.08, -0.05, 0.1])
    ps[3:7] = q / q.norm()
    ps[7:13] = torch.tensor([0.01, -0.008, 0.006, 0.004, -0.005, 0.003])
    return ps.to(DEV)


def _theta(P, all_culled=False):
    g = torch.Generator().manual_seed(100 + P)
    th = torch.zeros(P, 14)
    th[:, 0:3] = torch.randn(P, 3, generator=g) * torch.tensor([0.8, 0.5, 0.4]) + torch.tensor([0.0, 0.0, 3.0])
    idx = torch.arange(P)
    th[idx % 7 == 3, 2] = -1.0                                             # behind the camera
    th[idx % 11 == 5, 0] = 40.0                                            # far off-screen
    if all_culled:
        th[:, 2] = -1.0 - torch.rand(P, generator=g)
    th[:, 3:6] = torch.randn(P, 3, generator=g)
    th[:, 6] = torch.randn(P, generator=g)
    th[:, 7:10] = torch.log(torch.rand(P, 3, generator=g) * 0.22 + 0.03)
    th[:, 10:14] = torch.randn(P, 4, generator=g)                          # not normalised: the activation normalises
    return th.to(DEV).contiguous()


def _activate(theta, ps):
    lib, P = _lib.load(), theta.shape[0]
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=DEV)
    a = {"means": f(P, 3), "scales": f(P, 3), "rots": f(P, 4), "opac": f(P), "shs": f(P, 1, 3)}
    assert lib.cut3r_gs_activate(P, _p(theta), _p(ps), _p(a["means"]), _p(a["scales"]), _p(a["rots"]), _p(a["opac"]), _p(a["shs"]), None) == 0
    return a


def _settings(cam):
    return GR.GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
                                            kernel_size=0.0, bg=torch.zeros(3), scale_modifier=1.0, viewmatrix=torch.eye(4),
                                            projmatrix=cam.projection_matrix_host, sh_degree=0, campos=torch.zeros(3), prefiltered=False,
                                            require_coord=True, require_depth=True, debug=False)


def _pose_backward(P, a, cam, geom, dgeom, theta, ps, partials, sums):
    st = _settings(cam)
    return _lib.load().cut3r_gs_pose_backward(P, _p(a["means"]), _p(a["scales"]), _p(a["rots"]), _p(a["opac"]), IDENTITY16,
                                              _arr(cam.projection_matrix_host.reshape(-1).tolist()), W, H, st.tanfovx, st.tanfovy, 0.0, 1.0,
                                              _p(geom), _p(dgeom), _p(theta), _p(ps), _p(partials), _p(sums), None)


_CASES = {}


def _case(P):
    """forward, render backward, the chain and the new kernel for P Gaussians -- computed once per size, shared and left unchanged"""
    if P in _CASES:
        return _CASES[P]
    lib = _lib.load()
    cam, ps, theta = _camera(), _pose_state(), _theta(P)
    a = _activate(theta, ps)
    st = _settings(cam)
    out, radii, buf = GR._forward(a["means"], a["shs"], None, a["opac"], a["scales"], a["rots"], st)
    g = torch.Generator().manual_seed(7)
    cot = [torch.randn(c, H, W, generator=g).to(DEV) for c in (3, 3, 3, 1, 1, 1, 3)]
    dgeom = torch.empty(P, GR.GS_REC, device=DEV)
    bg = _arr([0, 0, 0])
    assert lib.cut3r_gs_render_backward(_p(buf.ranges), _p(buf.point_list), _p(buf.geom), P, W, H, st.tanfovx, st.tanfovy, bg, _p(buf.n_contrib),
                                        _p(buf.aux), _p(buf.alpha), _p(buf.coord), _p(buf.depth), _p(buf.normal), *[_p(t) for t in cot],
                                        _p(dgeom), None) == 0
    z = lambda *s: torch.zeros(*s, device=DEV)
    d = {"means": z(P, 3), "scales": z(P, 3), "rots": z(P, 4), "opac": z(P), "shs": z(P, 1, 3), "means2D": z(P, 3)}
    proj = _arr(cam.projection_matrix_host.reshape(-1).tolist())
    assert lib.cut3r_gs_preprocess_backward(P, _p(a["means"]), _p(a["scales"]), _p(a["rots"]), _p(a["opac"]), _p(a["shs"]), 0, 1, IDENTITY16, proj,
                                            _arr([0, 0, 0]), W, H, st.tanfovx, st.tanfovy, 0.0, 1.0, _p(buf.geom), _p(dgeom), _p(d["means"]),
                                            _p(d["scales"]), _p(d["rots"]), _p(d["opac"]), _p(d["shs"]), None, _p(d["means2D"]), None) == 0
    chain = z(16)
    assert lib.cut3r_gs_activate_backward(P, _p(theta), _p(ps), _p(d["means"]), _p(d["scales"]), _p(d["rots"]), _p(d["opac"]), _p(d["shs"]),
                                          _p(radii), 0.0, None, None, _p(chain), None) == 0
    rows = int(lib.cut3r_gs_pose_partial_rows(P))
    partials = torch.full((rows, 16), float("nan"), device=DEV)
    sums = torch.full((16,), float("nan"), device=DEV)                     # pre-filled: the kernel must WRITE, not accumulate
    assert _pose_backward(P, a, cam, buf.geom, dgeom, theta, ps, partials, sums) == 0
    torch.cuda.synchronize()
    _CASES[P] = dict(cam=cam, ps=ps, theta=theta, a=a, st=st, buf=buf, radii=radii, dgeom=dgeom, d=d, chain=chain, rows=rows, partials=partials,
                     sums=sums)
    return _CASES[P]


def _qmul(a, b):
    """Hamilton product of (x, y, z, w) quaternions, the formula of csrc/lie_math.h"""
    ax, ay, az, aw = a.unbind(-1)
    bx, by, bz, bw = b.unbind(-1)
    return torch.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                        aw * bw - ax * bx - ay * by - az * bz], -1)


def _qrot(q, v):
    """v + 2 w (u x v) + 2 u x (u x v), the formula of csrc/lie_math.h (q as stored: its norm is 1 only to fp32 rounding)"""
    u = q[..., :3].expand_as(v)
    uv = torch.cross(u, v, dim=-1)
    return v + 2 * q[..., 3:] * uv + 2 * torch.cross(u, uv, dim=-1)


def _terms64(c):
    """[P,16] fp64: every Gaussian's contribution to the 16 sums from the chain's per-Gaussian d_means / d_rots (the header of
    csrc/gs_train.hip: M = sum g y^T, s = sum g, r = sum g^q * conj(q_T * q_g))"""
    th, ps = c["theta"].double().cpu(), c["ps"].double().cpu()
    g, gr = c["d"]["means"].double().cpu(), c["d"]["rots"].double().cpu()
    tT, qT = ps[0:3], ps[3:7]
    y = _qrot(qT[None], th[:, 0:3]) + tT
    M = (g[:, :, None] * y[:, None, :]).reshape(-1, 9)
    q = th[:, 10:14]
    q = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    gq = torch.cat([q[:, 1:], q[:, :1]], -1)                               # (r, x, y, z) -> (x, y, z, w)
    gc = torch.cat([gr[:, 1:], gr[:, :1]], -1)
    qc = _qmul(qT[None].expand_as(gq), gq)
    r = _qmul(gc, torch.cat([-qc[:, :3], qc[:, 3:]], -1))
    return torch.cat([M, g, r], -1)


@pytest.mark.parametrize("P", SIZES)
def test_pose_sums_are_within_the_fp32_summation_bound_of_the_fp64_sums(P):
    """|new_k - ref_k| <= n_vis * 2^-24 * sum_p |term_p,k| + 1e-30: the worst case of an fp32 summation of n_vis terms that each carry one
    rounding (the new entry point forms its terms in fp64 from per-Gaussian gradients that are, bit for bit, the chain's: both launch the
    same kernel).  Measured on an MI355X, max_k |new - fp64| / bound: 0.72 (P = 1), 0.012, 0.0083, 0.0095, 0.0023, 0.0019, 0.00034 (P = 1000);
    the chain's own fp32 terms: 2.9 at P = 1, then 0.020 ... 0.00034"""
    c = _case(P)
    n_vis = int((c["radii"] > 0).sum())
    if P > 1:
        assert 0 < n_vis < P, (P, n_vis)                                   # culling occurs
    else:
        assert n_vis == 1
    t = _terms64(c)
    ref, mag = t.sum(0), t.abs().sum(0)
    bound = n_vis * 2.0 ** -24 * mag + 1e-30
    new, chain = c["sums"].double().cpu(), c["chain"].double().cpu()
    assert bool(torch.isfinite(new).all())                                  # (the NaN pre-fill was overwritten)
    r_new, r_chain = ((new - ref).abs() / bound).max(), ((chain - ref).abs() / bound).max()
    print(f"[gs pose bwd] P {P}: {n_vis} visible, max_k |new - fp64| / bound {float(r_new):.3e}, the chain's own {float(r_chain):.3e}, "
          f"max |sum| {float(ref.abs().max()):.3e}")
    assert float(mag.max()) > 0
    assert bool(((new - ref).abs() <= bound).all()), ((new - ref).abs() / bound).tolist()
    assert c["partials"].shape[0] == c["rows"] == (P + 255) // 256 and bool(torch.isfinite(c["partials"]).all())      # every row written


@pytest.mark.parametrize("P", (65, 1000))
def test_same_inputs_give_the_same_bits_and_the_output_is_overwritten(P):
    c = _case(P)
    partials = torch.full_like(c["partials"], float("nan"))
    sums = torch.full((16,), float("nan"), device=DEV)
    assert _pose_backward(P, c["a"], c["cam"], c["buf"].geom, c["dgeom"], c["theta"], c["ps"], partials, sums) == 0
    assert torch.equal(partials, c["partials"]) and torch.equal(sums, c["sums"])
    sums2 = torch.full((16,), 1e30, device=DEV)                            # written, not accumulated
    assert _pose_backward(P, c["a"], c["cam"], c["buf"].geom, c["dgeom"], c["theta"], c["ps"], partials, sums2) == 0
    assert torch.equal(sums2, c["sums"])


def test_culled_gaussians_contribute_exact_zeros():
    P = 300
    lib = _lib.load()
    cam, ps, theta = _camera(), _pose_state(), _theta(P, all_culled=True)
    a, st = _activate(theta, ps), _settings(cam)
    geom = torch.empty(P, GR.GS_REC, device=DEV)
    radii, tiles, offsets = (torch.empty(P, dtype=torch.int32, device=DEV) for _ in range(3))
    ws = torch.empty(GR.workspace_bytes(P, 0), dtype=torch.uint8, device=DEV)
    assert lib.cut3r_gs_preprocess(P, _p(a["means"]), _p(a["scales"]), _p(a["rots"]), _p(a["opac"]), _p(a["shs"]), 0, 1, None, IDENTITY16,
                                   _arr(cam.projection_matrix_host.reshape(-1).tolist()), _arr([0, 0, 0]), W, H, st.tanfovx, st.tanfovy, 0.0, 1.0,
                                   _p(geom), _p(radii), _p(tiles), _p(offsets), _p(ws), ws.numel(), None) == 0
    assert int((radii > 0).sum()) == 0
    dgeom = torch.randn(P, GR.GS_REC, device=DEV)                          # never read for a culled Gaussian
    partials = torch.full((int(lib.cut3r_gs_pose_partial_rows(P)), 16), float("nan"), device=DEV)
    sums = torch.full((16,), float("nan"), device=DEV)
    assert _pose_backward(P, a, cam, geom, dgeom, theta, ps, partials, sums) == 0
    assert torch.equal(sums, torch.zeros(16, device=DEV)) and torch.equal(partials, torch.zeros_like(partials))


def test_row_count_and_refused_arguments():
    lib = _lib.load()
    assert [int(lib.cut3r_gs_pose_partial_rows(p)) for p in (1, 256, 257, 1000)] == [1, 1, 2, 4]
    assert lib.cut3r_gs_pose_partial_rows(0) == -1 and lib.cut3r_gs_pose_partial_rows(-3) == -1
    c = _case(65)
    good = [c["a"]["means"], c["a"]["scales"], c["a"]["rots"], c["a"]["opac"], c["buf"].geom, c["dgeom"], c["theta"], c["ps"], torch.empty(1, 16, device=DEV),
            torch.empty(16, device=DEV)]
    proj = _arr(c["cam"].projection_matrix_host.reshape(-1).tolist())

    def call(P, t, view=IDENTITY16, pr=proj, w=W, h=H):
        return lib.cut3r_gs_pose_backward(P, _p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]), view, pr, w, h, c["st"].tanfovx, c["st"].tanfovy, 0.0, 1.0,
                                          _p(t[4]), _p(t[5]), _p(t[6]), _p(t[7]), _p(t[8]), _p(t[9]), None)
    assert call(0, good) == 1 and call(-1, good) == 1
    for k in range(len(good)):
        assert call(65, good[:k] + [None] + good[k + 1:]) == 1, k
    assert call(65, good, view=None) == 1 and call(65, good, pr=None) == 1 and call(65, good, w=0) == 1 and call(65, good, h=-2) == 1
    torch.cuda.synchronize()


def test_preprocess_backward_still_is_the_derivative_of_the_projection():
    """the kernel whose body moved into the shared function: d_means / d_scales / d_rots of three Gaussians against a central fp64 finite
    difference of the projection (oracle/gs_oracle.py preprocess) contracted with dgeom, within the tolerances tests/test_gs_gpu.py
    uses for this backward (2e-4 means and scales, 5e-4 rotations, of |ref| + mean |ref|)"""
    c = _case(65)
    dg = c["dgeom"].double().cpu()
    vis = (c["radii"] > 0).nonzero()[:, 0].cpu()
    pick = vis[[0, len(vis) // 2, len(vis) - 1]]
    st = {"image_height": H, "image_width": W, "tanfovx": c["st"].tanfovx, "tanfovy": c["st"].tanfovy, "kernel_size": 0.0, "scale_modifier": 1.0,
          "viewmatrix": torch.eye(4, dtype=torch.float64), "projmatrix": c["cam"].projection_matrix_host.double(), "sh_degree": 0,
          "campos": torch.zeros(3, dtype=torch.float64), "bg": torch.zeros(3, dtype=torch.float64)}
    x0 = torch.cat([c["a"]["means"], c["a"]["scales"], c["a"]["rots"]], 1).double().cpu()[pick]            # [3,10]
    op = c["a"]["opac"].double().cpu()[pick].reshape(-1, 1)
    dgp = dg[pick]

    def L(x):
        g = GO.preprocess(x[:, 0:3], op, x[:, 3:6], x[:, 6:10], None, torch.zeros(len(x), 3, dtype=torch.float64), st)
        f = torch.zeros(len(x), GR.GS_REC, dtype=torch.float64)
        f[:, 0:2], f[:, 3], f[:, 4:7], f[:, 7] = g["xy"], g["ts"], g["conic"], g["opacity"]
        f[:, 11:14], f[:, 14:20], f[:, 20:22], f[:, 22:25] = g["view_point"], g["camera_plane"], g["ray_plane"], g["normal"]
        w = dgp.clone()
        w[:, 2] = 0                                                        # (slot 2 carries the |d/dxy| statistic, not a gradient)
        w[:, 8:11] = 0                                                     # colour: no path to mean / scale / rotation at SH degree 0
        return (f * w).sum(1)
    ref = torch.zeros(3, 10, dtype=torch.float64)
    for k in range(10):
        h = 1e-6 * max(1.0, float(x0[:, k].abs().max()))
        e = torch.zeros(10, dtype=torch.float64)
        e[k] = h
        ref[:, k] = (L(x0 + e) - L(x0 - e)) / (2 * h)
    got = torch.cat([c["d"]["means"], c["d"]["scales"], c["d"]["rots"]], 1).double().cpu()[pick]
    for name, (a, b), tol in (("means", (0, 3), 2e-4), ("scales", (3, 6), 2e-4), ("rotations", (6, 10), 5e-4)):
        r, g = ref[:, a:b].numpy(), got[:, a:b].numpy()
        scale = np.abs(r).mean() + 1e-12
        err = np.abs(g - r)
        print(f"[gs pose bwd] preprocess_backward d {name}: mean |ref| {scale:.3e}, max |err| / (|ref| + scale) {(err / (np.abs(r) + scale)).max():.2e}")
        assert scale > 1e-9 and (err <= tol * (np.abs(r) + scale)).all(), name
