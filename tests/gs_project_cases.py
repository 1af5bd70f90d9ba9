"""The cases of tests/test_gs_project_cpu.py and tests/test_gs_project_gpu.py: the inputs of cut3r_gs_preprocess / _backward for five small
Gaussian sets.  Not collected by pytest.  Inputs are fp32 arrays (what the kernels read); the camera follows oracle/gs_oracle.py.

  one       P = 1,   50 x 37, identity view, kernel_size 0, scale_modifier 1, SH degree 0 stored with K = 16: the flat Gaussian whose thin
            axis is exactly perpendicular to its viewing ray (the `mlen` exit: planes and normal 0)
  sh65      P = 65,  50 x 37, identity view, kernel_size 0, scale_modifier 1.7, SH degree 1 stored with K = 16: what needs EXACT arithmetic
            (z = 0.2f itself: culled by `>`; the vbn floor at |e . ray| = 5e-8 and its neighbour at 2e-7) and the hand-built list
  hand65    P = 65,  64 x 48, a rotated and shifted view, kernel_size 0, scale_modifier 1, colours given (colors_precomp): the hand-built list
  hand257   P = 257, 50 x 37, another view, kernel_size 0.1, scale_modifier 1.7, SH degree 3, K = 16: the hand-built list
  scene300  P = 300, 64 x 48, the view of hand65, kernel_size 0.1, scale_modifier 1, SH degree 2 stored with K = 16: a random scene

The hand-built list (`hand_list`; positions and orientations are given in the CAMERA frame and carried to the world by the inverse view,
then rounded to fp32) puts one Gaussian clearly on each side of every branch; `expect` names, per Gaussian, the side it was built for
(tests/test_gs_project_cpu.py checks it against the reference, and that none of them is ambiguous).  The rest of every case is random."""
import math

import numpy as np

from tests.gs_render_oracle import F32, F64

CASES = {  # name: (P, H, W, view (rx, ry, rz, t), kernel_size, scale_modifier, sh degree or None: colours given, K, what it holds)
    "one": (1, 37, 50, None, 0.0, 1.0, 0, 16, ("mlen",)),
    "sh65": (65, 37, 50, None, 0.0, 1.7, 1, 16, ("exact", "list")),
    "hand65": (65, 48, 64, (0.15, -0.2, 0.1, (0.1, -0.05, 0.2)), 0.0, 1.0, None, 0, ("list",)),
    "hand257": (257, 37, 50, (-0.1, 0.25, -0.3, (-0.2, 0.1, 0.3)), 0.1, 1.7, 3, 16, ("list",)),
    "scene300": (300, 48, 64, (0.15, -0.2, 0.1, (0.1, -0.05, 0.2)), 0.1, 1.0, 2, 16, ()),
}
FOVX = 1.0
_CACHE = {}


def _w2c(view):
    M = np.eye(4)
    if view is None:
        return M
    rx, ry, rz, t = view
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    M[:3, :3] = (np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
                 @ np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]))
    M[:3, 3] = t
    return M


def _quat_of(R):
    """(r, x, y, z) of a rotation matrix with a positive trace-side (the small angles used here)"""
    r = 0.5 * math.sqrt(1.0 + R[0, 0] + R[1, 1] + R[2, 2])
    return np.array([r, (R[2, 1] - R[1, 2]) / (4 * r), (R[0, 2] - R[2, 0]) / (4 * r), (R[1, 0] - R[0, 1]) / (4 * r)])


def _qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def camera_of(name):
    """dict(W, H, tanx, tany, view [16], proj [16], campos [3], w2c): fp32 matrices as the host hands them over (transposed 4 x 4s)"""
    P, H, W, view = CASES[name][:4]
    from oracle import gs_oracle as GO
    import torch
    M = _w2c(view)
    st = GO.camera_settings(H, W, FOVX, FOVX * H / W, torch.from_numpy(M))
    f = lambda t: t.numpy().astype(F32).reshape(-1)
    Mi = np.linalg.inv(M)
    return dict(W=W, H=H, tanx=float(F32(st["tanfovx"])), tany=float(F32(st["tanfovy"])), view=f(st["viewmatrix"]), proj=f(st["projmatrix"]),
                campos=Mi[:3, 3].astype(F32), w2c=M)


def _u_of_pixel(px, n, tan):
    """x/z that projects to pixel coordinate px of n"""
    return ((2.0 * px + 1.0) / n - 1.0) * tan


def hand_list(cam, ks):
    """[(label, camera-frame point, scales, camera-frame quaternion, opacity, expectation)]: expectation {side name: value} on the reference's
    `side` / visible / rect, see tests/test_gs_project_cpu.py"""
    W, H, tx, ty = cam["W"], cam["H"], cam["tanx"], cam["tany"]
    rng = np.random.default_rng(11)
    qr = lambda: (lambda q: q / np.linalg.norm(q))(rng.normal(size=4))
    I4 = np.array([1.0, 0.0, 0.0, 0.0])
    at = lambda px, py, z=2.0: np.array([_u_of_pixel(px, W, tx) * z, _u_of_pixel(py, H, ty) * z, z])
    iso = lambda s: np.array([s, s, s])
    L = []
    add = lambda label, p, s, q, exp, op=0.6: L.append((label, np.asarray(p, dtype=F64), np.asarray(s, dtype=F64), np.asarray(q, dtype=F64), op, exp))
    add("z0.19", (0.01, 0.01, 0.19), iso(0.004), qr(), dict(in_front=False, visible=False))
    add("z0.21", (0.01, 0.01, 0.21), iso(0.004), qr(), dict(in_front=True, visible=True))
    add("x1.2", (1.2 * tx * 2.0, 0.1, 2.0), (0.35, 0.3, 0.25), qr(), dict(clamped=False, visible=True))
    add("x1.4", (1.4 * tx * 2.0, 0.1, 2.0), (0.35, 0.3, 0.25), qr(), dict(clamped=True, visible=True))
    add("y-1.2", (0.1, -1.2 * ty * 2.0, 2.0), (0.35, 0.3, 0.25), qr(), dict(clamped=False, visible=True))
    add("y-1.4", (0.1, -1.4 * ty * 2.0, 2.0), (0.35, 0.3, 0.25), qr(), dict(clamped=True, visible=True))
    # off screen to the left by a little less / more than the radius: set by `_place_at_edge` below (x pixel = 1 - radius +- 0.4)
    add("edge_in", at(-2.0, H / 2), iso(0.02), I4, dict(visible=True, edge=+0.4))
    add("edge_out", at(-2.0, H / 2), iso(0.02), I4, dict(visible=False, in_front=True, edge=-0.4))
    add("neg_xy", at(-0.3, -0.3), iso(0.03), qr(), dict(visible=True, rect0=(0, 0)))
    for k, (px, py) in enumerate(((0.2, 0.2), (W - 1.2, 0.3), (0.3, H - 1.2), (W - 0.8, H - 0.7))):
        add("corner%d" % k, at(px, py), iso(0.03), qr(), dict(visible=True))
    add("whole_grid", at(W / 2 + 0.3, H / 2 - 0.2), (1.5, 1.2, 1.0), qr(), dict(visible=True, full=True, radius_floored=False))
    add("thin5e-5", at(20.3, 12.1), (5e-5, 0.05, 0.06), qr(), dict(well=False, kmin=0, visible=True))
    add("thin2e-4", at(24.3, 12.1), (2e-4, 0.05, 0.06), qr(), dict(well=True, visible=True))
    add("pair01", at(28.3, 16.1), (5e-5, 5e-5, 0.01), qr(), dict(well=False, kmin=0, visible=True))
    add("pair02", at(30.3, 20.1), (5e-5, 0.01, 5e-5), qr(), dict(well=False, kmin=0, visible=True))
    add("pair12", at(32.3, 24.1), (0.01, 5e-5, 5e-5), qr(), dict(well=False, kmin=1, visible=True))
    add("thin_y", at(12.3, 24.1), (0.06, 4e-5, 0.05), qr(), dict(well=False, kmin=1, visible=True))
    add("thin_z", at(14.3, 28.1), (0.06, 0.05, 3e-5), qr(), dict(well=False, kmin=2, visible=True))
    if ks == 0.0:
        add("all0", at(16.3, 8.1), iso(0.0), qr(), dict(det_ok=False, visible=False, in_front=True))
    else:
        add("all0", at(16.3, 8.1), iso(0.0), qr(), dict(det_ok=True, visible=True, coef_zero=True))
    add("tiny", at(36.3, 8.1), iso(0.002), qr(), dict(radius_floored=True, visible=True))
    add("long", at(38.3, 28.1), (0.5, 0.04, 0.04), qr(), dict(radius_floored=False, visible=True))
    add("q0.7", at(10.3, 10.1), (0.08, 0.05, 0.03), 0.7 * qr(), dict(visible=True))
    add("q1.4", at(40.3, 20.1), (0.08, 0.05, 0.03), 1.4 * qr(), dict(visible=True))
    return L


def exact_list(cam):
    """identity view only: what needs exact arithmetic (camera frame = world frame)"""
    I4 = np.array([1.0, 0.0, 0.0, 0.0])
    z02 = float(F32(0.2))
    return [("z=0.2f", np.array([0.0, 0.0, z02]), np.array([0.004] * 3), I4, 0.6, dict(in_front=False, visible=False)),
            ("vbn5e-8", np.array([1e-7, 0.0, 2.0]), np.array([5e-5, 0.05, 0.05]), I4, 0.6, dict(well=False, kmin=0, bad=False, vbn_floored=True, visible=True)),
            ("vbn2e-7", np.array([4e-7, 0.0, 2.0]), np.array([5e-5, 0.05, 0.05]), I4, 0.6, dict(well=False, kmin=0, bad=False, vbn_floored=False, visible=True))]


def mlen_list(cam):
    return [("mlen0", np.array([0.0, 0.0, 2.0]), np.array([5e-5, 0.05, 0.05]), np.array([1.0, 0.0, 0.0, 0.0]), 0.6,
             dict(well=False, kmin=0, bad=True, visible=True))]


def _assemble(name, hand):
    P, H, W, view, ks, mod, deg, K, _ = CASES[name]
    cam = camera_of(name)
    rng = np.random.default_rng(P + 7 * H)
    M = cam["w2c"]
    Mi = np.linalg.inv(M)
    qc2w = _quat_of(Mi[:3, :3])
    means = rng.normal(size=(P, 3)) * 0.7 + np.array([0.0, 0.0, 3.0])
    means = means @ Mi[:3, :3].T + Mi[:3, 3]
    scales = rng.random((P, 3)) * 0.2 + 0.02
    rots = rng.normal(size=(P, 4))
    rots /= np.linalg.norm(rots, axis=1, keepdims=True)
    opac = rng.random((P, 1)) * 0.85 + 0.1
    slots = rng.permutation(P)[:len(hand)]
    labels, expect = {}, {}
    for i, (label, p, s, q, op, exp) in zip(slots, hand):
        means[i], scales[i], rots[i], opac[i] = Mi[:3, :3] @ p + Mi[:3, 3], s, _qmul(qc2w, q), op
        labels[label], expect[label] = int(i), exp
    case = dict(name=name, P=P, H=H, W=W, tanx=cam["tanx"], tany=cam["tany"], view=cam["view"], proj=cam["proj"], campos=cam["campos"], ks=ks, mod=mod,
                deg=deg if deg is not None else 0, K=K if deg is not None else 0, labels=labels, expect=expect,
                means=means.astype(F32), scales=scales.astype(F32), rots=rots.astype(F32), opac=opac.astype(F32))
    if deg is None:
        case["colors"], case["shs"] = rng.random((P, 3)).astype(F32), None
    else:
        shs = rng.normal(size=(P, K, 3)) * 0.3
        shs[:, 0] = rng.random((P, 3)) * 2.0 - 0.4
        for label in ("q0.7", "thin2e-4", "mlen0", "vbn2e-7"):                # channel 1 negative before the clamp, the other two positive
            if label in labels:
                shs[labels[label]] *= 0.05
                shs[labels[label], 0] = (1.0, -3.0, 0.5)
                expect[label] = dict(expect[label], clampbits=2)
        case["colors"], case["shs"] = None, shs.astype(F32)
    about = np.zeros(P, dtype=bool)
    about[list(labels.values())] = True
    case["about"] = about
    return case


def _place_at_edge(case):
    """moves edge_in / edge_out so that their x pixel is 1 - radius +- 0.4: x + radius + 15 is 16.4 (one tile) or 15.6 (none)"""
    from tests import gs_project_oracle as PO
    cam = camera_of(case["name"])
    Mi = np.linalg.inv(cam["w2c"])
    for label in ("edge_in", "edge_out"):
        if label not in case["labels"]:
            continue
        i, d = case["labels"][label], case["expect"][label]["edge"]
        for _ in range(3):
            one = dict(case, means=case["means"][i:i + 1], scales=case["scales"][i:i + 1], rots=case["rots"][i:i + 1], opac=case["opac"][i:i + 1],
                       shs=None if case["shs"] is None else case["shs"][i:i + 1], colors=None if case["colors"] is None else case["colors"][i:i + 1])
            with np.errstate(all="ignore"):
                cx = PO.Ctx(1, False)
                o = PO.project([cx.seed(one["means"][:, k], None) for k in range(3)], [cx.seed(one["scales"][:, k], None) for k in range(3)],
                               [cx.seed(one["rots"][:, k], None) for k in range(4)], PO._cam(one), cx)
            a, b, c = (float(t.v[0]) for t in o["cov"])
            mid = 0.5 * (a + c)
            rad = math.ceil(3.0 * math.sqrt(mid + math.sqrt(max(0.1, mid * mid - (a * c - b * b)))))
            p = np.array([_u_of_pixel(1.0 - rad + d, case["W"], cam["tanx"]) * 2.0, 0.0, 2.0])
            case["means"][i] = (Mi[:3, :3] @ p + Mi[:3, 3]).astype(F32)


def case(name):
    if name not in _CACHE:
        what = CASES[name][8]
        cam = camera_of(name)
        hand = []
        if "mlen" in what:
            hand += mlen_list(cam)
        if "exact" in what:
            hand += exact_list(cam)
        if "list" in what:
            hand += hand_list(cam, CASES[name][4])
        c = _assemble(name, hand)
        _place_at_edge(c)
        _CACHE[name] = c
    return _CACHE[name]


_REF = {}


def reference(name):
    """the forward and backward references of a case, computed once and left unchanged: `fwd`, the fp32 records `geom` the backward pass is
    fed, `dgeom` (random, zero for ambiguous Gaussians) and `bwd`"""
    if name not in _REF:
        from tests import gs_project_oracle as PO
        c = case(name)
        fwd = PO.forward_reference(c)
        geom = PO.records_f32(fwd)
        rng = np.random.default_rng(3)
        dgeom = np.zeros((c["P"], 32), dtype=F32)
        dgeom[:, :25] = rng.normal(size=(c["P"], 25))
        dgeom[fwd["ambiguous"]] = 0
        _REF[name] = dict(fwd=fwd, geom=geom, dgeom=dgeom, bwd=PO.backward_reference(c, geom, dgeom))
    return _REF[name]
