"""The Gaussian mapper's optimisation loops without an autograd tape: `GSMapper.optimization` and `GSMapper.pose_refine`
(hislam2/gs_backend_per_frame.py:451-587, :202-326) as direct calls into the C ABI -- about 25 launches per rendered view
instead of the ~100 launches + autograd bookkeeping of the tensor-op formulation in gs_mapper.py, which stays as the second
implementation the tests compare this one with (same losses, same Adam arithmetic, same pose update).

Per view and iteration:  cut3r_gs_activate -> cut3r_gs_preprocess / _bin / _render_forward (`_render`) -> loss kernels (+ the _map_coef /
_refine_coef launch for the scalar algebra between their two passes; `_colour_losses` is the mapping loops' block) -> the rasteriser's
_render_backward / _preprocess_backward -> cut3r_gs_activate_backward (`_backward`: gradient of theta accumulated over the views, 16 pose
sums per view) -> cut3r_gs_pose_step; then ONE Adam launch over all Gaussian parameters (`_adam`).  `pose_estimator` (a pose against the
frozen map, :123-177) ends its backward pass in cut3r_gs_pose_backward instead: dgeom -> the 16 pose sums in one kernel, no per-Gaussian
gradient, no Adam launch.

With Training.compensate_exposure (gs_backend_per_frame.py:516, :992) three launches per rendered view join them: cut3r_exposure_forward
between the rasteriser and the colour losses (pixel loss and SSIM then read the compensated image), cut3r_exposure_backward in place of
the `g_img += g_ssim` launch (the colour gradient back through A, and per-workgroup partial sums of the 12 exposure gradients), and
cut3r_gs_exposure_step after the pose step (Adam on A and b, state of ES floats per view, new per call like the reference's optimiser).
Without the flag the launches are the ones above.

The rasteriser's one host read per pass (the instance count) is taken in the FIRST iteration of a call only: later iterations run in
capacity mode (1.5 x the largest count seen + a margin, overflow flagged on the device).  The flag is read once at the end of the call; if
it is set, parameters, moments and poses are restored from the snapshot taken at the start and the whole call is redone with exact
counts -- no truncated iteration is ever kept.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from . import gaussian_rasterizer as GR
from ._lib import check
from .gaussian_rasterizer import _p, _s
from .gs_mapper import gt_normal, position_lr

PS = 32            # floats of pose state per view (include/cut3r_hip.h)
ES = 40            # floats of exposure state per view: A [9] row-major | b [3] | Adam m [12] | v [12] | steps | 3 x zero


def _arr(vals):
    return (C.c_float * len(vals))(*[float(v) for v in vals])


_IDENTITY16 = _arr([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1])
_ZERO3 = _arr([0, 0, 0])


def load_exposures(views, device):
    """[N, ES] from the views' exposure_a / exposure_b, moments and step count zero (the reference creates a new optimiser per call)"""
    es = torch.zeros(len(views), ES, dtype=torch.float32, device=device)
    for k, v in enumerate(views):
        es[k, 0:9] = v.exposure_a.detach().reshape(-1)
        es[k, 9:12] = v.exposure_b.detach()
    return es


def apply_exposure(color, view):
    """color [3,H,W] through the view's affine exposure model (cut3r_exposure_forward) -> a new [3,H,W] tensor"""
    if color.dtype != torch.float32 or color.dim() != 3 or color.shape[0] != 3 or not color.is_cuda:
        raise ValueError("apply_exposure: color must be a dense fp32 [3,H,W] tensor on the GPU")
    color = color.contiguous()
    es = load_exposures([view], color.device)
    out = torch.empty_like(color)
    check(_lib.load().cut3r_exposure_forward(_p(color), _p(es), color.shape[1], color.shape[2], _p(out), _s()), "exposure_forward")
    return out


class FusedTrainer:
    """workspaces + the two loops; one instance per GSMapper (buffers are re-sized when the number of Gaussians or the image size changes)"""

    def __init__(self, mapper):
        self.mp = mapper
        self.dev = mapper.device
        self.lib = _lib.load()
        self._shape = None
        self._cap = 0
        self.capacity = (1.5, 16384)             # capacity-mode iterations: factor on the largest instance count of iteration 0 + margin
        self.redone = 0                          # calls that overflowed their capacity and were redone from the snapshot
        self.exposure_state = None               # [N, ES] of the last optimization / global_BA call with exposure=True (else None)

    # ------------------------------------------------------------------ buffers
    def _buffers(self, P, H, W):
        if self._shape == (P, H, W):
            return
        dev = self.dev
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        i = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
        self.means, self.scales, self.rots, self.opac, self.shs = f(P, 3), f(P, 3), f(P, 4), f(P), f(P, 1, 3)
        self.geom, self.dgeom = f(P, GR.GS_REC), f(P, GR.GS_REC)
        self.radii, self.tiles, self.offsets = i(P), i(P), i(P)
        self.scan_ws = torch.empty(GR.workspace_bytes(P, 0), dtype=torch.uint8, device=dev)
        self.flat = f(P * 14 + P * 3)                  # d_means | d_scales | d_rots | d_opac | d_means2D | d_shs: zeroed together
        self.d_means, self.d_scales = self.flat[0:3 * P].view(P, 3), self.flat[3 * P:6 * P].view(P, 3)
        self.d_rots, self.d_opac = self.flat[6 * P:10 * P].view(P, 4), self.flat[10 * P:11 * P]
        self.d_means2D, self.d_shs = self.flat[11 * P:14 * P].view(P, 3), self.flat[14 * P:17 * P].view(P, 1, 3)
        self.gtheta = f(P, 14)
        if self._shape is None or self._shape[1:] != (H, W):
            self.img = {k: f(c, H, W) for k, c in (("color", 3), ("coord", 3), ("mcoord", 3), ("depth", 1), ("mdepth", 1), ("alpha", 1), ("normal", 3))}
            self.n_contrib, self.aux = i(2, H, W), f(2, H, W)
            self.smap, self.sd1, self.sd2, self.sd3 = f(3, H, W), f(3, H, W), f(3, H, W), f(3, H, W)
            self.g_img, self.g_ssim, self.g_depth = f(3, H, W), f(3, H, W), f(1, H, W)
            self.img_x = f(3, H, W)                    # the exposure-compensated colour image (exposure=True)
            self.zero_img = torch.zeros(3, H, W, dtype=torch.float32, device=dev)
            gx, gy = (W + 15) // 16, (H + 15) // 16
            self.ranges = i(gy * gx, 2)
            self.sums, self.coef, self.ratio = f(8), f(4), f(1)
            self.nvis, self.loss_acc, self.ssim_scale = f(1), torch.zeros(1, device=dev), f(1)
        self._shape = (P, H, W)
        self._cap = 0

    def _sort_buffers(self, n):
        if n <= self._cap:
            return
        dev = self.dev
        self._cap = int(n)
        self.keys_tmp = torch.empty(self._cap, dtype=torch.int64, device=dev)
        self.keys_sorted = torch.empty(self._cap, dtype=torch.int64, device=dev)
        self.vals_tmp = torch.empty(self._cap, dtype=torch.int32, device=dev)
        self.point_list = torch.empty(self._cap, dtype=torch.int32, device=dev)
        self.sort_ws = torch.empty(GR.workspace_bytes(self._shape[0], self._cap), dtype=torch.uint8, device=dev)

    @staticmethod
    def _image_size(views):
        """(H, W) shared by the views; the image buffers and the kernels' raw pointers assume ONE size and dense fp32 observations"""
        H, W = int(views[0].image_height), int(views[0].image_width)
        for v in views:
            if (int(v.image_height), int(v.image_width)) != (H, W):
                raise ValueError(f"tape-free GS trainer: views of different sizes ({v.image_height}x{v.image_width} vs {H}x{W})")
            if (tuple(v.original_image.shape) != (3, H, W) or tuple(v.depth.shape) != (H, W) or not v.original_image.is_contiguous()
                    or not v.depth.is_contiguous() or v.original_image.dtype != torch.float32 or v.depth.dtype != torch.float32):
                raise ValueError("tape-free GS trainer: a view's image / depth must be dense fp32 [3,H,W] / [H,W]")
        return H, W

    # ------------------------------------------------------------------ per-view pieces
    @staticmethod
    def _cam(v):
        c = getattr(v, "_fused_cam", None)
        if c is None:
            c = v._fused_cam = {"proj": _arr(v.projection_matrix_host.reshape(-1).tolist()), "tanx": math.tan(v.FoVx * 0.5),
                                "tany": math.tan(v.FoVy * 0.5), "K": (float(v.fx), float(v.fy), float(v.cx), float(v.cy))}
        return c

    def _render(self, v, ps_v, exact):
        """activations + rasteriser forward of one view into the shared buffers; returns the instance count (exact mode) or None"""
        lib, P = self.lib, self._shape[0]
        H, W = self._shape[1:]
        cam = self._cam(v)
        theta = self.mp.gaussians.theta
        check(lib.cut3r_gs_activate(P, _p(theta), _p(ps_v), _p(self.means), _p(self.scales), _p(self.rots), _p(self.opac), _p(self.shs), _s()),
              "gs_activate")
        check(lib.cut3r_gs_preprocess(P, _p(self.means), _p(self.scales), _p(self.rots), _p(self.opac), _p(self.shs), 0, 1, None, _IDENTITY16,
                                      cam["proj"], _ZERO3, W, H, cam["tanx"], cam["tany"], 0.0, 1.0, _p(self.geom), _p(self.radii), _p(self.tiles),
                                      _p(self.offsets), _p(self.scan_ws), self.scan_ws.numel(), _s()), "gs_preprocess")
        n_read = None
        if exact:
            n_read = int(self.offsets[-1].item()) & 0xffffffff
            if n_read > GR.MAX_INSTANCES:
                raise RuntimeError(f"GaussianRasterizer: {n_read} Gaussian/tile instances (limit {GR.MAX_INSTANCES}): degenerate scales or a diverged map")
            self._sort_buffers(max(1, n_read))
            n_inst, overflow = n_read, None
        else:
            n_inst, overflow = self._n_cap, GR.overflow_flag(self.dev)
        check(lib.cut3r_gs_bin(P, _p(self.geom), _p(self.offsets), n_inst, W, H, _p(self.keys_tmp), _p(self.vals_tmp), _p(self.keys_sorted),
                               _p(self.point_list), _p(self.ranges), _p(self.sort_ws), self.sort_ws.numel(), _p(overflow), _s()), "gs_bin")
        im = self.img
        check(lib.cut3r_gs_render_forward(_p(self.ranges), _p(self.point_list), _p(self.geom), W, H, cam["tanx"], cam["tany"], _ZERO3, _p(im["color"]),
                                          _p(im["coord"]), _p(im["mcoord"]), _p(im["depth"]), _p(im["mdepth"]), _p(im["alpha"]), _p(im["normal"]),
                                          _p(self.n_contrib), _p(self.aux), _s()), "gs_render_forward")
        return n_read

    def _render_backward(self, v, g_color, g_depth, g_normal=None):
        """rasteriser backward of one view (its forward buffers are still the current ones): the gradients of the colour, depth and
        (optionally) normal images -> self.dgeom"""
        P, (H, W) = self._shape[0], self._shape[1:]
        cam, im, z = self._cam(v), self.img, self.zero_img
        check(self.lib.cut3r_gs_render_backward(_p(self.ranges), _p(self.point_list), _p(self.geom), P, W, H, cam["tanx"], cam["tany"], _ZERO3,
                                                _p(self.n_contrib), _p(self.aux), _p(im["alpha"]), _p(im["coord"]), _p(im["depth"]), _p(im["normal"]),
                                                _p(g_color), _p(z), _p(z), _p(g_depth), _p(z), _p(z), _p(g_normal if g_normal is not None else z),
                                                _p(self.dgeom), _s()), "gs_render_backward")

    def _backward(self, v, ps_v, g_color, g_depth, iso_coef, gtheta, sums_v, g_normal=None):
        """rasteriser backward + activation chain of one view"""
        lib, P = self.lib, self._shape[0]
        H, W = self._shape[1:]
        cam = self._cam(v)
        self.flat.zero_()
        self._render_backward(v, g_color, g_depth, g_normal)
        check(lib.cut3r_gs_preprocess_backward(P, _p(self.means), _p(self.scales), _p(self.rots), _p(self.opac), _p(self.shs), 0, 1, _IDENTITY16,
                                               cam["proj"], _ZERO3, W, H, cam["tanx"], cam["tany"], 0.0, 1.0, _p(self.geom), _p(self.dgeom),
                                               _p(self.d_means), _p(self.d_scales), _p(self.d_rots), _p(self.d_opac), _p(self.d_shs), None,
                                               _p(self.d_means2D), _s()), "gs_preprocess_backward")
        check(lib.cut3r_gs_activate_backward(P, _p(self.mp.gaussians.theta), _p(ps_v), _p(self.d_means), _p(self.d_scales), _p(self.d_rots),
                                             _p(self.d_opac), _p(self.d_shs), _p(self.radii), float(iso_coef), _p(self.nvis), _p(gtheta), _p(sums_v),
                                             _s()), "gs_activate_backward")

    def _pose_backward(self, v, ps_v, g_color, g_depth, partials, sums_v):
        """rasteriser backward of one view, then dgeom straight to the view's 16 pose sums (cut3r_gs_pose_backward): the backward pass of
        an iteration that moves a pose against a frozen map.  sums_v is written, partials is scratch [cut3r_gs_pose_partial_rows(P), 16]"""
        P, (H, W) = self._shape[0], self._shape[1:]
        cam = self._cam(v)
        self._render_backward(v, g_color, g_depth)
        check(self.lib.cut3r_gs_pose_backward(P, _p(self.means), _p(self.scales), _p(self.rots), _p(self.opac), _IDENTITY16, cam["proj"], W, H,
                                              cam["tanx"], cam["tany"], 0.0, 1.0, _p(self.geom), _p(self.dgeom), _p(self.mp.gaussians.theta),
                                              _p(ps_v), _p(partials), _p(sums_v), _s()), "gs_pose_backward")

    def _compensate(self, es_v):
        """the rendered colour image through one view's exposure model -> self.img_x (what the colour losses then read)"""
        H, W = self._shape[1:]
        check(self.lib.cut3r_exposure_forward(_p(self.img["color"]), _p(es_v), H, W, _p(self.img_x), _s()), "exposure_forward")
        return self.img_x

    def _colour_losses(self, v, col, gt_n, w_depth, w_normal, g, acc, es_v=None, partials_v=None):
        """the colour block of one view, on the colour image `col` (the rendering, or its exposure-compensated copy) and the rendered depth:
        g x (0.8 L1 colour + w_depth inverse-depth L1 + w_normal agreement of the depth's normals with gt_n [3,H,W]) through the pixel-loss
        kernels and the coefficient launch between them (acc: where it adds that value, or None), 0.2 (1 - SSIM) at the weight the caller put
        into self.ssim_scale.  Leaves d loss / d rendered colour in self.g_img and d loss / d rendered depth in self.g_depth."""
        lib = self.lib
        H, W = self._shape[1:]
        K = self._cam(v)["K"]
        gt, depth = v.original_image, self.img["depth"]
        check(lib.cut3r_pixel_loss_forward(_p(col), _p(gt), _p(depth), _p(v.depth), _p(gt_n), H, W, K[0], K[1], K[2], K[3], _p(self.sums), _s()),
              "pixel_loss_forward")
        check(lib.cut3r_gs_map_coef(_p(self.sums), 0.8, float(w_depth), float(w_normal), g, H, W, _p(self.coef), _p(acc), _s()), "gs_map_coef")
        check(lib.cut3r_pixel_loss_backward(_p(col), _p(gt), _p(depth), _p(v.depth), _p(gt_n), H, W, K[0], K[1], K[2], K[3], _p(self.coef),
                                            _p(self.g_img), _p(self.g_depth), _s()), "pixel_loss_backward")
        check(lib.cut3r_ssim_forward(_p(col), _p(gt), 3, H, W, _p(self.smap), _p(self.sd1), _p(self.sd2), _p(self.sd3), _s()), "ssim_forward")
        check(lib.cut3r_ssim_backward(_p(col), _p(gt), _p(self.sd1), _p(self.sd2), _p(self.sd3), 3, H, W, _p(self.ssim_scale), _p(self.g_ssim),
                                      _s()), "ssim_backward")
        self._colour_gradient(es_v, partials_v)

    def _colour_gradient(self, es_v, partials_v):
        """g_img <- d loss / d rendered colour.  Without exposure: g_img + g_ssim.  With it: A (g_img + g_ssim), and the partial sums of the
        12 exposure gradients into partials_v (None: the exposure stays fixed)"""
        if es_v is None:
            self.g_img.add_(self.g_ssim)
            return
        H, W = self._shape[1:]
        check(self.lib.cut3r_exposure_backward(_p(self.img["color"]), _p(self.g_img), _p(self.g_ssim), _p(es_v), H, W, _p(self.g_img),
                                               _p(partials_v), _s()), "exposure_backward")

    def _adam(self, gm, reset=False):
        """ONE Adam step of all Gaussian parameters on self.gtheta; the step count advances on the host only (the device scalar of the
        tensor-op path goes stale).  reset: the step that follows an opacity reset leaves the opacity column where the reset put it, its
        moments zero -- the rule GaussianMap.step_like_reference states for the tensor-op path"""
        keep = gm.theta.detach()[:, 6:7].clone() if reset else None
        gm.steps += 1
        gm._steps_dev_stale = True
        b1, b2 = 0.9, 0.999
        check(self.lib.cut3r_gs_adam(self._shape[0] * 14, _p(gm.theta), _p(gm.m), _p(gm.v), _p(self.gtheta), _p(gm.lr), b1, b2, 1 - b1 ** gm.steps,
                                     1 - b2 ** gm.steps, 1e-15, _s()), "gs_adam")
        if reset:
            with torch.no_grad():
                gm.theta[:, 6:7] = keep
                gm.m[:, 6:7] = 0
                gm.v[:, 6:7] = 0

    def _single_view(self, v, ps_v, w_depth, w_normal, final, sums_v=None, es_v=None, partials=None, before_backward=None):
        """the part of an iteration global_BA and reinit_loop share: ONE view rendered with an exact instance count (the set of Gaussians
        changes under densification), the colour block at weight 1 against the view's own depth normals (into self.loss_acc when
        `final`), and the backward pass into self.gtheta / sums_v.  before_backward() runs between the two and may return the
        gradient of the rendered normal image."""
        gt_n = gt_normal(v)
        self.gtheta.zero_()
        if sums_v is not None:
            sums_v.zero_()
        if final:
            self.loss_acc.zero_()
        self._render(v, ps_v, True)
        col = self._compensate(es_v) if es_v is not None else self.img["color"]
        self._colour_losses(v, col, gt_n, w_depth, w_normal, 1.0, self.loss_acc if final else None, es_v, partials)
        g_normal = before_backward() if before_backward is not None else None
        self._backward(v, ps_v, self.g_img, self.g_depth, 0.0, self.gtheta, sums_v, g_normal=g_normal)

    # ------------------------------------------------------------------ pose state <-> cameras
    def _load_poses(self, views):
        ps = torch.zeros(len(views), PS, dtype=torch.float32, device=self.dev)
        for k, v in enumerate(views):
            ps[k, 0:7] = v.w2c_data
            ps[k, 7:10] = v.cam_trans_delta.detach()
            ps[k, 10:13] = v.cam_rot_delta.detach()
        return ps

    def _store_poses(self, views, ps):
        from .lietorch import SE3
        M = SE3(ps[:, 0:7].contiguous()).matrix()
        for k, v in enumerate(views):
            v.update_RT(M[k, :3, :3], M[k, :3, 3], data=ps[k, 0:7])
            v.cam_trans_delta.data.copy_(ps[k, 7:10])
            v.cam_rot_delta.data.copy_(ps[k, 10:13])

    @staticmethod
    def _store_exposures(views, es):
        for k, v in enumerate(views):
            v.exposure_a.data.copy_(es[k, 0:9].view(3, 3))
            v.exposure_b.data.copy_(es[k, 9:12])

    @staticmethod
    def _pose_snapshot(ps):
        """the snapshot of a loop that moves nothing but the pose state: taken now, put back by snapshot(restore=True)"""
        saved = ps.clone()

        def snapshot(restore=False):
            if restore:
                ps.copy_(saved)
        return snapshot

    # ------------------------------------------------------------------ the loops
    def _run(self, body, iters, snapshot):
        """iteration 0 with exact instance counts, the others in capacity mode; one overflow read at the end, redo from the snapshot if set"""
        flag = GR.overflow_flag(self.dev)
        flag.zero_()
        counts = body(0, True)
        self._n_cap = int(self.capacity[0] * max(counts)) + int(self.capacity[1])
        self._sort_buffers(self._n_cap)
        for it in range(1, iters):
            body(it, False)
        if iters > 1 and int(flag.item()):
            flag.zero_()
            self.redone += 1
            snapshot(restore=True)
            for it in range(iters):
                body(it, True)

    def optimization(self, views, iters, optimize_pose=True, exposure=False):
        """GSMapper.optimization without densification; returns the loss of the last iteration (float).  exposure: the colour losses read
        the rendering through each view's affine exposure model, whose 12 parameters step with the poses (only if optimize_pose)"""
        mp, gm, lib = self.mp, self.mp.gaussians, self.lib
        P = len(gm)
        H, W = self._image_size(views)
        self._buffers(P, H, W)
        N = len(views)
        g = 1.0 / N
        ps = self._load_poses(views)
        sums = torch.zeros(N, 16, dtype=torch.float32, device=self.dev) if optimize_pose else None
        lr = mp.config["opt_params"]["pose_lr"]
        es = self.exposure_state = load_exposures(views, self.dev) if exposure else None
        elr = mp.config["opt_params"].get("exposure_lr", 0.0005)
        rows = int(lib.cut3r_exposure_partial_rows(H, W))
        partials = torch.empty(N, rows, 12, dtype=torch.float32, device=self.dev) if exposure and optimize_pose else None
        self.ssim_scale.fill_(-0.2 * g / (3 * H * W))
        saved = {}

        def snapshot(restore=False):
            if restore:
                gm.theta.data.copy_(saved["theta"]); gm.m.copy_(saved["m"]); gm.v.copy_(saved["v"]); ps.copy_(saved["ps"])
                gm.steps = saved["steps"]
                if es is not None:
                    es.copy_(saved["es"])
            else:
                saved.update(theta=gm.theta.detach().clone(), m=gm.m.clone(), v=gm.v.clone(), ps=ps.clone(), steps=gm.steps,
                             es=es.clone() if es is not None else None)
        snapshot()
        gt_n = [gt_normal(v) for v in views]              # the keyframes' own depth normals (constant while their depth stays)
        last = [None]

        def body(it, exact):
            final = it == iters - 1
            self.gtheta.zero_()
            if sums is not None:
                sums.zero_()
            if final:
                self.loss_acc.zero_()
            counts = []
            extra = 0.0
            for k, v in enumerate(views):
                counts.append(self._render(v, ps[k], exact))
                col = self._compensate(es[k]) if es is not None else self.img["color"]
                self._colour_losses(v, col, gt_n[k], mp.lambda_depth, mp.lambda_normal, g, self.loss_acc if final else None,
                                    es[k] if es is not None else None, partials[k] if partials is not None else None)
                if final:                                 # the reported loss: the two terms that have no sums kernel, in tensor operations
                    vis = self.radii > 0
                    sc = self.scales
                    iso = (torch.abs(sc - sc.mean(dim=1, keepdim=True)) * vis[:, None]).sum() / (3 * vis.sum()).clamp_min(1)
                    extra = extra + g * (0.2 * (1.0 - self.smap.mean()) + mp.lambda_iso * iso)
                self._backward(v, ps[k], self.g_img, self.g_depth, g * mp.lambda_iso, self.gtheta, sums[k] if sums is not None else None)
            self._adam(gm)
            if sums is not None:
                for k in range(N):
                    check(lib.cut3r_gs_pose_step(_p(ps[k]), _p(sums[k]), 0.0, None, lr * 2, lr * 10, 1, _s()), "gs_pose_step")
            if partials is not None:
                for k in range(N):
                    check(lib.cut3r_gs_exposure_step(_p(es[k]), _p(partials[k]), rows, elr, _s()), "gs_exposure_step")
            if final:
                last[0] = self.loss_acc[0] + extra
            return counts

        self._run(body, iters, snapshot)
        if optimize_pose:
            self._store_poses(views, ps)
            if es is not None:
                self._store_exposures(views, es)
        return float(last[0]) if last[0] is not None else None

    def pose_refine(self, views, iters, alpha_th=0.5):
        """the optimisation part of GSMapper.pose_refine: the Gaussians stay fixed, the increments of the views' poses move (not folded
        until the end, as the reference's update_pose after the loop)"""
        mp, gm, lib = self.mp, self.mp.gaussians, self.lib
        P = len(gm)
        H, W = self._image_size(views)
        self._buffers(P, H, W)
        B = len(views)
        ps = self._load_poses(views)
        sums = torch.zeros(B, 16, dtype=torch.float32, device=self.dev)
        ratios = torch.zeros(B, 1, dtype=torch.float32, device=self.dev)
        lr = mp.config["opt_params"]["pose_lr"]

        def body(it, exact):
            sums.zero_()
            counts = []
            for k, v in enumerate(views):
                im = self.img
                counts.append(self._render(v, ps[k], exact))
                check(lib.cut3r_refine_loss_forward(_p(im["color"]), _p(v.original_image), _p(im["depth"]), _p(v.depth), _p(im["alpha"]),
                                                    float(alpha_th), H, W, _p(self.sums), _s()), "refine_loss_forward")
                check(lib.cut3r_gs_refine_coef(_p(self.sums), 5.0 / B, 1.0 / B, H, W, _p(self.coef), _p(ratios[k]), None, _s()), "gs_refine_coef")
                check(lib.cut3r_refine_loss_backward(_p(im["color"]), _p(v.original_image), _p(im["depth"]), _p(v.depth), _p(im["alpha"]),
                                                     float(alpha_th), H, W, _p(self.coef), _p(self.g_img), _p(self.g_depth), _s()), "refine_loss_backward")
                self._backward(v, ps[k], self.g_img, self.g_depth, 0.0, None, sums[k])
            for k in range(B):
                check(lib.cut3r_gs_pose_step(_p(ps[k]), _p(sums[k]), 0.05 / B, _p(ratios[k]), lr * 2, lr * 10, 0, _s()), "gs_pose_step")
            return counts

        self._run(body, iters, self._pose_snapshot(ps))
        for k in range(B):                                # update_pose: T <- exp(delta) T, delta <- 0
            check(lib.cut3r_gs_pose_step(_p(ps[k]), _p(sums[k]), 0.0, None, 0.0, 0.0, 2, _s()), "gs_pose_step (fold)")
        self._store_poses(views, ps)

    def pose_estimator(self, view, iters, use_depth=False, pose_backward="fused"):
        """GSMapper.pose_estimator's loop (gs_backend_per_frame.py:143-167): the Gaussians stay fixed, the view's increments take one Adam
        step (both at opt_params.pose_lr) per iteration and are folded into the pose after every one.  Loss: 0.8 L1 + 0.2 (1 - SSIM), with
        use_depth plus the mean of |1/d - 1/gt_d| over gt_d > 0.001 and d > 0.001 (the pixel-loss kernels with w_depth = 1; without it
        view.depth is all zero, the mask empty and its clamped count 1).  pose_backward: "fused" = cut3r_gs_pose_backward (one kernel, no
        per-Gaussian gradient in memory), "chain" = cut3r_gs_preprocess_backward + cut3r_gs_activate_backward(gtheta = NULL)."""
        if pose_backward not in ("fused", "chain"):
            raise ValueError(f"pose_backward must be 'fused' or 'chain', not {pose_backward!r}")
        mp, lib = self.mp, self.lib
        P = len(mp.gaussians)
        views = [view]
        H, W = self._image_size(views)
        self._buffers(P, H, W)
        ps = self._load_poses(views)
        sums = torch.zeros(16, dtype=torch.float32, device=self.dev)
        rows = int(lib.cut3r_gs_pose_partial_rows(P))
        partials = torch.empty(rows, 16, dtype=torch.float32, device=self.dev) if pose_backward == "fused" else None
        lr = float(mp.config["opt_params"]["pose_lr"])
        w_depth = 1.0 if use_depth else 0.0
        self.ssim_scale.fill_(-0.2 / (3 * H * W))

        def body(it, exact):
            count = self._render(view, ps[0], exact)
            self._colour_losses(view, self.img["color"], self.zero_img, w_depth, 0.0, 1.0, None)
            if partials is not None:
                self._pose_backward(view, ps[0], self.g_img, self.g_depth, partials, sums)
            else:
                sums.zero_()
                self._backward(view, ps[0], self.g_img, self.g_depth, 0.0, None, sums)
            check(lib.cut3r_gs_pose_step(_p(ps[0]), _p(sums), 0.0, None, lr, lr, 1, _s()), "gs_pose_step")
            return [count]

        self._run(body, iters, self._pose_snapshot(ps))
        self._store_poses(views, ps)

    def global_BA(self, iteration_total, densify=True, densify_every=None, opacity_reset=True, seed=0, exposure=False):
        """GSMapper.global_BA (gs_backend_per_frame.py:946-1058): one randomly drawn keyframe per iteration,
        colour + (inverse depth) + depth-normal agreement + the rendered-normal term (cut3r_normal_agree_*), densification statistics
        (cut3r_gs_densify_stats), clone / split / prune and opacity resets at the reference's iterations, position learning-rate decay.
        The instance count is read every iteration (the set of Gaussians changes under densification).  exposure: the colour losses read
        the rendering through the drawn view's exposure model, which steps with its pose (moments kept over the iterations of the call)."""
        import random
        mp, lib = self.mp, self.lib
        views = list(mp.viewpoints.values())
        H, W = self._image_size(views)
        ps = self._load_poses(views)
        sums = torch.zeros(len(views), 16, dtype=torch.float32, device=self.dev)
        rng = random.Random(seed)
        tr, op = mp.config["Training"], mp.config["opt_params"]
        update_every, reset_every = tr.get("gaussian_update_every", 200), tr.get("gaussian_reset", 3001)
        lr = op["pose_lr"]
        w_d, w_n = (mp.lambda_depth / 10, mp.lambda_normal) if densify_every is not None else (0.0, mp.lambda_normal / 2)
        self._buffers(len(mp.gaussians), H, W)
        self.ssim_scale.fill_(-0.2 / (3 * H * W))
        es = self.exposure_state = load_exposures(views, self.dev) if exposure else None
        elr = op.get("exposure_lr", 0.0005)
        rows = int(lib.cut3r_exposure_partial_rows(H, W))
        partials = torch.empty(rows, 12, dtype=torch.float32, device=self.dev) if exposure else None
        g_nrm = torch.empty(3, H, W, dtype=torch.float32, device=self.dev)
        last = None

        def rendered_normal_term():
            """agreement of the rendered normal of view v with the normal of its rendered depth: the value into the reported loss, the
            gradient into g_nrm and (added) self.g_depth"""
            nonlocal last
            im, K = self.img, self._cam(v)["K"]
            if final:
                check(lib.cut3r_normal_agree_forward(_p(im["normal"]), _p(im["depth"]), H, W, K[0], K[1], K[2], K[3], _p(self.nvis), _s()),
                      "normal_agree_forward")
                last = self.loss_acc[0] + 0.2 * (1.0 - self.smap.mean()) + w_n * self.nvis[0] / (H * W)
            check(lib.cut3r_normal_agree_backward(_p(im["normal"]), _p(im["depth"]), H, W, K[0], K[1], K[2], K[3], float(w_n) / (H * W), _p(g_nrm),
                                                  _p(self.g_depth), _s()), "normal_agree_backward")
            return g_nrm

        for iteration in range(iteration_total):
            mp.iteration_count += 1
            gm = mp.gaussians
            P = len(gm)
            self._buffers(P, H, W)
            k = rng.randint(0, len(views) - 1)
            v = views[k]
            final = iteration == iteration_total - 1
            self._single_view(v, ps[k], w_d, w_n, final, sums[k], es[k] if es is not None else None, partials, rendered_normal_term)
            if iteration < 10000 and densify:
                check(lib.cut3r_gs_densify_stats(P, _p(self.radii), _p(self.d_means2D), _p(gm.max_radii2D), _p(gm.grad_accum), _p(gm.grad_accum_abs), _p(gm.denom), _s()),
                      "gs_densify_stats")
            # the reference's order (gs_backend_per_frame.py:1025-1041): densify_and_prune / reset_opacity come BEFORE optimizer.step() and
            # re-create the parameters, whose .grad is then None: Adam skips every group after a densification (no update, no moment
            # update, no step increment) and the opacity group after a reset (_adam)
            do_densify = do_reset = False
            if iteration < 10000 and densify:
                do_densify = (iteration == iteration_total // 2) if densify_every is not None else ((mp.iteration_count + 1) % update_every == 0)
                if do_densify:
                    gm.densify_and_prune(op["densify_grad_threshold"], mp.gaussian_th, mp.gaussian_extent, mp.size_threshold)
                do_reset = bool((mp.iteration_count + 1) % reset_every == 0 and opacity_reset)
                if do_reset:
                    gm.reset_opacity()
            if not do_densify:
                self._adam(gm, reset=do_reset)
            if densify and "position_lr_final" in op:
                gm.lr[0, 0:3] = position_lr(op, iteration)
            check(lib.cut3r_gs_pose_step(_p(ps[k]), _p(sums[k]), 0.0, None, lr * 2, lr * 10, 1, _s()), "gs_pose_step")
            if es is not None:
                check(lib.cut3r_gs_exposure_step(_p(es[k]), _p(partials), rows, elr, _s()), "gs_exposure_step")
        self._store_poses(views, ps)
        if es is not None:
            self._store_exposures(views, es)
        return float(last) if last is not None else None

    def reinit_loop(self, iteration_total, seed=0):
        """the training loop of GSMapper.gaussian_reinit (gs_backend_per_frame.py:865-944): single-view iterations with FIXED poses --
        colour, inverse depth and the depth-normal term -- densification statistics and clone / split / prune every
        Training.gaussian_update_every iterations after the first 1000"""
        import random
        mp, lib = self.mp, self.lib
        views = list(mp.viewpoints.values())
        H, W = self._image_size(views)
        ps = self._load_poses(views)
        rng = random.Random(seed)
        update_every = mp.config["Training"].get("gaussian_update_every", 200)
        op = mp.config["opt_params"]
        self._buffers(len(mp.gaussians), H, W)
        self.ssim_scale.fill_(-0.2 / (3 * H * W))
        last = None

        def report():
            nonlocal last
            if final:
                last = self.loss_acc[0] + 0.2 * (1.0 - self.smap.mean())

        for iteration in range(iteration_total):
            gm = mp.gaussians
            P = len(gm)
            self._buffers(P, H, W)
            k = rng.randint(0, len(views) - 1)
            final = iteration == iteration_total - 1
            self._single_view(views[k], ps[k], mp.lambda_depth, mp.lambda_normal, final, before_backward=report)
            if iteration > 1000:
                check(lib.cut3r_gs_densify_stats(P, _p(self.radii), _p(self.d_means2D), _p(gm.max_radii2D), _p(gm.grad_accum), _p(gm.grad_accum_abs), _p(gm.denom), _s()),
                      "gs_densify_stats")
            if iteration > 1000 and (iteration + 1) % update_every == 0:
                # (gs_backend_per_frame.py:920-935: densification first, then an optimizer.step() that finds no gradients)
                gm.densify_and_prune(op["densify_grad_threshold"], mp.gaussian_th, mp.gaussian_extent, mp.size_threshold)
            else:
                self._adam(gm)
        return float(last) if last is not None else None
