"""Dense reconstruction: TSDF fusion of depth maps and triangle-mesh extraction on the gfx950 kernels of csrc/tsdf.hip.

The reference makes a mesh after every run (scripts/run_replica.py:40-52 -> tsdf_integrate.py): the keyframe depth and colour renders
of the Gaussian map go into an Open3D VoxelBlockGrid and `tsdf_mesh_w{w:.1f}.ply` is written per weight threshold.  Here:

  TSDFVolume       a DENSE voxel grid in HBM (fp32 planes tsdf, weight, color[3]: 20 B per voxel), at most 2^31 - 1 voxels
  SparseTSDFVolume the same lattice and the same per-voxel fusion restricted to allocated bricks of 8^3 voxels (csrc/tsdf_sparse.hip):
                   memory follows the surface area, so a floor of rooms, a finer voxel or objects far apart fit where the dense grid
                   raises; on its allocated voxels it holds the dense grid's bits and its mesh is the dense mesh (`sparse=True` below)
  fuse_keyframes   the tracker's keyframe store (depth, image, w2c, intrinsics, optional confidence gate) -> TSDFVolume
  fuse_mapper      the reference's source: every mapper keyframe rendered at its refined pose, quantised as the reference's files are
                   (hislam2/gaussian/utils/eval_utils.py:124-134: depth uint16 at 6553.5 per metre, colour (x*255) truncated to u8)
  LiveTSDFVolume   the sparse volume's lattice and bricks with integer accumulators (csrc/tsdf_live.hip): views are added, removed and
                   re-posed exactly while a run goes on, and the volume always equals a fresh fusion of the views that are in
  ray_cast         (all volumes) depth, normal and colour images of the fused model at given poses, marched through the voxels
                   (csrc/tsdf_raycast.hip: Open3D's VoxelBlockGrid.ray_cast); shade / write_previews turn them into PNGs
  write_ply / read_ply   binary little-endian PLY (x y z float, red green blue uchar, vertex_indices uchar count + int32)

Truncation: tsdf_integrate.py passes no sdf_trunc, so Open3D's default of 8 voxels applies; that is the default here
(`trunc_voxels=8.0`), a choice, not something pinned by a run of the reference.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from . import ops, views
from .views import inverse_affine as c2w_rows     # camera->world rows fp32 [B,12] of world->camera rows: the mark kernel and the ray cast

DEPTH_SCALE = 6553.5            # tsdf_integrate.py --depth_scale, eval_utils.py:131


class Mesh(NamedTuple):
    vertices: np.ndarray        # float32 [V,3]
    colors: np.ndarray          # uint8 [V,3]
    faces: np.ndarray           # int32 [F,3]


class RayCast(NamedTuple):
    depth: torch.Tensor         # float32 [B,H,W] z-depth of the surface, 0 where the ray misses
    normal: torch.Tensor        # float32 [B,H,W,3] world frame, towards the viewer, 0 on a miss (None when not asked for)
    color: torch.Tensor         # uint8 [B,3,H,W], 0 on a miss (None when not asked for)


def _lattice(lo, hi, voxel_size, pad):
    """(lo - pad, dims) of the voxel lattice over [lo - pad, hi + pad]: the last centre at >= hi + pad"""
    lo = np.asarray(lo, np.float64) - pad
    hi = np.asarray(hi, np.float64) + pad
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(hi >= lo)):
        raise ValueError(f"TSDF bounds {lo} .. {hi} are not a box")
    return lo, [int(math.ceil((h - l) / voxel_size - 1e-6)) + 1 for l, h in zip(lo, hi)]


def _stack(dev, depth, w2c, K, rgb, conf, conf_min):
    """the views of integrate() as the kernels take them: depth [B,H,W], w2c [B,12], K [B,4] fp32, rgb u8, conf fp32 or None"""
    depth = torch.as_tensor(depth).to(dev, torch.float32).contiguous()
    if depth.dim() == 2:
        depth = depth[None]
    B = depth.shape[0]
    w2c = views.pose_rows(w2c, torch.float32, single=True).reshape(-1, 12).to(dev).contiguous()
    if w2c.shape[0] != B:
        raise ValueError(f"{B} depth maps, {w2c.shape[0]} poses")
    K = views.intrinsics(K, B, torch.float32).to(dev)
    if rgb is not None:
        rgb = torch.as_tensor(rgb).to(dev).contiguous()
    if conf is not None and conf_min is not None:
        conf = torch.as_tensor(conf).to(dev, torch.float32).contiguous()
    else:
        conf = None
    return depth, w2c, K, rgb, conf


class _Volume:
    """What the two volumes share: the fp32 lattice and truncation, from_bounds, the batching of views into launches of <= 16 and the mesh
    as numpy arrays.  A subclass checks its dims, owns its storage and supplies grid_for, _integrate_batch and _extract."""

    def __init__(self, origin, voxel_size, dims, trunc_voxels, depth_max, device):
        if not voxel_size > 0 or not trunc_voxels > 0:
            raise ValueError("voxel_size and trunc_voxels must be > 0")
        self.origin = tuple(float(np.float32(o)) for o in origin)
        self.voxel_size = float(np.float32(voxel_size))
        self.dims = tuple(dims)
        self.trunc = float(np.float32(trunc_voxels * self.voxel_size))
        self.depth_max = float(depth_max)
        self.device = torch.device(device)

    @classmethod
    def _from_bounds(cls, lo, hi, voxel_size, pad, limit, trunc_voxels, depth_max, device):
        pad = trunc_voxels * voxel_size if pad is None else pad
        origin, dims = cls.grid_for(lo, hi, voxel_size, pad, limit)
        return cls(origin, voxel_size, dims, trunc_voxels=trunc_voxels, depth_max=depth_max, device=device)

    def _integrate(self, depth, w2c, K, rgb, conf, conf_ds, conf_min):
        """the views (as _stack returns them) through _integrate_batch, <= 16 at a time, in order"""
        for a in range(0, depth.shape[0], ops.TSDF_MAX_VIEWS):
            b = a + ops.TSDF_MAX_VIEWS
            self._integrate_batch(depth[a:b], w2c[a:b], K[a:b], self.trunc, self.depth_max, rgb=None if rgb is None else rgb[a:b],
                                  conf=None if conf is None else conf[a:b], conf_ds=conf_ds, conf_min=0.0 if conf_min is None else conf_min)
        return self

    @torch.no_grad()
    def extract_mesh(self, weight_threshold=1.0) -> Mesh:
        return Mesh(*(t.cpu().numpy() for t in self._extract(weight_threshold)))

    @torch.no_grad()
    def ray_cast(self, w2c, K, H, W, depth_min=0.0, depth_max=None, weight_threshold=1.0, step_voxels=0.5, normals=True, colors=True,
                 count=False):
        """the fused model seen from B views of H x W (Open3D VoxelBlockGrid.ray_cast), in launches of <= 16: w2c [B,12] (or [B,3,4] /
        [B,4,4]) world->camera, K [4] or [B,4] fx fy cx cy.  Every pixel's ray is sampled at z-depths depth_min + k * step_voxels *
        voxel_size up to depth_max (None: the volume's own); the surface lies between a sample with tsdf >= 0 and the next with tsdf <
        0, both in cells whose corners all have weight >= weight_threshold.  A ray that meets a negative value first (the camera is
        inside or behind a surface, or the ray comes out of unknown space) misses.  count=True: also the int32 [B,H,W] samples looked
        up per ray, as a fourth value."""
        w2c = views.pose_rows(w2c, torch.float32, single=True).reshape(-1, 12)
        B = w2c.shape[0]
        if B < 1:
            raise ValueError("ray_cast: no poses")
        c2w = torch.from_numpy(c2w_rows(w2c.cpu().numpy())).to(self.device)
        K = views.intrinsics(K, B, torch.float32).to(self.device)
        t_max = self.depth_max if depth_max is None else float(depth_max)
        step = float(np.float32(step_voxels * self.voxel_size))
        out = [self._ray_cast_batch(c2w[a:a + ops.TSDF_MAX_VIEWS], K[a:a + ops.TSDF_MAX_VIEWS], int(H), int(W), float(depth_min), t_max, step,
                                    weight_threshold=weight_threshold, normals=normals, colors=colors, count=count)
               for a in range(0, B, ops.TSDF_MAX_VIEWS)]
        depth, normal, color, samples = (None if q[0] is None else torch.cat(q) for q in zip(*out))
        return (RayCast(depth, normal, color), samples) if count else RayCast(depth, normal, color)


class TSDFVolume(_Volume):
    """Dense TSDF grid: voxel (i, j, k) at origin + voxel_size * (i, j, k), planes [Z,Y,X] (x fastest); tsdf = 1, weight = color = 0 at start."""

    def __init__(self, origin, voxel_size, dims, trunc_voxels=8.0, depth_max=5.0, device="cuda:0"):
        X, Y, Z = (int(d) for d in dims)
        if min(X, Y, Z) <= 0 or X * Y * Z >= 2 ** 31:
            raise ValueError(f"TSDF grid {X}x{Y}x{Z}: dims must be > 0 and X*Y*Z < 2^31")
        super().__init__(origin, voxel_size, (X, Y, Z), trunc_voxels, depth_max, device)
        self.tsdf = torch.ones(Z, Y, X, dtype=torch.float32, device=self.device)
        self.weight = torch.zeros(Z, Y, X, dtype=torch.float32, device=self.device)
        self.color = torch.zeros(3, Z, Y, X, dtype=torch.float32, device=self.device)

    @staticmethod
    def grid_for(lo, hi, voxel_size, pad, max_voxels=2 ** 30):
        """(origin, dims) of the grid over [lo - pad, hi + pad]; ValueError naming the memory when it exceeds max_voxels"""
        lo, dims = _lattice(lo, hi, voxel_size, pad)
        n = dims[0] * dims[1] * dims[2]
        if n > max_voxels or n >= 2 ** 31:
            raise ValueError(f"TSDF grid {dims[0]}x{dims[1]}x{dims[2]} = {n} voxels needs {n * 20 / 1e9:.1f} GB at 20 B per voxel "
                             f"(limit {min(max_voxels, 2 ** 31 - 1)} voxels): raise voxel_size or max_voxels, or tighten the bounds")
        return tuple(float(v) for v in lo), tuple(dims)

    @classmethod
    def from_bounds(cls, lo, hi, voxel_size, pad=None, max_voxels=2 ** 30, trunc_voxels=8.0, depth_max=5.0, device="cuda:0"):
        """the grid covering the box [lo, hi] padded by `pad` (default: the truncation distance)"""
        return cls._from_bounds(lo, hi, voxel_size, pad, max_voxels, trunc_voxels, depth_max, device)

    @property
    def nbytes(self):
        return 20 * self.dims[0] * self.dims[1] * self.dims[2]

    @torch.no_grad()
    def integrate(self, depth, w2c, K, rgb=None, conf=None, conf_ds=1, conf_min=None):
        """fuse B views in order, in launches of <= 16.  depth [B,H,W] metres; w2c [B,12] (or [B,3,4] / [B,4,4]) world->camera; K [4] or
        [B,4] fx fy cx cy; rgb u8 [B,3,H,W]; conf [B,h,w] at stride conf_ds, pixels with conf < conf_min skipped (conf_min None: no gate)."""
        return self._integrate(*_stack(self.device, depth, w2c, K, rgb, conf, conf_min), conf_ds, conf_min)

    def _integrate_batch(self, *views, **gate):
        ops.tsdf_integrate(self.tsdf, self.weight, self.color, self.origin, self.voxel_size, *views, **gate)

    def _extract(self, weight_threshold):
        return ops.tsdf_extract_mesh(self.tsdf, self.weight, self.color, self.origin, self.voxel_size, weight_threshold)

    def _ray_cast_batch(self, c2w, K, H, W, t_min, t_max, step, **out):
        return ops.tsdf_ray_cast(self.tsdf, self.weight, self.color, self.origin, self.voxel_size, c2w, K, H, W, t_min, t_max, step, **out)


class SparseTSDFVolume(_Volume):
    """Sparse TSDF volume: the lattice of TSDFVolume over a VIRTUAL grid `dims` (voxel (i, j, k) at origin + voxel_size * (i, j, k)), stored
    only where bricks of 8^3 voxels are allocated.  An allocated voxel holds what the dense grid would hold, bit for bit: every view
    updates every allocated voxel it would update there, free space included.

    allocate() flags the bricks that the views can give a negative tsdf, or a 26-neighbour of one (a superset, from the depth maps
    alone), so the mesh of a volume whose views were all allocated before any was integrated equals the dense mesh as a set of
    triangles; vertices come in (pool voxel, direction mask) order, faces in (pool cell, tetrahedron, triangle) order.  A brick
    allocated after some views were integrated has missed those views: integrate(allocate=True) on a fresh volume, or allocate() over
    all views first and integrate(allocate=False) after, as fuse_keyframes / fuse_mapper do.

    Limits: dims <= 2^20 per axis, ceil(dims / 8) bricks <= 2^28 table entries (5 B each), allocated voxels < 2^31."""

    def __init__(self, origin, voxel_size, dims, trunc_voxels=8.0, depth_max=5.0, device="cuda:0"):
        X, Y, Z = (int(d) for d in dims)
        if min(X, Y, Z) <= 0 or max(X, Y, Z) > ops.TSDF_SPARSE_MAX_DIM:
            raise ValueError(f"sparse TSDF grid {X}x{Y}x{Z}: dims must be in 1..{ops.TSDF_SPARSE_MAX_DIM} per axis")
        BX, BY, BZ = ops.tsdf_brick_dims((X, Y, Z))
        if BX * BY * BZ > ops.TSDF_SPARSE_MAX_TABLE:
            raise ValueError(f"sparse TSDF grid {X}x{Y}x{Z}: {BX * BY * BZ} bricks exceed the table limit of {ops.TSDF_SPARSE_MAX_TABLE} entries")
        super().__init__(origin, voxel_size, (X, Y, Z), trunc_voxels, depth_max, device)
        self.brick_dims = (BX, BY, BZ)
        self.flags = torch.zeros(BZ, BY, BX, dtype=torch.uint8, device=self.device)
        self.table = torch.full((BZ, BY, BX), -1, dtype=torch.int32, device=self.device)
        self.bricks = torch.zeros(0, dtype=torch.int32, device=self.device)
        self.tsdf = torch.ones(0, ops.TSDF_BRICK_VOXELS, dtype=torch.float32, device=self.device)
        self.weight = torch.zeros(0, ops.TSDF_BRICK_VOXELS, dtype=torch.float32, device=self.device)
        self.color = torch.zeros(3, 0, ops.TSDF_BRICK_VOXELS, dtype=torch.float32, device=self.device)

    @staticmethod
    def grid_for(lo, hi, voxel_size, pad, max_bricks=ops.TSDF_SPARSE_MAX_TABLE):
        """(origin, dims) of the virtual grid over [lo - pad, hi + pad], the lattice TSDFVolume.grid_for gives; ValueError when it has
        more than max_bricks bricks of 8^3 voxels (the table holds 5 B per brick, allocated or not)"""
        lo, dims = _lattice(lo, hi, voxel_size, pad)
        nb = int(np.prod([(d + ops.TSDF_BRICK - 1) // ops.TSDF_BRICK for d in dims], dtype=object))
        cap = min(int(max_bricks), ops.TSDF_SPARSE_MAX_TABLE)
        if max(dims) > ops.TSDF_SPARSE_MAX_DIM or nb > cap:
            raise ValueError(f"sparse TSDF grid {dims[0]}x{dims[1]}x{dims[2]} = {nb} bricks needs a {nb * 5 / 1e9:.1f} GB table at 5 B per brick "
                             f"(limit {cap} bricks, {ops.TSDF_SPARSE_MAX_DIM} voxels per axis): raise voxel_size or tighten the bounds")
        return tuple(float(v) for v in lo), tuple(dims)

    @classmethod
    def from_bounds(cls, lo, hi, voxel_size, pad=None, max_bricks=ops.TSDF_SPARSE_MAX_TABLE, trunc_voxels=8.0, depth_max=5.0, device="cuda:0"):
        """the virtual grid covering the box [lo, hi] padded by `pad` (default: the truncation distance); nothing is allocated yet"""
        return cls._from_bounds(lo, hi, voxel_size, pad, max_bricks, trunc_voxels, depth_max, device)

    @property
    def n_bricks(self):
        return int(self.bricks.shape[0])

    @property
    def nbytes(self):
        """pool (20 B per allocated voxel) + brick list + table and flags (5 B per brick of the virtual grid)"""
        return (20 * ops.TSDF_BRICK_VOXELS + 4) * self.n_bricks + 5 * self.table.numel()

    @torch.no_grad()
    def allocate(self, depth, w2c, K):
        """allocate the bricks the views can give a negative tsdf or a neighbour of one; returns how many were added.  Bricks already
        there keep their values; a new brick starts at tsdf = 1, weight = color = 0 and has missed every view integrated so far."""
        depth, w2c, K, _, _ = _stack(self.device, depth, w2c, K, None, None, None)
        c2w = torch.from_numpy(c2w_rows(w2c.cpu().numpy())).to(self.device)
        ops.tsdf_sparse_mark(self.flags, self.dims, self.origin, self.voxel_size, depth, c2w, K, self.trunc, self.depth_max)
        old = self.bricks
        n = ops.tsdf_sparse_assign(self.flags, self.table, self.dims)
        if n == old.shape[0]:
            return 0
        if n * ops.TSDF_BRICK_VOXELS >= 2 ** 31:
            raise ValueError(f"sparse TSDF pool of {n} bricks: 2^31 voxels or more ({n * ops.TSDF_BRICK_VOXELS * 20 / 1e9:.1f} GB)")
        self.bricks = torch.nonzero(self.flags.reshape(-1)).reshape(-1).to(torch.int32)
        tsdf = torch.ones(n, ops.TSDF_BRICK_VOXELS, dtype=torch.float32, device=self.device)
        weight = torch.zeros(n, ops.TSDF_BRICK_VOXELS, dtype=torch.float32, device=self.device)
        color = torch.zeros(3, n, ops.TSDF_BRICK_VOXELS, dtype=torch.float32, device=self.device)
        if old.shape[0]:
            slot = self.table.reshape(-1)[old.long()].long()           # where the bricks that were there have moved
            tsdf[slot], weight[slot], color[:, slot] = self.tsdf, self.weight, self.color
        self.tsdf, self.weight, self.color = tsdf, weight, color
        return n - int(old.shape[0])

    @torch.no_grad()
    def integrate(self, depth, w2c, K, rgb=None, conf=None, conf_ds=1, conf_min=None, allocate=True):
        """TSDFVolume.integrate over the allocated bricks.  allocate=True first allocates for ALL the views given (then fuses them in
        launches of <= 16): right for a fresh volume; on a volume that already holds views, the bricks it adds have missed those."""
        depth, w2c, K, rgb, conf = _stack(self.device, depth, w2c, K, rgb, conf, conf_min)
        if allocate:
            self.allocate(depth, w2c, K)
        if self.n_bricks == 0:
            return self
        return self._integrate(depth, w2c, K, rgb, conf, conf_ds, conf_min)

    def _integrate_batch(self, *views, **gate):
        ops.tsdf_sparse_integrate(self.tsdf, self.weight, self.color, self.bricks, self.dims, self.origin, self.voxel_size, *views, **gate)

    def _extract(self, weight_threshold):
        if self.n_bricks == 0:
            return torch.zeros(0, 3, dtype=torch.float32), torch.zeros(0, 3, dtype=torch.uint8), torch.zeros(0, 3, dtype=torch.int32)
        return ops.tsdf_sparse_extract_mesh(self.tsdf, self.weight, self.color, self.table, self.bricks, self.dims, self.origin,
                                            self.voxel_size, weight_threshold)

    def _ray_cast_batch(self, c2w, K, H, W, t_min, t_max, step, weight_threshold=1.0, normals=True, colors=True, count=False):
        if self.n_bricks == 0:                                          # nothing stored: every ray misses
            B, dev = c2w.shape[0], self.device
            return (torch.zeros(B, H, W, dtype=torch.float32, device=dev),
                    torch.zeros(B, H, W, 3, dtype=torch.float32, device=dev) if normals else None,
                    torch.zeros(B, 3, H, W, dtype=torch.uint8, device=dev) if colors else None,
                    torch.zeros(B, H, W, dtype=torch.int32, device=dev) if count else None)
        return ops.tsdf_sparse_ray_cast(self.tsdf, self.weight, self.color, self.table, self.bricks, self.dims, self.origin, self.voxel_size,
                                        c2w, K, H, W, t_min, t_max, step, weight_threshold=weight_threshold, normals=normals, colors=colors,
                                        count=count)

    @torch.no_grad()
    def allocated_mask(self):
        """bool [Z,Y,X]: the voxels of the virtual grid that are stored (raises above the dense limit of 2^31 - 1 voxels)"""
        X, Y, Z = self._dense_dims()
        m = self.flags.bool()[:, None, :, None, :, None].expand(-1, 8, -1, 8, -1, 8)
        return m.reshape(self.brick_dims[2] * 8, self.brick_dims[1] * 8, self.brick_dims[0] * 8)[:Z, :Y, :X].contiguous()

    def _dense_dims(self):
        X, Y, Z = self.dims
        if self.table.numel() * ops.TSDF_BRICK_VOXELS >= 2 ** 31:
            raise ValueError(f"sparse TSDF grid {X}x{Y}x{Z}: too large for dense planes (2^31 voxels or more)")
        return X, Y, Z

    @torch.no_grad()
    def to_dense(self):
        """(tsdf [Z,Y,X], weight [Z,Y,X], color [3,Z,Y,X]) of the virtual grid, 1 / 0 / 0 where nothing is allocated (raises above the
        dense limit of 2^31 - 1 voxels)"""
        out = _dense_from_bricks(self.bricks, self.brick_dims, self._dense_dims(), (self.tsdf, self.weight, *self.color), (1.0, 0.0, 0.0, 0.0, 0.0))
        return out[0], out[1], torch.stack(out[2:])


def _dense_from_bricks(bricks, brick_dims, dims, pools, inits):
    """per pool plane [nb,512] of a brick volume: the plane [Z,Y,X] of the virtual grid, `init` where no brick is allocated"""
    X, Y, Z = dims
    BX, BY, BZ = brick_dims
    t = bricks.long()
    bx, by, bz = t % BX, (t // BX) % BY, t // (BX * BY)
    out = []
    for pool, init in zip(pools, inits):
        d = torch.full((BZ, 8, BY, 8, BX, 8), init, dtype=pool.dtype, device=pool.device)
        d[bz, :, by, :, bx, :] = pool.reshape(-1, 8, 8, 8)
        out.append(d.reshape(BZ * 8, BY * 8, BX * 8)[:Z, :Y, :X].contiguous())
    return out


class LiveRecord(NamedTuple):
    """a view that is in a LiveTSDFVolume, as the volume's own device copies: exactly the bits that put it in, so that taking it out
    replays them (the keyframe store rewrites poses and depths in place)"""
    depth: torch.Tensor         # float32 [H,W]
    w2c: torch.Tensor           # float32 [12]
    K: torch.Tensor             # float32 [4]
    rgb: torch.Tensor           # uint8 [3,H,W], None in a colourless volume
    conf: torch.Tensor          # float32 [h,w] at stride conf_ds, None without a gate
    conf_ds: int
    conf_min: float

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.depth, self.w2c, self.K, self.rgb, self.conf) if t is not None)

    def launch_key(self):
        """views that can share a launch: one image size and one confidence gate"""
        return (tuple(self.depth.shape), None if self.conf is None else (tuple(self.conf.shape), self.conf_ds, self.conf_min))


class LiveTSDFVolume(_Volume):
    """A TSDF volume that is kept current while a run goes on: views are added, removed and re-posed EXACTLY.  The lattice, the brick
    table (flags, table, bricks; mark and assign), the mesh extraction and the ray cast are SparseTSDFVolume's; the pool holds integer
    accumulators (csrc/tsdf_live.hip) instead of a running fp32 average:

        acc int32 [5,nb,512]   sum_q, count, sum_r, sum_g, sum_b      q = rint(32768 * min(1, sdf / trunc)) per view, exact

    Integer sums commute and a subtraction undoes an addition, so acc depends on the SET of views that are in and on nothing else: after
    any history of add / remove / update it equals, bit for bit, a fresh volume given the final views (on the bricks that one allocates;
    bricks are never freed, so this one may hold more).  A brick allocated late catches up on every view already in -- the volume keeps
    its own copy of each (LiveRecord), keyed by an integer id.  The mesh and the ray cast read fp32 planes resolved from acc as correctly
    rounded means: they are NOT the bits of SparseTSDFVolume, whose running average rounds at every view; the tsdf differs by at most
    2^-16 + 3 n 2^-24 after n views.

    color: whether colour is accumulated, fixed for the volume's life; every view then comes with rgb, or none does.
    Limits: SparseTSDFVolume's, and at most 65535 views in at once (65535 * 32768 < 2^31)."""

    def __init__(self, origin, voxel_size, dims, trunc_voxels=8.0, depth_max=5.0, device="cuda:0", color=True):
        X, Y, Z = (int(d) for d in dims)
        if min(X, Y, Z) <= 0 or max(X, Y, Z) > ops.TSDF_SPARSE_MAX_DIM:
            raise ValueError(f"live TSDF grid {X}x{Y}x{Z}: dims must be in 1..{ops.TSDF_SPARSE_MAX_DIM} per axis")
        BX, BY, BZ = ops.tsdf_brick_dims((X, Y, Z))
        if BX * BY * BZ > ops.TSDF_SPARSE_MAX_TABLE:
            raise ValueError(f"live TSDF grid {X}x{Y}x{Z}: {BX * BY * BZ} bricks exceed the table limit of {ops.TSDF_SPARSE_MAX_TABLE} entries")
        super().__init__(origin, voxel_size, (X, Y, Z), trunc_voxels, depth_max, device)
        self.brick_dims = (BX, BY, BZ)
        self.colored = bool(color)
        self.flags = torch.zeros(BZ, BY, BX, dtype=torch.uint8, device=self.device)
        self.table = torch.full((BZ, BY, BX), -1, dtype=torch.int32, device=self.device)
        self.bricks = torch.zeros(0, dtype=torch.int32, device=self.device)
        self.acc = torch.zeros(5, 0, ops.TSDF_BRICK_VOXELS, dtype=torch.int32, device=self.device)
        self.records = {}                       # id -> LiveRecord of every view that is in
        self._planes = None                     # (tsdf, weight, color) resolved from acc; None after any change

    grid_for = staticmethod(SparseTSDFVolume.grid_for)

    @classmethod
    def from_bounds(cls, lo, hi, voxel_size, pad=None, max_bricks=ops.TSDF_SPARSE_MAX_TABLE, trunc_voxels=8.0, depth_max=5.0, device="cuda:0",
                    color=True):
        """the virtual grid covering the box [lo, hi] padded by `pad` (default: the truncation distance); nothing is allocated yet"""
        pad = trunc_voxels * voxel_size if pad is None else pad
        origin, dims = cls.grid_for(lo, hi, voxel_size, pad, max_bricks)
        return cls(origin, voxel_size, dims, trunc_voxels=trunc_voxels, depth_max=depth_max, device=device, color=color)

    @classmethod
    def around(cls, center, half_extent, voxel_size, trunc_voxels=8.0, depth_max=5.0, device="cuda:0", color=True):
        """the virtual grid as a cube of half side `half_extent` around `center` -- a run does not know its bounds up front.  Raises, with
        the table's size, past the table limits; views that reach outside the cube are clipped to it."""
        if not float(half_extent) > 0:
            raise ValueError("half_extent must be > 0")
        c = np.asarray(center, np.float64).reshape(3)
        return cls.from_bounds(c - float(half_extent), c + float(half_extent), voxel_size, pad=0.0, trunc_voxels=trunc_voxels,
                               depth_max=depth_max, device=device, color=color)

    @property
    def n_bricks(self):
        return int(self.bricks.shape[0])

    @property
    def nbytes(self):
        """accumulators (20 B per allocated voxel) + brick list + table and flags (5 B per brick of the virtual grid) + the records + the
        resolved planes when they exist (another 20 B per allocated voxel)"""
        n = (20 * ops.TSDF_BRICK_VOXELS + 4) * self.n_bricks + 5 * self.table.numel() + sum(r.nbytes for r in self.records.values())
        return n + (20 * ops.TSDF_BRICK_VOXELS * self.n_bricks if self._planes is not None else 0)

    # ------------------------------------------------------------------------------------------------------------------ the pool
    def _allocate(self, depth, w2c, K):
        """SparseTSDFVolume.allocate on the accumulators; returns the pool slots that are new (int32, ascending), None when there is none"""
        c2w = torch.from_numpy(c2w_rows(w2c.cpu().numpy())).to(self.device)
        ops.tsdf_sparse_mark(self.flags, self.dims, self.origin, self.voxel_size, depth, c2w, K, self.trunc, self.depth_max)
        old = self.bricks
        n = ops.tsdf_sparse_assign(self.flags, self.table, self.dims)
        if n == old.shape[0]:
            return None
        if n * ops.TSDF_BRICK_VOXELS >= 2 ** 31:
            raise ValueError(f"live TSDF pool of {n} bricks: 2^31 voxels or more ({n * ops.TSDF_BRICK_VOXELS * 20 / 1e9:.1f} GB)")
        self.bricks = torch.nonzero(self.flags.reshape(-1)).reshape(-1).to(torch.int32)
        self._planes = None
        return self._regrow(old, n)

    def _regrow(self, old, n):
        """the pool of n bricks with the accumulators of the bricks `old` moved to their new slots (a copy of the whole pool); returns the
        other slots (int32, ascending), which start at zero"""
        acc = torch.zeros(5, n, ops.TSDF_BRICK_VOXELS, dtype=torch.int32, device=self.device)
        fresh = torch.ones(n, dtype=torch.bool, device=self.device)
        if old.shape[0]:
            slot = self.table.reshape(-1)[old.long()].long()           # where the bricks that were there have moved
            acc[:, slot] = self.acc
            fresh[slot] = False
        self.acc = acc
        return torch.nonzero(fresh).reshape(-1).to(torch.int32)

    def _apply(self, items, slots=None):
        """items: (LiveRecord, subtract) pairs -> launches of <= 16 views that share an image size and a gate, over `slots` (None: all)"""
        if self.n_bricks == 0 or not items:
            return
        groups = {}
        for rec, sub in items:
            groups.setdefault(rec.launch_key(), []).append((rec, sub))
        for group in groups.values():
            for a in range(0, len(group), ops.TSDF_MAX_VIEWS):
                part = group[a:a + ops.TSDF_MAX_VIEWS]
                recs = [r for r, _ in part]
                r0 = recs[0]
                ops.tsdf_live_integrate(
                    self.acc, self.bricks, self.dims, self.origin, self.voxel_size, torch.stack([r.depth for r in recs]),
                    torch.stack([r.w2c for r in recs]), torch.stack([r.K for r in recs]), self.trunc, self.depth_max,
                    rgb=torch.stack([r.rgb for r in recs]) if self.colored else None,
                    conf=None if r0.conf is None else torch.stack([r.conf for r in recs]), conf_ds=r0.conf_ds, conf_min=r0.conf_min,
                    slots=slots, subtract_mask=sum(1 << b for b, (_, sub) in enumerate(part) if sub))
        self._planes = None

    def _ids(self, ids, present):
        ids = [int(i) for i in (ids.tolist() if hasattr(ids, "tolist") else ids)]
        if len(set(ids)) != len(ids):
            raise ValueError(f"view ids {ids}: an id is given twice")
        for i in ids:
            if (i in self.records) != present:
                raise ValueError(f"view id {i} is {'not in' if present else 'already in'} the live volume")
        return ids

    # ----------------------------------------------------------------------------------------------------------------- the views
    @torch.no_grad()
    def add(self, ids, depth, w2c, K, rgb=None, conf=None, conf_ds=1, conf_min=None):
        """put B views in under the ids given (integers not in use): the arguments of TSDFVolume.integrate.  The bricks these views need
        are allocated, the ones that are new catch up on every view already in, then the new views go into all bricks."""
        ids = self._ids(ids, present=False)
        if (rgb is not None) != self.colored:
            raise ValueError("a coloured live volume takes every view with rgb, a colourless one takes none with it")
        if len(self.records) + len(ids) > ops.TSDF_LIVE_MAX_VIEWS:
            raise ValueError(f"more than {ops.TSDF_LIVE_MAX_VIEWS} views in a live volume: the int32 accumulators could overflow")
        depth, w2c, K, rgb, conf = _stack(self.device, depth, w2c, K, rgb, conf, conf_min)
        if depth.shape[0] != len(ids):
            raise ValueError(f"{len(ids)} ids, {depth.shape[0]} depth maps")
        depth, w2c, K = depth.clone(), w2c.clone(), K.clone()            # the volume's own copies
        rgb, conf = (None if t is None else t.clone() for t in (rgb, conf))
        ops._tsdf_views("LiveTSDFVolume.add", depth, w2c, "w2c", K, self.voxel_size, self.trunc, None, rgb, conf, conf_ds)
        gate = (int(conf_ds), float(conf_min)) if conf is not None else (1, 0.0)
        new = [LiveRecord(depth[b], w2c[b], K[b], None if rgb is None else rgb[b], None if conf is None else conf[b], *gate)
               for b in range(len(ids))]
        fresh = self._allocate(depth, w2c, K)
        if fresh is not None:
            self._apply([(r, False) for r in self.records.values()], slots=fresh)
        self._apply([(r, False) for r in new])
        self.records.update(zip(ids, new))
        return self

    @torch.no_grad()
    def remove(self, ids):
        """take the views out: one subtracting launch per 16, the exact inverse of what put them in.  Bricks are never freed."""
        ids = self._ids(ids, present=True)
        self._apply([(self.records[i], True) for i in ids])
        for i in ids:
            del self.records[i]
        return self

    @torch.no_grad()
    def update(self, ids, w2c=None, depth=None):
        """re-pose views that are in and / or replace their depth maps (None keeps what is recorded): w2c [B,12] (or [B,3,4] / [B,4,4]),
        depth [B,H,W] of the recorded size.  The bricks the new versions need are allocated and catch up on every record as it stands --
        the old versions of these views included, since the launches that follow take those out of every brick; old (subtracted) and new
        (added) versions then share launches, so a voxel both see is read and written once."""
        ids = self._ids(ids, present=True)
        if not ids or (w2c is None and depth is None):
            return self
        old = [self.records[i] for i in ids]
        B = len(ids)
        if w2c is not None:
            w2c = views.pose_rows(w2c, torch.float32, single=True).reshape(-1, 12).to(self.device).clone()
            if w2c.shape[0] != B:
                raise ValueError(f"{B} ids, {w2c.shape[0]} poses")
        if depth is not None:
            depth = torch.as_tensor(depth).to(self.device, torch.float32)
            depth = (depth[None] if depth.dim() == 2 else depth).clone()
            if depth.shape[0] != B or any(tuple(depth.shape[1:]) != tuple(r.depth.shape) for r in old):
                raise ValueError(f"depth {tuple(depth.shape)}: {B} maps of the recorded size are expected")
        new = [r._replace(w2c=r.w2c if w2c is None else w2c[b], depth=r.depth if depth is None else depth[b]) for b, r in enumerate(old)]
        for key in {r.launch_key() for r in new}:                        # mark takes views of one size at a time
            part = [r for r in new if r.launch_key() == key]
            fresh = self._allocate(torch.stack([r.depth for r in part]), torch.stack([r.w2c for r in part]), torch.stack([r.K for r in part]))
            if fresh is not None:
                self._apply([(r, False) for r in self.records.values()], slots=fresh)
        self._apply([pair for o, n in zip(old, new) for pair in ((o, True), (n, False))])
        self.records.update(zip(ids, new))
        return self

    @torch.no_grad()
    def sync(self, keyframes, n, conf_min=None):
        """bring the volume up to the tracker's keyframe store, keyframe i under id i: keyframes len(records) .. n-1 are added (depth,
        image when the volume is coloured, w2c, intrinsics and, with conf_min, the stored confidence gate, as fuse_keyframes takes them),
        and the keyframes already in whose stored w2c row or depth plane no longer has the recorded bits are updated -- one batched
        comparison on the device and one read-back.  Returns (added, updated); with nothing changed no integrate is launched."""
        kf = keyframes
        n, m = int(n), len(self.records)
        if sorted(self.records) != list(range(m)):
            raise ValueError("sync needs the views in to be keyframes 0 .. m-1")
        if n < m:
            raise ValueError(f"{m} keyframes are in the volume, the store has {n}")
        changed = []
        if m:
            recs = [self.records[i] for i in range(m)]
            dw = (torch.stack([r.w2c for r in recs]).view(torch.int32) != kf.w2c[:m].view(torch.int32)).any(1)
            dd = (torch.stack([r.depth for r in recs]).view(torch.int32) != kf.depth[:m].view(torch.int32)).flatten(1).any(1)
            changed = torch.nonzero(dw | dd).reshape(-1).cpu().tolist()
        if changed:
            idx = torch.as_tensor(changed, device=kf.w2c.device)
            self.update(changed, w2c=kf.w2c[idx], depth=kf.depth[idx])
        if n > m:
            idx = torch.arange(m, n, device=kf.device)
            conf = kf.conf_ds[idx // 5, idx % 5] if conf_min is not None else None
            self.add(range(m, n), kf.depth[m:n], kf.w2c[m:n], kf.intrinsic[m:n].to(kf.device, torch.float32),
                     rgb=kf.image[m:n] if self.colored else None, conf=conf, conf_ds=kf.downsample_ratio, conf_min=conf_min)
        return n - m, len(changed)

    # ------------------------------------------------------------------------------------------------------------ what is read
    @torch.no_grad()
    def resolve(self):
        """(tsdf [nb,512], weight [nb,512], color [3,nb,512]) fp32: the accumulators as the pool planes of SparseTSDFVolume, kept until the
        next add, remove or update"""
        if self._planes is None:
            nb = self.n_bricks
            planes = (torch.empty(nb, ops.TSDF_BRICK_VOXELS, dtype=torch.float32, device=self.device),
                      torch.empty(nb, ops.TSDF_BRICK_VOXELS, dtype=torch.float32, device=self.device),
                      torch.empty(3, nb, ops.TSDF_BRICK_VOXELS, dtype=torch.float32, device=self.device))
            if nb:
                ops.tsdf_live_resolve(self.acc, *planes)
            self._planes = planes
        return self._planes

    def _extract(self, weight_threshold):
        if self.n_bricks == 0:
            return torch.zeros(0, 3, dtype=torch.float32), torch.zeros(0, 3, dtype=torch.uint8), torch.zeros(0, 3, dtype=torch.int32)
        return ops.tsdf_sparse_extract_mesh(*self.resolve(), self.table, self.bricks, self.dims, self.origin, self.voxel_size, weight_threshold)

    def _ray_cast_batch(self, c2w, K, H, W, t_min, t_max, step, weight_threshold=1.0, normals=True, colors=True, count=False):
        if self.n_bricks == 0:                                          # nothing stored: every ray misses
            B, dev = c2w.shape[0], self.device
            return (torch.zeros(B, H, W, dtype=torch.float32, device=dev),
                    torch.zeros(B, H, W, 3, dtype=torch.float32, device=dev) if normals else None,
                    torch.zeros(B, 3, H, W, dtype=torch.uint8, device=dev) if colors else None,
                    torch.zeros(B, H, W, dtype=torch.int32, device=dev) if count else None)
        return ops.tsdf_sparse_ray_cast(*self.resolve(), self.table, self.bricks, self.dims, self.origin, self.voxel_size, c2w, K, H, W, t_min,
                                        t_max, step, weight_threshold=weight_threshold, normals=normals, colors=colors, count=count)

    allocated_mask = SparseTSDFVolume.allocated_mask
    _dense_dims = SparseTSDFVolume._dense_dims

    @torch.no_grad()
    def to_dense_acc(self):
        """int32 [5,Z,Y,X]: the accumulators over the virtual grid, zeros where nothing is allocated (raises above the dense limit)"""
        return torch.stack(_dense_from_bricks(self.bricks, self.brick_dims, self._dense_dims(), tuple(self.acc), (0,) * 5))

    @torch.no_grad()
    def to_dense(self):
        """the resolved planes as SparseTSDFVolume.to_dense lays them out: (tsdf [Z,Y,X], weight [Z,Y,X], color [3,Z,Y,X]), 1 / 0 / 0 where
        nothing is allocated"""
        tsdf, weight, color = self.resolve()
        out = _dense_from_bricks(self.bricks, self.brick_dims, self._dense_dims(), (tsdf, weight, *color), (1.0, 0.0, 0.0, 0.0, 0.0))
        return out[0], out[1], torch.stack(out[2:])


# ------------------------------------------------------------------------------------------------------------------- previews
@torch.no_grad()
def shade(normal, w2c):
    """a normal map of the ray cast as an image: normal [B,H,W,3] (world frame) rotated into each camera's frame by w2c [B,12] (or
    [B,3,4] / [B,4,4]) and mapped (n_cam * 0.5 + 0.5) * 255 -> uint8 [B,H,W,3]; black where the normal is 0 (the ray missed)"""
    B = normal.shape[0]
    R = views.pose_rows(w2c, torch.float32, single=True)[:, :, :3].to(normal.device)
    if R.shape[0] != B:
        raise ValueError(f"shade: {B} normal maps, {R.shape[0]} poses")
    n = torch.einsum("bij,bhwj->bhwi", R, normal)
    img = torch.floor((n * 0.5 + 0.5).clamp(0, 1) * 255 + 0.5).to(torch.uint8)
    return img * (normal != 0).any(-1, keepdim=True)


@torch.no_grad()
def write_previews(volume, w2c, K, H, W, outdir, every=1, first=0, **cast):
    """ray-cast every `every`-th view and write <outdir>/{i:05d}_depth.png (16 bits at DEPTH_SCALE per metre, 0 = no surface),
    {i:05d}_normal.png (shade) and {i:05d}_color.png; i is `first` + the view's index in w2c.  cast: the options of ray_cast.  Returns the
    indices (into w2c) written and the RayCast of those views."""
    import os
    from PIL import Image
    if int(every) < 1:
        raise ValueError("every must be >= 1")
    w = views.pose_rows(w2c, torch.float32, single=True).reshape(-1, 12)
    idx = list(range(0, w.shape[0], int(every)))
    K = views.intrinsics(K, w.shape[0], torch.float32)
    rc = volume.ray_cast(w[idx], K[idx], H, W, normals=True, colors=True, **cast)
    raw = torch.floor(torch.clamp(rc.depth * DEPTH_SCALE, 0, 65535)).cpu().numpy().astype(np.uint16)
    nrm = shade(rc.normal, w[idx]).cpu().numpy()
    col = rc.color.permute(0, 2, 3, 1).contiguous().cpu().numpy()
    os.makedirs(outdir, exist_ok=True)
    for n, i in enumerate(idx):
        Image.fromarray(raw[n]).save(os.path.join(outdir, f"{first + i:05d}_depth.png"))
        Image.fromarray(nrm[n]).save(os.path.join(outdir, f"{first + i:05d}_normal.png"))
        Image.fromarray(col[n]).save(os.path.join(outdir, f"{first + i:05d}_color.png"))
    return idx, rc


# ------------------------------------------------------------------------------------------------------------------------ PLY
def write_ply(path, mesh: Mesh) -> None:
    V, F = len(mesh.vertices), len(mesh.faces)
    vert = np.empty(V, np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")]))
    v = np.asarray(mesh.vertices, np.float32).reshape(V, 3)
    c = np.asarray(mesh.colors, np.uint8).reshape(V, 3) if mesh.colors is not None else np.zeros((V, 3), np.uint8)
    vert["x"], vert["y"], vert["z"] = v[:, 0], v[:, 1], v[:, 2]
    vert["red"], vert["green"], vert["blue"] = c[:, 0], c[:, 1], c[:, 2]
    face = np.empty(F, np.dtype([("n", "u1"), ("idx", "<i4", (3,))]))
    face["n"] = 3
    face["idx"] = np.asarray(mesh.faces, np.int32).reshape(F, 3)
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {V}\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\n"
              f"element face {F}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(vert.tobytes())
        fh.write(face.tobytes())


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "<i2", "int16": "<i2", "ushort": "<u2", "uint16": "<u2",
              "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4", "float": "<f4", "float32": "<f4", "double": "<f8",
              "float64": "<f8"}


def read_ply(path) -> Mesh:
    """binary little-endian PLY with scalar vertex properties (x y z, optional red green blue) and triangle faces"""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    lines = data[:end].decode("ascii").splitlines()
    if "format binary_little_endian 1.0" not in lines:
        raise ValueError(f"{path}: only binary_little_endian PLY is read")
    elements, cur = [], None
    for ln in lines:
        tok = ln.split()
        if tok[:1] == ["element"]:
            cur = [tok[1], int(tok[2]), []]
            elements.append(cur)
        elif tok[:1] == ["property"]:
            cur[2].append(tok[1:])
    off = end + len(b"end_header\n")
    verts = cols = faces = None
    for name, count, props in elements:
        if name == "face":
            if len(props) != 1 or props[0][0] != "list":
                raise ValueError(f"{path}: faces must be one list property")
            dt = np.dtype([("n", _PLY_TYPES[props[0][1]]), ("idx", _PLY_TYPES[props[0][2]], (3,))])
            arr = np.frombuffer(data, dt, count, off)
            if count and not np.all(arr["n"] == 3):
                raise ValueError(f"{path}: only triangle faces are read")
            faces = arr["idx"].astype(np.int32)
        else:
            if any(p[0] == "list" for p in props):
                raise ValueError(f"{path}: list property in element {name}")
            dt = np.dtype([(p[1], _PLY_TYPES[p[0]]) for p in props])
            arr = np.frombuffer(data, dt, count, off)
            if name == "vertex":
                verts = np.stack([arr["x"], arr["y"], arr["z"]], 1).astype(np.float32)
                if "red" in arr.dtype.names:
                    cols = np.stack([arr["red"], arr["green"], arr["blue"]], 1).astype(np.uint8)
        off += dt.itemsize * count
    if verts is None:
        raise ValueError(f"{path}: no vertex element")
    return Mesh(verts, cols if cols is not None else np.zeros((len(verts), 3), np.uint8),
                faces if faces is not None else np.zeros((0, 3), np.int32))


# -------------------------------------------------------------------------------------------------------------------- sources
@torch.no_grad()
def depth_bounds(depth, w2c, K, depth_max):
    """AABB (lo, hi) in world coordinates of the back-projected pixels with 0 < d <= depth_max (None when there is none)"""
    B, H, W = depth.shape
    dev = depth.device
    rows = w2c.reshape(B, 3, 4).double()
    R, t = rows[:, :, :3], rows[:, :, 3]
    K = K.reshape(B, 4).double().to(dev)
    v, u = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    lo = torch.full((3,), math.inf, dtype=torch.float64, device=dev)
    hi = -lo
    for b in range(B):
        d = depth[b].double()
        ok = (d > 0) & (d <= depth_max)
        if not bool(ok.any()):
            continue
        dd = d[ok]
        pc = torch.stack([(u[ok] - K[b, 2]) / K[b, 0] * dd, (v[ok] - K[b, 3]) / K[b, 1] * dd, dd], 1)
        pw = (pc - t[b]) @ R[b]                          # R^T (p - t)
        lo = torch.minimum(lo, pw.min(0).values)
        hi = torch.maximum(hi, pw.max(0).values)
    if not bool(torch.isfinite(lo).all()):
        return None
    return lo.cpu().numpy(), hi.cpu().numpy()


def _fuse(depth, w2c, K, voxel_size, trunc_voxels, depth_max, bounds, max_voxels, device, sparse, consistency=None, **maps):
    """the volume over `bounds` (None: the AABB of the valid depths) with all the views fused; sparse: bricks allocated over all views first.
    consistency: a depth_consistency.ConsistencyOptions -- the depth stack is cross-checked between neighbouring views first and the
    rejected pixels are zeroed before the bounds and the integration see them; the volume's `consistency` is then (pixels kept, pixels
    valid before) as device scalars, None without the filter.  maps: rgb and the confidence gate of integrate()."""
    stats = None
    if consistency is not None:
        from . import depth_consistency
        valid = torch.isfinite(depth) & (depth > 0) & (depth <= depth_max)
        depth, keep = depth_consistency.apply(depth, w2c, K, consistency, depth_max)
        stats = (keep.sum(), valid.sum())
    if bounds is None:
        bounds = depth_bounds(depth, w2c, K, depth_max)
        if bounds is None:
            raise ValueError(f"no depth in (0, {depth_max}]: nothing to fuse")
    if sparse:                                                       # max_voxels caps the dense grid only
        vol = SparseTSDFVolume.from_bounds(bounds[0], bounds[1], voxel_size, trunc_voxels=trunc_voxels, depth_max=depth_max, device=device)
        vol.allocate(depth, w2c, K)
        maps["allocate"] = False
    else:
        vol = TSDFVolume.from_bounds(bounds[0], bounds[1], voxel_size, max_voxels=max_voxels, trunc_voxels=trunc_voxels, depth_max=depth_max,
                                     device=device)
    vol.integrate(depth, w2c, K, **maps)
    vol.consistency = stats
    return vol


@torch.no_grad()
def fuse_keyframes(keyframes, n, voxel_size, trunc_voxels=8.0, depth_max=5.0, conf_min=None, bounds=None, max_voxels=2 ** 30, sparse=False,
                   consistency=None):
    """the tracker's keyframes 0..n-1: depth (s*z at tracking resolution), image, the device world->camera rows and the intrinsics; with
    conf_min, pixels whose stored confidence (conf_ds[i // 5, i % 5], at the store's downsample ratio) is below it are skipped.
    bounds: (lo, hi) or None = the AABB of the valid depths padded by the truncation distance.  sparse: a SparseTSDFVolume (bricks
    allocated over all views, then all views fused) in place of the dense grid; max_voxels does not apply to it.  consistency: a
    depth_consistency.ConsistencyOptions, the multi-view filter of the depth maps ahead of the fusion (None: the maps as they are)."""
    kf = keyframes
    n = int(n)
    if n <= 0:
        raise ValueError("no tracked keyframes to fuse")
    dev = kf.device
    depth = kf.depth[:n].contiguous()
    rgb = kf.image[:n].contiguous()
    w2c = kf.w2c[:n].contiguous()
    K = kf.intrinsic[:n].to(dev, torch.float32).contiguous()
    conf = None
    if conf_min is not None:
        idx = torch.arange(n, device=dev)
        conf = kf.conf_ds[idx // 5, idx % 5].contiguous()
    return _fuse(depth, w2c, K, voxel_size, trunc_voxels, depth_max, bounds, max_voxels, dev, sparse, consistency=consistency, rgb=rgb,
                 conf=conf, conf_ds=kf.downsample_ratio, conf_min=conf_min)


@torch.no_grad()
def render_mapper_views(mapper):
    """per mapper keyframe (sorted): quantised depth [H,W] (metres), colour u8 [3,H,W], w2c rows [12], K [4] -- what the reference's
    eval_rendering_kf writes to renders_kf/{depth,image}_after_opt and tsdf_integrate.py reads back"""
    from .gs_mapper import get_pose, render
    depths, rgbs, w2cs, Ks = [], [], [], []
    for k in sorted(mapper.viewpoints):
        v = mapper.viewpoints[k]
        pkg = render(v, mapper.gaussians, mapper.background)
        image = pkg["render"]
        if getattr(v, "exposure_a", None) is not None:                  # eval_utils.py:123
            image = (image.permute(1, 2, 0) @ v.exposure_a + v.exposure_b).permute(2, 0, 1)
        image = torch.clamp(image, 0.0, 1.0)
        rgbs.append((image * 255).to(torch.uint8))                     # numpy astype(uint8): truncation
        d = pkg["depth"].reshape(image.shape[-2:]).float()
        depths.append(torch.floor(torch.clamp(d * DEPTH_SCALE, 0, 65535)) / DEPTH_SCALE)
        w2cs.append(get_pose(v).detach()[:3, :4].reshape(12).float())
        Ks.append(torch.tensor([v.fx, v.fy, v.cx, v.cy], dtype=torch.float32))
    dev = mapper.device
    return (torch.stack(depths).contiguous(), torch.stack(rgbs).contiguous(), torch.stack(w2cs).contiguous(),
            torch.stack(Ks).to(dev).contiguous())


@torch.no_grad()
def fuse_mapper(mapper, voxel_size, trunc_voxels=8.0, depth_max=5.0, bounds=None, max_voxels=2 ** 30, sparse=False, consistency=None):
    """the reference's source (tsdf_integrate.py over renders_kf/*_after_opt): every mapper keyframe rendered at its refined pose.  The
    intrinsics are the views' own, as the reference passes intrinsics.npy unchanged.  sparse, consistency: as in fuse_keyframes."""
    if not mapper.viewpoints:
        raise ValueError("the mapper has no keyframes to fuse")
    depth, rgb, w2c, K = render_mapper_views(mapper)
    return _fuse(depth, w2c, K, voxel_size, trunc_voxels, depth_max, bounds, max_voxels, mapper.device, sparse, consistency=consistency, rgb=rgb)
