#!/usr/bin/env python3
"""TSDF fusion and mesh extraction (csrc/tsdf.hip) on a synthetic six-walled room: 300 depth + colour views at 384x512 from inside
a 6 x 5 x 3 m box, fused at each voxel size (default 0.02 m and 0.006 m, the finest setting of scripts/run_replica.py:44).

Per voxel size: integration time of the 300 views at B = 1 (300 launches) and B = 16 (19 launches), voxel-view updates/s, effective
HBM bytes/s against the measured 6.3 TB/s (bytes = 40 B read + written per voxel a launch updates + the images it reads), and the
extraction entry points (count + two scans, totals read-back, emit).  With --sparse also the sparse brick volume
(csrc/tsdf_sparse.hip) on the same views: bricks allocated against the minimal set (the bricks holding a voxel with tsdf < 0 or one of
its 26 neighbours, from the dense volume), bytes against the dense 38 B per voxel, allocation / integration / extraction times, and
whether its mesh has the dense mesh's vertex and face counts.  Host clock around work that ends in a device synchronise,
after a warm-up of every shape; best of --reps.  Kernel-level split of count / scan / emit: run under `rocprofv3 --kernel-trace --stats`.
usage: python tools/bench_tsdf.py [--voxel 0.02 0.006] [--views 300] [--reps 2] [--sparse] [--json out.json]"""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cut3r_slam_amd import _lib, ops
from cut3r_slam_amd.tsdf import SparseTSDFVolume, TSDFVolume

HBM_TBS = 6.3          # measured float4 copy rate of the MI355X (MI355X_MICROARCH: 6.29 TB/s)
ROOM = (6.0, 5.0, 3.0)
DEV = "cuda:0"


def look_dirs(n, g):
    """world->camera rows [n,12] and camera centres: positions inside the room, yaw all round, pitch within +-25 degrees"""
    rows, eyes = [], []
    for _ in range(n):
        eye = np.array([g.uniform(0.8, ROOM[0] - 0.8), g.uniform(0.8, ROOM[1] - 0.8), g.uniform(0.9, ROOM[2] - 0.9)])
        yaw, pitch = g.uniform(0, 2 * math.pi), g.uniform(-0.45, 0.45)
        z = np.array([math.cos(yaw) * math.cos(pitch), math.sin(yaw) * math.cos(pitch), math.sin(pitch)])
        x = np.cross(z, (0.0, 0.0, 1.0))
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        R = np.stack([x, y, z])
        rows.append(np.concatenate([R, (-R @ eye)[:, None]], 1).reshape(12))
        eyes.append(eye)
    return np.asarray(rows, np.float32), np.asarray(eyes)


@torch.no_grad()
def render_room(w2c, H, W, f):
    """z-depth [B,H,W] of the inside of the box and a colour u8 [B,3,H,W] that varies over the walls (float64 ray casts on the GPU)"""
    B = w2c.shape[0]
    rows = torch.from_numpy(w2c.astype(np.float64)).to(DEV).reshape(B, 3, 4)
    R, t = rows[:, :, :3], rows[:, :, 3]
    v, u = torch.meshgrid(torch.arange(H, device=DEV, dtype=torch.float64), torch.arange(W, device=DEV, dtype=torch.float64), indexing="ij")
    dc = torch.stack([(u - (W - 1) / 2) / f, (v - (H - 1) / 2) / f, torch.ones_like(u)], -1)        # [H,W,3], z = 1
    depth = torch.empty(B, H, W, dtype=torch.float32, device=DEV)
    rgb = torch.empty(B, 3, H, W, dtype=torch.uint8, device=DEV)
    hi = torch.tensor(ROOM, dtype=torch.float64, device=DEV)
    for b in range(B):
        eye = -R[b].T @ t[b]
        dw = dc @ R[b]                                                   # R^T d
        with torch.no_grad():
            tt = torch.where(dw > 0, (hi - eye) / dw, torch.where(dw < 0, -eye / dw, torch.full_like(dw, math.inf)))
        s = tt.min(-1).values                                            # first wall hit; z-depth = s (ray z = 1)
        p = eye + s[..., None] * dw
        depth[b] = s.float()
        col = torch.stack([127.5 + 100 * torch.sin(3 * p[..., 0] + p[..., 2]), 127.5 + 100 * torch.cos(2 * p[..., 1]),
                           127.5 + 100 * torch.sin(4 * p[..., 2] + p[..., 0])])
        rgb[b] = col.round().clamp(0, 255).to(torch.uint8)
    return depth, rgb


def timed(fn, reps):
    best = math.inf
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def touched_bytes(vol, depth, w2c, K, rgb, B):
    """bytes a run at batch B moves: 40 B per voxel updated by a launch (20 B read + 20 B written), + the pixels each launch reads"""
    vol.tsdf.fill_(1.0)
    vol.weight.zero_()
    vol.color.zero_()
    touched = 0
    n = depth.shape[0]
    for a in range(0, n, B):
        before = vol.weight.clone()
        ops.tsdf_integrate(vol.tsdf, vol.weight, vol.color, vol.origin, vol.voxel_size, depth[a:a + B], w2c[a:a + B], K[a:a + B], vol.trunc,
                           vol.depth_max, rgb=rgb[a:a + B])
        touched += int((vol.weight != before).sum())
        del before
    H, W = depth.shape[1:]
    return 40 * touched + n * H * W * 7, touched, float(vol.weight.double().sum())


@torch.no_grad()
def minimal_bricks(tsdf):
    """bricks of 8^3 voxels that hold a voxel with tsdf < 0 or one of its 26 neighbours"""
    need = tsdf < 0
    for ax in range(3):                                                  # the 3x3x3 dilation, one axis at a time
        grown = need.clone()
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        grown[tuple(lo)] |= need[tuple(hi)]
        grown[tuple(hi)] |= need[tuple(lo)]
        need = grown
    Z, Y, X = need.shape
    need = torch.nn.functional.pad(need, (0, -X % 8, 0, -Y % 8, 0, -Z % 8))
    Z, Y, X = need.shape
    return int(need.reshape(Z // 8, 8, Y // 8, 8, X // 8, 8).any(5).any(3).any(1).sum())


def bench_sparse(vol, nv, nf, depth, rgb, w2c, K, reps):
    """the sparse volume on the lattice of the dense `vol` (which holds the fused views): allocate all views, integrate at B = 16, extract"""
    n = depth.shape[0]
    X, Y, Z = vol.dims
    made = []

    def fresh():
        made[:] = [SparseTSDFVolume(vol.origin, vol.voxel_size, vol.dims, depth_max=vol.depth_max, device=DEV)]

    def allocate():
        fresh()
        made[0].allocate(depth, w2c, K)

    def both():
        allocate()
        made[0].integrate(depth, w2c, K, rgb=rgb, allocate=False)

    both()                                                               # warm-up
    t_fresh = timed(fresh, reps)
    t_alloc = timed(allocate, reps) - t_fresh
    t_both = timed(both, reps) - t_fresh
    sp = made[0]
    t_ext = timed(lambda: sp.extract_mesh(1.0), reps)
    mesh = sp.extract_mesh(1.0)
    ws = _lib.load().cut3r_tsdf_sparse_mesh_workspace_bytes(sp.n_bricks)
    need = minimal_bricks(vol.tsdf)
    dense_bytes = 38 * X * Y * Z
    return {"bricks": sp.n_bricks, "table_entries": sp.table.numel(), "minimal_bricks": need, "allocated_over_minimal": round(sp.n_bricks / need, 3),
            "fraction_of_grid_allocated": round(sp.n_bricks / sp.table.numel(), 4), "pool_and_table_GB": round(sp.nbytes / 1e9, 3),
            "workspace_GB": round(ws / 1e9, 3), "total_over_dense_38B_per_voxel": round((sp.nbytes + ws) / dense_bytes, 4),
            "allocate_ms": round(1e3 * t_alloc, 2), "integrate_B16_ms": round(1e3 * (t_both - t_alloc), 2),
            "allocate_plus_integrate_ms": round(1e3 * t_both, 2), "extract_mesh_ms_incl_allocation_and_host_copy": round(1e3 * t_ext, 2),
            "vertices": len(mesh.vertices), "faces": len(mesh.faces), "same_counts_as_dense": len(mesh.vertices) == nv and len(mesh.faces) == nf}


def bench_voxel(voxel, depth, rgb, w2c, K, reps, sparse=False):
    pad = 8 * voxel
    vol = TSDFVolume.from_bounds((0, 0, 0), ROOM, voxel, pad=pad, max_voxels=2 ** 31 - 1, device=DEV)
    X, Y, Z = vol.dims
    N = X * Y * Z
    n = depth.shape[0]
    out = {"voxel_m": voxel, "dims": [X, Y, Z], "voxels": N, "volume_GB": round(vol.nbytes / 1e9, 2), "trunc_m": vol.trunc}

    def run(B):
        def f():
            vol.tsdf.fill_(1.0)
            vol.weight.zero_()
            vol.color.zero_()
            torch.cuda.synchronize()
            for a in range(0, n, B):
                ops.tsdf_integrate(vol.tsdf, vol.weight, vol.color, vol.origin, vol.voxel_size, depth[a:a + B], w2c[a:a + B], K[a:a + B],
                                   vol.trunc, vol.depth_max, rgb=rgb[a:a + B])
        return f

    def reset_time():
        vol.tsdf.fill_(1.0)
        vol.weight.zero_()
        vol.color.zero_()

    t_reset = timed(reset_time, reps)
    for B in (1, 16):
        run(B)()                                                         # warm-up of the shape
        t = timed(run(B), reps) - t_reset
        nbytes, touched, updates = touched_bytes(vol, depth, w2c, K, rgb, B)
        out[f"B{B}"] = {"launches": (n + B - 1) // B, "integrate_ms": round(1e3 * t, 2), "voxel_view_updates": int(updates),
                        "updates_per_s": float(f"{updates / t:.4g}"), "voxels_touched_per_launch_sum": touched,
                        "effective_GBps": round(nbytes / t / 1e9, 1), "fraction_of_6.3TBps": round(nbytes / t / 1e12 / HBM_TBS, 3),
                        "grid_visits_per_s": float(f"{N * ((n + B - 1) // B) / t:.4g}")}
    run(16)()
    lib = _lib.load()
    nbytes = lib.cut3r_tsdf_mesh_workspace_bytes(X, Y, Z)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    totals = torch.empty(2, dtype=torch.int64, device=DEV)
    s = ops._stream()

    def count():
        _lib.check(lib.cut3r_tsdf_mesh_count(ops._p(vol.tsdf), ops._p(vol.weight), X, Y, Z, 1.0, ops._p(ws), nbytes, ops._p(totals), s), "count")

    count()
    nv, nf = (int(v) for v in totals.cpu())
    verts = torch.empty(nv, 3, device=DEV)
    cols = torch.empty(nv, 3, dtype=torch.uint8, device=DEV)
    faces = torch.empty(nf, 3, dtype=torch.int32, device=DEV)

    def emit():
        _lib.check(lib.cut3r_tsdf_mesh_emit(ops._p(vol.tsdf), ops._p(vol.color), X, Y, Z, *[float(o) for o in vol.origin], vol.voxel_size,
                                            ops._p(ws), nbytes, ops._p(verts), ops._p(cols), ops._p(faces), nv, nf, s), "emit")

    emit()
    t_count = timed(count, reps)
    t_emit = timed(emit, reps)
    t_all = timed(lambda: vol.extract_mesh(1.0), reps)
    out["extract"] = {"vertices": nv, "faces": nf, "workspace_GB": round(nbytes / 1e9, 2), "count_and_scans_ms": round(1e3 * t_count, 2),
                      "emit_ms": round(1e3 * t_emit, 2), "extract_mesh_ms_incl_allocation_and_host_copy": round(1e3 * t_all, 2),
                      "count_pass_GBps_lower_bound": round(N * 10 / t_count / 1e9, 1)}
    del ws, verts, cols, faces
    if sparse:
        torch.cuda.empty_cache()
        out["sparse"] = bench_sparse(vol, nv, nf, depth, rgb, w2c, K, reps)
    del vol
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel", type=float, nargs="+", default=[0.02, 0.006])
    ap.add_argument("--views", type=int, default=300)
    ap.add_argument("--size", type=int, nargs=2, default=[384, 512])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--sparse", action="store_true", help="also the sparse brick volume on the same views")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf needs the GPU")
    H, W = args.size
    f = W / 2.0                                                          # 90 degree horizontal field of view
    g = np.random.default_rng(0)
    w2c_np, _ = look_dirs(args.views, g)
    depth, rgb = render_room(w2c_np, H, W, f)
    w2c = torch.from_numpy(w2c_np).to(DEV)
    K = torch.tensor([[f, f, (W - 1) / 2, (H - 1) / 2]], dtype=torch.float32, device=DEV).expand(args.views, 4).contiguous()
    res = {"scene": f"six-walled room {ROOM[0]} x {ROOM[1]} x {ROOM[2]} m, {args.views} views at {W}x{H}, f = {f:g}, trunc = 8 voxels",
           "device": torch.cuda.get_device_name(0), "results": []}
    for v in args.voxel:
        r = bench_voxel(v, depth, rgb, w2c, K, args.reps, args.sparse)
        res["results"].append(r)
        print(json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
