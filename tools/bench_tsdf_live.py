#!/usr/bin/env python3
"""The live TSDF volume (csrc/tsdf_live.hip, tsdf.LiveTSDFVolume) on a Replica-shaped synthetic keyframe store: the six-walled room of
tools/bench_tsdf.py, --views keyframes (default 300) of 384x512 at voxel 0.02, added in windows of 5 as a run would add them.

Reports, from device events after a warm-up: the time of one add() of a 5-keyframe window at the start, the middle and the end of the
run; next to each, what a user has to do without the live volume to get a current model at that moment -- fuse_keyframes(sparse=True) of
all keyframes present; an update() of 16 and of 128 keyframes (poses nudged); resolve + mesh extraction; and the share of the whole run
spent in pool regrowth (LiveTSDFVolume._regrow: a copy of the whole pool per allocation).
usage: python tools/bench_tsdf_live.py [--views 300] [--voxel 0.02] [--json out.json]"""
import argparse
import json
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from bench_tsdf import DEV, ROOM, look_dirs, render_room
from cut3r_slam_amd.tsdf import LiveTSDFVolume, fuse_keyframes

WINDOW = 5


class Timer:
    """device-event times in ms, summed per name"""

    def __init__(self):
        self.spans = []

    def __call__(self, name, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        self.spans.append((name, a, b))
        return out

    def totals(self):
        torch.cuda.synchronize()
        out = {}
        for name, a, b in self.spans:
            out.setdefault(name, []).append(a.elapsed_time(b))
        return out


def run(store, n, voxel, timer, checkpoints):
    centre = np.asarray(ROOM) / 2
    vol = LiveTSDFVolume.around(centre, max(ROOM) / 2 + 8 * voxel, voxel, device=DEV)
    regrow = vol._regrow
    vol._regrow = lambda old, nb: timer("regrow", lambda: regrow(old, nb))
    for a in range(0, n, WINDOW):
        b = min(n, a + WINDOW)
        timer(f"add@{a}", lambda: vol.sync(store, b))
        if a in checkpoints:
            timer(f"fuse_keyframes_sparse@{b}", lambda: fuse_keyframes(store, b, voxel, sparse=True))
    return vol


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=300)
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--size", type=int, nargs=2, default=[384, 512])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf_live needs the GPU")
    H, W = args.size
    n, f = args.views, W / 2.0
    w2c_np, _ = look_dirs(n, np.random.default_rng(0))
    depth, rgb = render_room(w2c_np, H, W, f)
    store = types.SimpleNamespace(device=torch.device(DEV), depth=depth, image=rgb, w2c=torch.from_numpy(w2c_np).to(DEV), downsample_ratio=2,
                                  intrinsic=torch.tensor([[f, f, (W - 1) / 2, (H - 1) / 2]], dtype=torch.float32).expand(n, 4).contiguous(),
                                  conf_ds=None)
    last = (n - 1) // WINDOW * WINDOW
    checkpoints = (0, last // 2 // WINDOW * WINDOW, last)
    warm = run(store, min(n, 4 * WINDOW), args.voxel, Timer(), (0,))                 # warm-up of every kernel and allocator path
    warm.update([0, 1], w2c=store.w2c[:2] * 1.0)
    warm.extract_mesh(1.0)
    del warm
    timer = Timer()
    whole = timer("run", lambda: run(store, n, args.voxel, timer, checkpoints))
    for k in (16, 128):
        if k <= n:
            ids = list(range(0, k))
            moved = store.w2c[:k].clone()
            moved[:, 3] += 0.01                                                      # 1 cm along the camera's x axis
            timer(f"update_{k}", lambda: whole.update(ids, w2c=moved))
    timer("resolve", lambda: whole.resolve())
    mesh = timer("extract_mesh_after_resolve", lambda: whole.extract_mesh(1.0))
    t = timer.totals()
    fused = sum(sum(v) for k, v in t.items() if k.startswith("fuse_keyframes"))
    res = {"scene": f"six-walled room {ROOM[0]} x {ROOM[1]} x {ROOM[2]} m, {n} keyframes at {W}x{H}, voxel {args.voxel:g}, windows of {WINDOW}",
           "device": torch.cuda.get_device_name(0), "bricks": whole.n_bricks, "table_entries": whole.table.numel(),
           "volume_GB": round(whole.nbytes / 1e9, 3), "vertices": len(mesh.vertices), "faces": len(mesh.faces)}
    for name, a in zip(("first", "middle", "last"), checkpoints):
        b = min(n, a + WINDOW)
        res[f"add_{name}_window_ms"] = round(t[f"add@{a}"][0], 3)
        res[f"fuse_keyframes_sparse_of_{b}_ms"] = round(t[f"fuse_keyframes_sparse@{b}"][0], 3)
    adds = sum(sum(v) for k, v in t.items() if k.startswith("add@"))
    res.update({"all_adds_ms": round(adds, 2), "regrow_ms": round(sum(t.get("regrow", [0.0])), 2), "regrow_calls": len(t.get("regrow", [])),
                "regrow_share_of_adds": round(sum(t.get("regrow", [0.0])) / adds, 4), "run_ms_incl_the_three_fusions": round(t["run"][0], 2),
                "the_three_fusions_ms": round(fused, 2)})
    for k in (16, 128):
        if f"update_{k}" in t:
            res[f"update_{k}_ms"] = round(t[f"update_{k}"][0], 3)
    res["resolve_ms"] = round(t["resolve"][0], 3)
    res["extract_mesh_ms_incl_host_copy"] = round(t["extract_mesh_after_resolve"][0], 3)
    print(json.dumps(res), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
