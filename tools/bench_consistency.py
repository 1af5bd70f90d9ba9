#!/usr/bin/env python3
"""Multi-view depth consistency (csrc/consistency.hip, cut3r_slam_amd/depth_consistency.py) at tracking resolution: --views (64) keyframe
depth maps of 384 x 512 of the box room of tests/consistency_oracle.py along its camera walk (analytic depths, 3 % floaters), checked with
window 2 (S = 4 sources) and window 4 (S = 8), without and with the averaged depth.

Times (device events around synchronised work, after a warm-up; best of --reps): the kernel alone (the tables already on the device, one
launch over all views), ops.depth_consistency (with the upload of the tables) and depth_consistency.filter_depths (with the torch masking).
With each kernel time the memory floor: every view's depth plane read once as reference and once per source, (1 + S) x 4 B a pixel, and the
two u8 planes (+ the fp32 average) written, at the measured 6.3 TB/s of the MI355X; neighbouring views share their source planes through
the caches, so the kernel can come in under this count of bytes only by that reuse.
usage: python tools/bench_consistency.py [--views 64] [--size 384 512] [--reps 5] [--json out.json]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cut3r_slam_amd import _lib, ops
from cut3r_slam_amd import depth_consistency as DC
from tests import consistency_oracle as O

DEV = "cuda:0"
HBM_TBS = 6.3          # measured float4 copy rate of the MI355X
DEPTH_MAX = 10.0


def timed(fn, reps):
    """best of reps, ms, by device events around fn (the stream is idle before and after), after one warm-up"""
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def walk(n):
    """the box room's camera walk of 7 views stretched over n views"""
    t = np.linspace(0.0, 6.0, n)
    c = np.stack([0.12 * (t - 3), 0.04 * np.cos(t), -0.5 + 0.05 * t], 1)
    return c, np.stack([O.rot_yaw_pitch(0.08 * (k - 3), 0.03 * np.sin(k)) for k in t])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--size", type=int, nargs=2, default=[384, 512])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_consistency needs a GPU: a time measured anywhere else says nothing")
    H, W = a.size
    n = a.views
    f = 0.5 * W
    K = np.tile(np.array([f, f, (W - 1) / 2, (H - 1) / 2], np.float32), (n, 1))
    c, Rm = walk(n)
    depth, mask = O.inject_floaters(O.room_depth(c, Rm, K, H, W), 0.03, 0)
    w2c = O.w2c_rows(c, Rm)
    d = torch.from_numpy(depth).to(DEV)
    k = torch.from_numpy(K).to(DEV)
    lib = _lib.load()
    r = {"views": n, "H": H, "W": W, "hbm_TBps": HBM_TBS, "floaters": int(mask.sum())}
    for window in (2, 4):
        src = DC.neighbour_table(n, window)
        S = src.shape[1]
        ref = np.arange(n, dtype=np.int32)
        fwd, bwd = DC.relative_rows(w2c, ref, src)
        ref_d, src_d = torch.from_numpy(ref).to(DEV), torch.from_numpy(src).to(DEV)
        fwd_d, bwd_d = torch.from_numpy(fwd).to(DEV), torch.from_numpy(bwd).to(DEV)
        sup = torch.empty(n, H, W, dtype=torch.uint8, device=DEV)
        vio = torch.empty_like(sup)
        avg = torch.empty(n, H, W, dtype=torch.float32, device=DEV)
        p = lambda t: C.c_void_p(t.data_ptr())
        pairs = int((src >= 0).sum())
        for average in (False, True):
            def kernel():
                ops.check(lib.cut3r_depth_consistency(p(d), p(k), n, H, W, p(ref_d), p(src_d), n, S, p(fwd_d), p(bwd_d), DEPTH_MAX, 1.0, 0.01,
                                                      1e-3, p(sup), p(vio), p(avg) if average else C.c_void_p(0), ops._stream()),
                          "cut3r_depth_consistency")
            ms = timed(kernel, a.reps)
            # the floor counts the sources a view really has (the ends of the walk have fewer)
            nbytes = H * W * (4 * (n + pairs) + n * (2 + (4 if average else 0)))
            floor_ms = nbytes / (HBM_TBS * 1e12) * 1e3
            tag = f"w{window}{'_avg' if average else ''}"
            r[tag] = {"S": S, "pairs": pairs, "kernel_ms": ms, "us_per_keyframe": 1e3 * ms / n, "bytes": nbytes, "floor_ms": floor_ms,
                      "ratio_to_floor": ms / floor_ms, "effective_GBps": nbytes / ms / 1e6}
            r[tag]["op_ms"] = timed(lambda: ops.depth_consistency(d, k, ref, src, fwd, bwd, DEPTH_MAX, average=average), a.reps)
            r[tag]["filter_depths_ms"] = timed(lambda: DC.filter_depths(d, w2c, k, window=window, depth_max=DEPTH_MAX, average=average), a.reps)
        _, keep = DC.filter_depths(d, w2c, k, window=window, depth_max=DEPTH_MAX)
        m = torch.from_numpy(mask).to(DEV)
        r[f"w{window}"]["kept_clean"] = float(keep[~m].float().mean())
        r[f"w{window}"]["kept_floaters"] = float(keep[m].float().mean())
        print(f"[bench_consistency] window {window}: " + json.dumps(r[f"w{window}"]), file=sys.stderr, flush=True)
    print(json.dumps(r))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(r, fh, indent=1)


if __name__ == "__main__":
    main()
