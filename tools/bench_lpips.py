#!/usr/bin/env python3
"""LPIPS micro-benchmark (cut3r_slam_amd/lpips.py, csrc/lpips.hip): milliseconds per image pair, per stage and in total, at 384x512 and
680x1200, for one pair per call (what GSMapper.eval_rendering adds per scored frame) and for `--batch` pairs per call; the achieved
TFLOP/s of each convolution against the 157 TF fp32 roof of the MI355X; and beside it the time of one `render` of the synthetic wall of
tools/bench_gs.py (cut3r_slam_amd/synth.gs_wall_window) at the same image size in the same process.

Method: synthetic weights (real widths), random images; HIP events on the stream between the stages of LPIPS.forward; `--warmup` untimed
calls per shape, then `--repeats` timed calls, the median per stage.  FLOP of a convolution = 2 M K Co (M = output pixels of all images of
the call; padded taps counted, as the kernel multiplies them).  `impl=1` (the same chain as fmaf on the VALU) is timed at one pair per call
for comparison.
usage: python tools/bench_lpips.py [--batch 8] [--repeats 9] [--warmup 2] [--json FILE]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from cut3r_slam_amd import gs_mapper as GM, synth
from cut3r_slam_amd import lpips as LP

ROOF_TF = 157.0


def stage_times(L, a, b, warmup, repeats):
    """median ms per stage over `repeats` calls, and of the whole call"""
    runs = []
    for r in range(warmup + repeats):
        ev = []
        L.forward(a, b, events=ev)
        torch.cuda.synchronize()
        if r >= warmup:
            t = {ev[i][0]: ev[i - 1][1].elapsed_time(ev[i][1]) for i in range(1, len(ev))}
            t["total"] = ev[0][1].elapsed_time(ev[-1][1])
            runs.append(t)
    return {k: statistics.median(x[k] for x in runs) for k in runs[0]}


def conv_flops(n, H, W):
    """name -> FLOP of the convolution for n images of H x W"""
    out = {}
    for l, (_, ci, co, k, stride, pad) in enumerate(LP.LAYERS):
        if LP.POOL_BEFORE[l]:
            H, W = (H - 3) // 2 + 1, (W - 3) // 2 + 1
        H, W = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        out[f"conv{l + 1}"] = 2.0 * n * H * W * k * k * ci * co
    return out


def render_ms(H, W, warmup, repeats, dev):
    focal = 440.0 * W / 512                                    # the wall fills the frame at either size
    packet, _, cfg = synth.gs_wall_window(H, W, focal=focal, device=dev)
    m = GM.GSMapper(cfg, focal, focal, W / 2, H / 2, downsample_ratio=2, device=dev)
    m.run(packet, iterations=5, init_iters=20, gba_per_view=1)
    v = m.viewpoints[sorted(m.viewpoints)[0]]
    ts = []
    with torch.no_grad():
        for r in range(warmup + repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            GM.render(v, m.gaussians, m.background)
            e1.record()
            torch.cuda.synchronize()
            if r >= warmup:
                ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), len(m.gaussians), (int(v.image_height), int(v.image_width))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips needs a GPU")
    dev = "cuda:0"
    sd = LP.synth_lpips_state_dict(0)
    mfma, valu = LP.LPIPS(sd, dev), LP.LPIPS(sd, dev, impl=1)
    g = torch.Generator().manual_seed(0)
    out = {"batch": args.batch, "repeats": args.repeats, "warmup": args.warmup, "roof_tf": ROOF_TF, "sizes": {}}
    for H, W in ((384, 512), (680, 1200)):
        a, b = (torch.rand(args.batch, 3, H, W, generator=g).to(dev) for _ in range(2))
        same = float(mfma(a[0], b[0])) == float(valu(a[0], b[0]))
        res = {"mfma_equals_valu": same}
        for name, L, B in (("mfma_1", mfma, 1), (f"mfma_{args.batch}", mfma, args.batch), ("valu_1", valu, 1)):
            t = stage_times(L, a[:B], b[:B], args.warmup, args.repeats)
            fl = conv_flops(2 * B, H, W)
            row = {"ms_per_pair": {k: v / B for k, v in t.items()}, "conv_tflops": {k: fl[k] / (t[k] * 1e-3) / 1e12 for k in fl},
                   "gflop_per_pair": sum(fl.values()) / B / 1e9}
            res[name] = row
            convs = ", ".join(f"{k} {row['ms_per_pair'][k]:.3f} ms {row['conv_tflops'][k]:.1f} TF ({100 * row['conv_tflops'][k] / ROOF_TF:.0f}%)" for k in fl)
            rest = sum(v for k, v in row["ms_per_pair"].items() if k != "total" and k not in fl)
            print(f"{H}x{W} {name:8s}: {row['ms_per_pair']['total']:.3f} ms per pair ({row['gflop_per_pair']:.1f} GFLOP); {convs}; input + pools + tails {rest:.3f} ms")
        rms, P, size = render_ms(H, W, args.warmup, args.repeats, dev)
        res["render_ms"], res["gaussians"], res["render_size"] = rms, P, list(size)
        print(f"{H}x{W} render of one view ({size[0]}x{size[1]}, {P} Gaussians): {rms:.3f} ms; LPIPS of one pair adds "
              f"{res['mfma_1']['ms_per_pair']['total'] / rms:.2f} x that")
        out["sizes"][f"{H}x{W}"] = res
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w", encoding="utf-8") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
