"""LPIPS (AlexNet) of the rendering evaluation: gaussian/utils/eval_utils.py:29,83,92 and :115,141,150,
LearnedPerceptualImagePatchSimilarity(net_type="alex", normalize=True).

The network is ours (csrc/lpips.hip: five convolutions on the fp32 MFMA, two max-pools, one tail per tap), the weights are the user's files
(load_lpips_weights: weights-only loading, nothing is ever fetched), and the tests run on seeded synthetic weights
(synth_lpips_state_dict).  The arithmetic is one definite order of fp32 operations, restated in tests/lpips_oracle.py:

  input   x = ((2 v - 1) - shift_c) / scale_c, shift (-.030, -.088, -.188), scale (.458, .448, .450)
  conv    acc = bias[co]; acc = fmaf(w[co,ky,kx,ci], x, acc) over (ky, kx, ci), ci fastest; a padded tap is fmaf(w, 0, acc); relu
  tap     ss = fmaf(f_c, f_c, ss); n_c = f_c / sqrt(1e-8 + ss) (norm="torchmetrics") or f_c / (sqrt(ss) + 1e-10) (norm="lpips");
          d = n0_c - n1_c; v = fmaf(lin_c, d d, v) over ascending c
  score   sum over the five taps of the fp64 mean of v

Both normalisation rules, the constants and the slice boundaries are written from knowledge of torchmetrics, lpips and torchvision, none
of which this project can run: parity with torchmetrics itself is unpinned.
"""
from __future__ import annotations

import os
import zlib
from collections import OrderedDict

import numpy as np
import torch

# torchvision AlexNet `features`: index -> (ci, co, kernel, stride, pad); a 3x3 stride-2 max-pool precedes the second and the third
LAYERS = ((0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1), (10, 256, 256, 3, 1, 1))
POOL_BEFORE = (False, True, True, False, False)
MIN_SIZE = 31                     # the smallest H, W at which every tap has a pixel (taps 7x7, 3x3, 1x1, 1x1, 1x1)
NORMS = ("torchmetrics", "lpips")
_SLICE = {0: 1, 3: 2, 6: 3, 8: 4, 10: 5}


def schema():
    """canonical key -> shape (torchvision's `features.*` and the lpips package's `lin{l}.model.1.weight`)"""
    s = OrderedDict()
    for idx, ci, co, k, _, _ in LAYERS:
        s[f"features.{idx}.weight"] = (co, ci, k, k)
        s[f"features.{idx}.bias"] = (co,)
    for l, (_, _, co, _, _, _) in enumerate(LAYERS):
        s[f"lin{l}.model.1.weight"] = (1, co, 1, 1)
    return s


def synth_lpips_state_dict(seed: int = 0) -> "OrderedDict[str, torch.Tensor]":
    """seeded weights at the real widths: convolutions N(0, 2 / fan_in), biases N(0, 0.1^2), lin weights uniform in [0, 1/C) (the trained
    ones are non-negative too); one PCG64 stream per key, so the same seed gives the same bits on any machine"""
    sd = OrderedDict()
    for key, shape in schema().items():
        g = np.random.Generator(np.random.PCG64(np.random.SeedSequence([seed, zlib.crc32(key.encode())])))
        if key.startswith("lin"):
            t = g.random(size=shape, dtype=np.float32) / np.float32(shape[1])
        elif key.endswith("bias"):
            t = np.float32(0.1) * g.standard_normal(size=shape, dtype=np.float32)
        else:
            t = g.standard_normal(size=shape, dtype=np.float32) * np.float32(np.sqrt(2.0 / (shape[1] * shape[2] * shape[3])))
        sd[key] = torch.from_numpy(t.astype(np.float32))
    return sd


def _canonical(key: str):
    """a key of any accepted spelling -> the canonical key, or None for an entry that is not part of the metric"""
    parts = key.split(".")
    while parts and parts[0] in ("module", "net"):
        parts = parts[1:]
    if not parts or parts[0] == "classifier":
        return None
    if parts[0] == "features" and len(parts) == 3 and parts[1].isdigit() and int(parts[1]) in _SLICE and parts[2] in ("weight", "bias"):
        return ".".join(parts)
    if parts[0].startswith("slice") and len(parts) == 3 and parts[1].isdigit() and parts[2] in ("weight", "bias"):
        idx = int(parts[1])
        if idx in _SLICE and parts[0] == f"slice{_SLICE[idx]}":
            return f"features.{idx}.{parts[2]}"
        return None
    if parts[0] == "lins" and len(parts) == 5 and parts[1].isdigit() and parts[2:] == ["model", "1", "weight"] and int(parts[1]) < 5:
        return f"lin{int(parts[1])}.model.1.weight"
    if len(parts) == 4 and parts[0] in [f"lin{l}" for l in range(5)] and parts[1:] == ["model", "1", "weight"]:
        return ".".join(parts)
    return None


def canonical_state_dict(sd) -> "OrderedDict[str, torch.Tensor]":
    """any accepted spelling -> the canonical keys, fp32 host tensors; ValueError naming the first missing or mis-shaped tensor"""
    got = {}
    for k, v in sd.items():
        c = _canonical(k)
        if c is not None and torch.is_tensor(v):
            got[c] = v
    out = OrderedDict()
    for key, shape in schema().items():
        if key not in got:
            raise ValueError(f"LPIPS weights: {key} is missing")
        if tuple(got[key].shape) != shape:
            raise ValueError(f"LPIPS weights: {key} has shape {tuple(got[key].shape)}, expected {shape}")
        out[key] = got[key].detach().to("cpu", torch.float32).contiguous()
    return out


def load_lpips_weights(*paths) -> "OrderedDict[str, torch.Tensor]":
    """the backbone and the lin layers from one or several local files (torchvision's alexnet checkpoint and the lpips package's alex.pth, or
    one file holding both): .safetensors, or .pth read with torch.load(weights_only=True).  Later files override earlier ones."""
    if not paths:
        raise ValueError("LPIPS weights: no file given")
    merged = {}
    for path in paths:
        path = os.fspath(path)
        if not os.path.isfile(path):
            raise FileNotFoundError(f"{path}: no such weights file (this runtime never fetches one)")
        if path.endswith(".safetensors"):
            from safetensors.torch import load_file
            sd = load_file(path, device="cpu")
        else:
            sd = torch.load(path, map_location="cpu", weights_only=True)
            if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
                sd = sd["state_dict"]
        if not isinstance(sd, dict):
            raise ValueError(f"{path}: not a state dict")
        merged.update(sd)
    return canonical_state_dict(merged)


class LPIPS:
    """lpips = LPIPS(state_dict); lpips(a, b) -> float for [3,H,W] images in [0,1], a fp64 [B] tensor for [B,3,H,W].  GPU tensors only.
    impl: the convolution path of ops.lpips_conv (0, the default: the fp32 MFMA; the others exist for the tests and the benchmark)."""

    def __init__(self, state_dict, device="cuda:0", norm="torchmetrics", impl=0):
        if norm not in NORMS:
            raise ValueError(f"norm must be one of {NORMS}")
        sd = canonical_state_dict(state_dict)
        self.device, self.norm, self.impl = torch.device(device), norm, int(impl)
        if self.device.type != "cuda":
            raise ValueError("LPIPS runs on the GPU only (no CPU fallback in the product path)")
        # [co,ci,kh,kw] -> [kh,kw,ci,co]: k = (ky, kx, ci) with ci fastest, co contiguous for the kernel's weight tile.  Host tensors
        # until the first call (_upload), so that the refusals below need no GPU
        self.w = [sd[f"features.{i}.weight"].permute(2, 3, 1, 0).contiguous() for i, *_ in LAYERS]
        self.b = [sd[f"features.{i}.bias"] for i, *_ in LAYERS]
        self.lin = [sd[f"lin{l}.model.1.weight"].reshape(-1).contiguous() for l in range(5)]
        self._on_device = False

    def _upload(self):
        if not self._on_device:
            self.w, self.b, self.lin = ([t.to(self.device) for t in ts] for ts in (self.w, self.b, self.lin))
            self._on_device = True

    def _pair(self, a, b):
        if not (torch.is_tensor(a) and torch.is_tensor(b)):
            raise ValueError("LPIPS: a and b must be tensors")
        if not (a.is_cuda and b.is_cuda):
            raise ValueError("LPIPS: tensors must live on the GPU (no CPU fallback in the product path)")
        if a.shape != b.shape:
            raise ValueError(f"LPIPS: the images differ in shape: {tuple(a.shape)} and {tuple(b.shape)}")
        if a.dim() not in (3, 4) or a.shape[-3] != 3 or not (a.is_floating_point() and b.is_floating_point()):
            raise ValueError("LPIPS: a and b are float [3,H,W] or [B,3,H,W] in [0,1]")
        check_size(a.shape[-2], a.shape[-1])
        a, b = (t.reshape(-1, 3, *t.shape[-2:]).to(self.device, torch.float32).contiguous() for t in (a, b))
        if a.shape[0] == 0:
            raise ValueError("LPIPS: an empty batch")
        return a, b

    def forward(self, a, b, events=None):
        """-> (features [5] of [2B,Hl,Wl,C] (first images, then second images), v [5] of [B,Hl,Wl], score fp64 [B]).  events: a list that
        receives one recorded (name, torch.cuda.Event) per stage (tools/bench_lpips.py)."""
        from . import ops

        def mark(name):
            if events is not None:
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                events.append((name, e))
        a, b = self._pair(a, b)
        self._upload()
        score = torch.empty(a.shape[0], dtype=torch.float64, device=self.device)
        mark("start")
        x = ops.lpips_input(a, b)
        mark("input")
        feats, vs = [], []
        for l, (_, _, _, _, stride, pad) in enumerate(LAYERS):
            if POOL_BEFORE[l]:
                x = ops.lpips_pool(x)
                mark(f"pool{l + 1}")
            x = ops.lpips_conv(x, self.w[l], self.b[l], stride, pad, self.impl)
            mark(f"conv{l + 1}")
            feats.append(x)
        for l in range(5):
            vs.append(ops.lpips_tail(feats[l], self.lin[l], score, accumulate=l > 0, norm=self.norm))
            mark(f"tail{l + 1}")
        return feats, vs, score

    def maps(self, a, b):
        """the five feature pairs [(f_a, f_b)] as [B,Hl,Wl,C] (a single pair: [Hl,Wl,C]) and the five v_l [B,Hl,Wl] ([Hl,Wl])"""
        single = a.dim() == 3
        feats, vs, _ = self.forward(a, b)
        B = vs[0].shape[0]
        pairs = [(f[:B], f[B:]) for f in feats]
        if single:
            return [(p[0], q[0]) for p, q in pairs], [v[0] for v in vs]
        return pairs, vs

    def __call__(self, a, b):
        single = torch.is_tensor(a) and a.dim() == 3
        score = self.forward(a, b)[2]
        return float(score[0]) if single else score


def check_size(H, W):
    if int(H) < MIN_SIZE or int(W) < MIN_SIZE:
        raise ValueError(f"LPIPS needs images of at least {MIN_SIZE}x{MIN_SIZE} pixels (the last taps would be empty), got {int(H)}x{int(W)}")


# ---- command line: re-score a directory of renderings (renders/image_after_opt) against its frames
def _read(path, device):
    from PIL import Image
    with Image.open(path) as im:
        x = np.array(im.convert("RGB"), dtype=np.uint8)          # a copy: torch wants a writable array
    return (torch.from_numpy(x).to(device).permute(2, 0, 1).float() / 255.0).contiguous()


def score_paths(lpips, a, b):
    """[(name_a, name_b, value)] of two image files, or of two directories paired by natural-sorted name"""
    from .stream import natsorted
    if os.path.isdir(a) != os.path.isdir(b):
        raise ValueError("A and B are two images or two directories")
    if os.path.isdir(a):
        na, nb = natsorted(os.listdir(a)), natsorted(os.listdir(b))
        if len(na) != len(nb) or not na:
            raise ValueError(f"{a} holds {len(na)} files and {b} holds {len(nb)}: nothing to pair")
        pairs = [(os.path.join(a, x), os.path.join(b, y)) for x, y in zip(na, nb)]
    else:
        pairs = [(a, b)]
    return [(pa, pb, lpips(_read(pa, lpips.device), _read(pb, lpips.device))) for pa, pb in pairs]


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="LPIPS (AlexNet) of two images, or of two directories paired by natural-sorted name")
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--weights", nargs="+", required=True, help="local .safetensors / .pth files with the AlexNet features and the lin layers")
    ap.add_argument("--norm", choices=NORMS, default="torchmetrics")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    lp = LPIPS(load_lpips_weights(*args.weights), args.device, args.norm)
    rows = score_paths(lp, args.a, args.b)
    for pa, pb, v in rows:
        print(f"{os.path.basename(pa)} {os.path.basename(pb)} {v:.6f}")
    print(f"mean_lpips {sum(r[2] for r in rows) / len(rows):.6f}")
    return rows


if __name__ == "__main__":
    main()
