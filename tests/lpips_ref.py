"""Shared by the LPIPS tests (not a test module): deterministic image pairs, the cached oracle results, and an independent restatement of
the metric in torch on the CPU (F.conv2d / F.max_pool2d, written from the AlexNet architecture and the torchmetrics / lpips rules, not
from tests/lpips_oracle.py) in a chosen precision."""
import numpy as np
import torch
import torch.nn.functional as F

from cut3r_slam_amd.lpips import synth_lpips_state_dict
from tests import lpips_oracle as LO

SIZES = ((31, 31), (35, 47), (67, 95))
SEED = 7
_CACHE = {}


def weights():
    if "sd" not in _CACHE:
        _CACHE["sd"] = synth_lpips_state_dict(SEED)
    return _CACHE["sd"]


def pair(H, W, seed=0):
    """two fp32 images [3,H,W] in [0,1]: a smooth pattern with noise, and a shifted, differently noised version of it (exact 0 and 1 occur)"""
    g = np.random.default_rng([seed, H, W])
    y, x = np.meshgrid(np.linspace(0, 3, H), np.linspace(0, 4, W), indexing="ij")
    base = np.stack([0.5 + 0.5 * np.sin(2 * x + y), 0.5 + 0.5 * np.cos(3 * y - x), 0.5 + 0.5 * np.sin(x * y)])
    a = np.clip(base + 0.3 * g.standard_normal(base.shape), 0, 1).astype(np.float32)
    b = np.clip(np.roll(base, 1, 2) + 0.3 * g.standard_normal(base.shape), 0, 1).astype(np.float32)
    return a, b


def oracle(H, W, norm="torchmetrics"):
    """tests/lpips_oracle.py on pair(H, W), computed once per size (the features serve both norm rules); never modified by a test"""
    key = (H, W)
    if key not in _CACHE:
        a, b = pair(H, W)
        sd = {k: v.numpy() for k, v in weights().items()}
        _CACHE[key] = (LO.features(sd, a), LO.features(sd, b))
    if (H, W, norm) not in _CACHE:
        fa, fb = _CACHE[key]
        vs = [LO.tap(fa[l], fb[l], weights()[f"lin{l}.model.1.weight"].numpy().reshape(-1), norm) for l in range(5)]
        score = 0.0
        for v in vs:
            score += float(np.sum(v.astype(np.float64)) / v.size)
        _CACHE[(H, W, norm)] = (fa, fb, vs, score)
    return _CACHE[(H, W, norm)]


def torch_score(sd, a, b, norm, dtype):
    """the metric as torchmetrics / lpips compute it, in `dtype` on the CPU; the constants are the fp32 values of the contract"""
    t = lambda v: torch.tensor(v, dtype=torch.float32).to(dtype)
    shift, scale = t([-.030, -.088, -.188]).view(1, 3, 1, 1), t([.458, .448, .450]).view(1, 3, 1, 1)
    w = {k: v.to(dtype) for k, v in sd.items()}

    def taps(img):
        x = (2 * torch.as_tensor(img).to(dtype)[None] - 1 - shift) / scale
        out = []
        x = F.relu(F.conv2d(x, w["features.0.weight"], w["features.0.bias"], stride=4, padding=2))
        out.append(x)
        x = F.max_pool2d(x, kernel_size=3, stride=2)
        x = F.relu(F.conv2d(x, w["features.3.weight"], w["features.3.bias"], padding=2))
        out.append(x)
        x = F.max_pool2d(x, kernel_size=3, stride=2)
        for idx in (6, 8, 10):
            x = F.relu(F.conv2d(x, w[f"features.{idx}.weight"], w[f"features.{idx}.bias"], padding=1))
            out.append(x)
        return out

    def unit(f):
        ss = (f ** 2).sum(1, keepdim=True)
        return f / torch.sqrt(t(1e-8) + ss) if norm == "torchmetrics" else f / (torch.sqrt(ss) + t(1e-10))

    score = 0.0
    for l, (f0, f1) in enumerate(zip(taps(a), taps(b))):
        d = (unit(f0) - unit(f1)) ** 2
        score += float(F.conv2d(d, w[f"lin{l}.model.1.weight"]).double().mean())
    return score
