"""numpy restatement of the LPIPS contract (cut3r_slam_amd/lpips.py, csrc/lpips.hip), operation by operation in fp32, with an exact fp32
fused multiply-add.  Not a test module: tests/test_lpips_cpu.py checks it against an independent fp64 formulation, tests/test_lpips_gpu.py
compares the kernels with it bit for bit.

fma32(a, b, c): the product of two fp32 numbers is exact in fp64 (48 bits); the fp64 sum of product and addend is rounded to ODD (TwoSum
gives the exact residual: when it is non-zero and the sum's last bit is even, the sum moves one ulp towards the residual), and a value
rounded to odd at 53 bits rounds to fp32 exactly as the unrounded value would (53 >= 2 * 24 + 2)."""
import numpy as np

LAYERS = ((0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1), (10, 256, 256, 3, 1, 1))
POOL_BEFORE = (False, True, True, False, False)
SHIFT = np.array([-.030, -.088, -.188], np.float32)
SCALE = np.array([.458, .448, .450], np.float32)
f32 = np.float32


def fma32(a, b, c):
    a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0) & even & np.isfinite(s)
    if fix.any():
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(f32)


def transform(img):
    """[3,H,W] in [0,1] -> channels-last [H,W,3]"""
    v = np.ascontiguousarray(np.asarray(img, f32).transpose(1, 2, 0))
    return ((f32(2) * v - f32(1)) - SHIFT) / SCALE


def conv_relu(x, w, bias, stride, pad):
    """x [H,W,Ci], w [Co,Ci,KH,KW] (the checkpoint's layout), bias [Co] -> [Ho,Wo,Co]: the chain over (ky, kx, ci) from the bias"""
    H, W, Ci = x.shape
    Co, _, KH, KW = w.shape
    Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    xp = np.zeros((H + 2 * pad, W + 2 * pad, Ci), f32)
    xp[pad:pad + H, pad:pad + W] = x
    acc = np.broadcast_to(np.asarray(bias, f32), (Ho, Wo, Co)).copy()
    for ky in range(KH):
        for kx in range(KW):
            win = xp[ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]       # [Ho,Wo,Ci]
            for ci in range(Ci):
                acc = fma32(w[:, ci, ky, kx][None, None, :], win[:, :, ci:ci + 1], acc)
    return np.maximum(acc, f32(0))


def pool(x):
    H, W, _ = x.shape
    Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    out = None
    for dy in range(3):
        for dx in range(3):
            win = x[dy:dy + 2 * (Ho - 1) + 1:2, dx:dx + 2 * (Wo - 1) + 1:2]
            out = win.copy() if out is None else np.maximum(out, win)
    return out


def features(sd, img):
    x = transform(img)
    out = []
    for l, (idx, _, _, _, stride, pad) in enumerate(LAYERS):
        if POOL_BEFORE[l]:
            x = pool(x)
        x = conv_relu(x, np.asarray(sd[f"features.{idx}.weight"], f32), np.asarray(sd[f"features.{idx}.bias"], f32), stride, pad)
        out.append(x)
    return out


def tap(f0, f1, lin, norm="torchmetrics"):
    """f0, f1 [H,W,C], lin [C] -> v [H,W]"""
    C = f0.shape[-1]
    n = []
    for f in (f0, f1):
        ss = np.zeros(f.shape[:2], f32)
        for c in range(C):
            ss = fma32(f[..., c], f[..., c], ss)
        den = np.sqrt(f32(1e-8) + ss) if norm == "torchmetrics" else np.sqrt(ss) + f32(1e-10)
        n.append(f / den[..., None])
    d = n[0] - n[1]
    q = d * d
    v = np.zeros(f0.shape[:2], f32)
    for c in range(C):
        v = fma32(lin[c], q[..., c], v)
    return v


def lpips(sd, a, b, norm="torchmetrics"):
    """-> (features of a [5], features of b [5], v [5], score (python float, fp64 arithmetic))"""
    sd = {k: np.asarray(v, f32) for k, v in sd.items()}
    fa, fb = features(sd, a), features(sd, b)
    vs = [tap(fa[l], fb[l], sd[f"lin{l}.model.1.weight"].reshape(-1), norm) for l in range(5)]
    score = 0.0
    for v in vs:
        score += float(np.sum(v.astype(np.float64)) / v.size)
    return fa, fb, vs, score
