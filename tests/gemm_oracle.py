"""fp64 reference, per-element fp32 error bound and an fp32 emulation (with named mutants) of the GEMM family of csrc/gemm.hip:
Linear (+bias)(+GELU | ReLU)(+res1)(+res2) with fp16 or fp32 residuals and output, 3x3 convolution over NHWC (stride 1 | 2, pad 1,
optional ReLU on load), ConvTranspose with kernel == stride (pixel-shuffle scatter) and batched problems.  CPU only (torch).

Every problem is reduced to  C[z] = epi(A2[z] W[z]^T)  with A2 [Z, M, K] (the im2col matrix of a convolution, K ordered (ky, kx, ci) as
the weight panel is) and W [Z, N, K], both fp16-valued.

The bound (u = 2^-24; derived, not fitted).  Let acc = sum_k a_k w_k and S = sum_k |a_k w_k| of one output element.
  * Products of two fp16 numbers have 22 significant bits: exact in fp32.
  * Accumulator.  v_mfma_f32_16x16x32_f16 adds 32 products to the accumulator per instruction; a row needs ceil(K / 32) of them.  MODEL
    (a supposition about the hardware, not a measurement): inside one instruction the 32-product block sum is formed with one fp32
    rounding and added to the accumulator with another, and either may truncate instead of rounding to nearest (2 u instead of u each):
    4 u times the magnitude of what is being formed, which never exceeds S.  One more term for the zero-padded / first instruction:
        e_acc = 4 u (ceil(K / 32) + 1) S.
    Tile 16 splits K over NW = 4 | 8 waves and adds the partial sums in wave order with ordinary fp32 adds (round to nearest, u each, each
    partial result <= S):  + (NW - 1) u S.
    If correct kernels exceeded this on the GPU, the fall-back is the order-free bound (K - 1) 2^-23 S (any summation order, round to nearest),
    never a refitted constant (DESIGN.md says which one holds).
  * Bias, res1, res2: one round-to-nearest add each, u |result| (the residual operands are exact in fp32); the running error is carried along.
  * GELU(x) = x Phi(x): |GELU'| <= 1.13, so the input error grows by at most that factor; the erf evaluation (erff for fp32 outputs,
    Abramowitz-Stegun 7.1.26 with |error| <= 1.5e-7 = 2.6 u for fp16 outputs, + the rounding of its polynomial) is carried as an ABSOLUTE
    error 4 u of erf, i.e. 0.5 |x| 4 u of the result (absolute, because 1 + erf cancels for x << 0 -- the case the column block shifted to
    -3 is there for); plus one rounding of the product.  ReLU is exact and 1-Lipschitz.
  * fp16 store: 2^-11 |value| + half a subnormal step (2^-25).
Only first-order terms, except that every |value| is taken as |reference| + the error so far (so the bound never relies on the error
being small next to the value)."""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24
C_MFMA = 4.0
K_ERF = 4.0
GELU_LIP = 1.13


# ------------------------------------------------------------------------------------------------ operands -> (A2, W)
def im2col3(x, stride, relu_in=False, mutant=None):
    """x [B, H, W, Cin] -> [B * Ho * Wo, 9 * Cin] with K ordered (ky, kx, ci), pad 1; dtype kept.  Mutants: see MUTANTS."""
    B, H, W, Cin = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if relu_in:
        x = torch.relu(x)
    flat = x.reshape(B * H * W, Cin)
    org = 0 if (mutant == "stride_origin" and stride == 2) else -1
    b = torch.arange(B).view(B, 1, 1)
    oy = torch.arange(Ho).view(1, Ho, 1) * stride + org
    ox = torch.arange(Wo).view(1, 1, Wo) * stride + org
    cols = []
    for ky in range(3):
        for kx in range(3):
            iy, ix = (oy + ky).expand(B, Ho, Wo), (ox + kx).expand(B, Ho, Wo)
            ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            lin = (b * H + iy) * W + ix                              # the flat pixel address an unchecked tap would read
            if mutant == "pad_neighbour":                            # x out of range, y in range: the neighbouring row's pixel
                ok = ok | ((iy >= 0) & (iy < H) & (lin >= 0) & (lin < B * H * W))
            if mutant == "image_border":                             # y out of range: the previous / next image's border row
                ok = ok | ((ix >= 0) & (ix < W) & (lin >= 0) & (lin < B * H * W))
            v = flat[lin.clamp(0, B * H * W - 1).reshape(-1)]
            cols.append(torch.where(ok.reshape(-1, 1), v, torch.zeros_like(v)))
    return torch.cat(cols, dim=1)


def as_gemm(p, mutant=None):
    """problem dict (tests/gemm_cases.py: operands) -> A2 [Z, M, K], W [Z, N, K] (fp16 values, dtype fp16)"""
    if p["kind"] == "conv":
        A2 = im2col3(p["x"], p["stride"], p["relu_in"], mutant).unsqueeze(0)
    else:
        A2 = p["A"]
        if p["relu_in"]:
            A2 = torch.relu(A2)
    W = p["W"]
    if mutant == "relu_w" and p["relu_in"]:
        W = torch.relu(W)
    return A2, W


def scatter(p, y, mutant=None):
    """[Z, M, N] -> the layout of the output buffer: unchanged, or the pixel shuffle [1, B * H s * W s, Cout] of a ConvTranspose"""
    if p["kind"] != "convT":
        return y
    B, H, W, s, Cout = p["shuf"]
    t = y.reshape(B, H, W, s, s, Cout)                               # n = (i * s + j) * Cout + co
    t = t.permute(0, 1, 4, 2, 3, 5) if mutant == "shuf_swap" else t.permute(0, 1, 3, 2, 4, 5)
    return t.reshape(1, B * H * s * W * s, Cout)


def bias_of(p, dtype, mutant=None):
    """bias broadcast to [Z, 1, N] (a ConvTranspose's bias is per output channel: n % Cout)"""
    b = p["bias"]
    if b is None:
        return None
    if mutant == "bias_batch0":
        b = b[:1].expand_as(b)
    if mutant == "bias_f16":
        b = b.half().float()
    if p["kind"] == "convT":
        s = p["shuf"][3]
        b = b.repeat(1, s * s)
    return b.to(dtype).unsqueeze(1)


# ------------------------------------------------------------------------------------------------ reference + bound
def reference(p, nwave=0, order_free=False):
    """-> (ref, bound), float64 [Z, M, N] (scattered layout for a ConvTranspose).  nwave: 4 | 8 for the split-K skinny kernel, else 0.
    order_free: the fall-back accumulator term (K - 1) 2^-23 S in place of the MFMA model's (for measurements; the tests use the model)."""
    A2, W = as_gemm(p)
    A2, W = A2.double(), W.double()
    K = A2.shape[-1]
    v = A2 @ W.transpose(-1, -2)
    S = A2.abs() @ W.abs().transpose(-1, -2)
    err = (K - 1) * 2 * U * S if order_free else C_MFMA * U * (math.ceil(K / 32) + 1) * S
    if nwave and not order_free:
        err = err + (nwave - 1) * U * S
    b = bias_of(p, torch.float64)
    if b is not None:
        v = v + b
        err = err + U * (v.abs() + err)
    if p["act"] == 1:
        x = v
        v = F.gelu(x)
        err = GELU_LIP * err + 0.5 * x.abs() * K_ERF * U
        err = err + U * (v.abs() + err)
    elif p["act"] == 2:
        v = torch.relu(v)
    for r in (p["res1"], p["res2"]):
        if r is not None:
            v = v + r.double()
            err = err + U * (v.abs() + err)
    if p["out"] == torch.float16:
        err = err + 2.0 ** -11 * (v.abs() + err) + 2.0 ** -25
    return scatter(p, v), scatter(p, err)


# ------------------------------------------------------------------------------------------------ emulation
MUTANTS = {
    "tanh_gelu": "tanh-GELU in place of the erf-GELU",
    "k_tail": "the K tail behind the last whole 64-wide K-tile dropped",
    "bias_f16": "bias rounded to fp16",
    "acc_f16": "accumulator (+ bias, activation) rounded to fp16 before the residual add",
    "no_res2": "res2 ignored",
    "pad_neighbour": "a padding tap left / right of the image read from the neighbouring row instead of zero",
    "stride_origin": "the origin of a stride-2 window off by one",
    "image_border": "a padding tap above / below the image read from the previous / next image's border row",
    "relu_w": "the ReLU on load applied to the weight fragments too",
    "shuf_swap": "(i, j) swapped in the pixel-shuffle scatter",
    "bias_batch0": "bias taken from batch 0",
}


def applies(mutant, p):
    """whether the mutant changes anything in this problem"""
    return {
        "tanh_gelu": p["act"] == 1,
        "k_tail": p["kind"] != "conv" and p["W"].shape[-1] % 64 != 0,
        "bias_f16": p["bias"] is not None,
        "acc_f16": p["res1"] is not None,
        "no_res2": p["res2"] is not None,
        "pad_neighbour": p["kind"] == "conv",
        "stride_origin": p["kind"] == "conv" and p["stride"] == 2,
        "image_border": p["kind"] == "conv" and p["x"].shape[0] > 1,
        "relu_w": bool(p["relu_in"]),
        "shuf_swap": p["kind"] == "convT",
        "bias_batch0": p["bias"] is not None and p["bias"].shape[0] > 1,
    }[mutant]


def emulate(p, nwave=0, mutant=None):
    """The kernels' arithmetic in torch fp32 on the fp16-rounded operands: K in chunks of 32 (one MFMA each) added to the accumulator in
    order (tile 16: the chunks dealt to nwave waves in contiguous runs, the partial sums added in wave order), then the epilogue order of
    gemm_tile_body: bias, activation, res1, res2, store.  -> the output in its own dtype, [Z, M, N] (scattered for a ConvTranspose)."""
    assert mutant is None or mutant in MUTANTS
    A2, W = as_gemm(p, mutant)
    A2, W = A2.float(), W.float()
    K = A2.shape[-1]
    if mutant == "k_tail":
        K -= K % 64
    steps = [(k, min(k + 32, K)) for k in range(0, K, 32)]
    runs = [steps]
    if nwave:
        per = -(-len(steps) // nwave)
        runs = [steps[w * per:(w + 1) * per] for w in range(nwave)]
    acc = None
    for run in runs:
        part = torch.zeros(A2.shape[0], A2.shape[1], W.shape[1], dtype=torch.float32)
        for k0, k1 in run:
            part = part + A2[..., k0:k1] @ W[..., k0:k1].transpose(-1, -2)
        acc = part if acc is None else acc + part
    v = acc
    b = bias_of(p, torch.float32, mutant)
    if b is not None:
        v = v + b
    if p["act"] == 1:
        v = F.gelu(v, approximate="tanh") if mutant == "tanh_gelu" else 0.5 * v * (1.0 + torch.erf(v * 0.70710678118654752440))
    elif p["act"] == 2:
        v = torch.relu(v)
    if mutant == "acc_f16":
        v = v.half().float()
    if p["res1"] is not None:
        v = v + p["res1"].float()
    if p["res2"] is not None and mutant != "no_res2":
        v = v + p["res2"].float()
    return scatter(p, v.to(p["out"]), mutant)


def worst_ratio(got, ref, bound):
    """max over elements of |got - ref| / bound (nan / inf in `got` count as inf) and the flat index where it occurs"""
    r = ((got.double() - ref).abs() / bound).reshape(-1)
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    i = int(r.argmax())
    return float(r[i]), i


def torch_reference(p):
    """the same operation through torch's own operators in fp64 (F.conv2d / matmul / F.conv_transpose2d): what `reference` is checked against"""
    b = p["bias"]
    if p["kind"] == "conv":
        x = p["x"].double().permute(0, 3, 1, 2)
        if p["relu_in"]:
            x = torch.relu(x)
        Cin = x.shape[1]
        w = p["W"][0].double().reshape(-1, 3, 3, Cin).permute(0, 3, 1, 2)
        y = F.conv2d(x, w, None if b is None else b[0].double(), stride=p["stride"], padding=1).permute(0, 2, 3, 1)
        y = y.reshape(1, -1, y.shape[-1])
    elif p["kind"] == "convT":
        B, H, Wd, s, Cout = p["shuf"]
        x = p["A"][0].double().reshape(B, H, Wd, -1).permute(0, 3, 1, 2)
        w = p["W"][0].double().reshape(s, s, Cout, -1).permute(3, 2, 0, 1)              # [Cin, Cout, i, j]
        y = F.conv_transpose2d(x, w, b[0].double(), stride=s).permute(0, 2, 3, 1).reshape(1, -1, Cout)
        return y
    else:
        A = torch.relu(p["A"].double()) if p["relu_in"] else p["A"].double()
        y = torch.matmul(A, p["W"].double().transpose(-1, -2))
        if b is not None:
            y = y + b.double().unsqueeze(1)
    if p["act"] == 1:
        y = F.gelu(y)
    elif p["act"] == 2:
        y = torch.relu(y)
    for r in (p["res1"], p["res2"]):
        if r is not None:
            y = y + r.double()
    return y
