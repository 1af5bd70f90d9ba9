"""CPU: the LPIPS oracle (tests/lpips_oracle.py) and the weight loader of cut3r_slam_amd/lpips.py.  No kernel runs here."""
import ctypes
import ctypes.util
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cut3r_slam_amd import lpips as LP  # noqa: E402
from tests import lpips_oracle as LO  # noqa: E402
from tests import lpips_ref as LR  # noqa: E402


def _libm_fmaf(a, b, c):
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    return np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)


def test_fma32_is_libm_fmaf():
    """random triples over many exponents; near-ties (the exact result half an fp32 ulp from two neighbours, nudged by the addend's last
    bits); cancellations (c = -round(a b), so the result is the product's rounding error)"""
    g = np.random.default_rng(0)
    n = 20000
    a = (g.standard_normal(n) * 2.0 ** g.integers(-20, 20, n)).astype(np.float32)
    b = (g.standard_normal(n) * 2.0 ** g.integers(-20, 20, n)).astype(np.float32)
    c = (g.standard_normal(n) * 2.0 ** g.integers(-20, 20, n)).astype(np.float32)
    # near-ties: a b = an odd multiple of 2^-24 next to 1 (a = 1 + 2^-12 ... products with 25+ significant bits), c tiny of either sign
    ta = (1 + g.integers(1, 2 ** 12, n) * 2.0 ** -12).astype(np.float32)
    tb = (1 + (2 * g.integers(0, 2 ** 11, n) + 1) * 2.0 ** -13).astype(np.float32)
    tc = (g.choice([-1.0, 1.0], n) * 2.0 ** g.integers(-60, -24, n)).astype(np.float32)
    # cancellations
    ca = g.standard_normal(n).astype(np.float32)
    cb = g.standard_normal(n).astype(np.float32)
    cc = -(ca * cb)
    A, B, C = np.concatenate([a, ta, ca]), np.concatenate([b, tb, cb]), np.concatenate([c, tc, cc])
    got, want = LO.fma32(A, B, C), _libm_fmaf(A, B, C)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (np.concatenate([ca * cb + cc]) == 0).all() and (got[2 * n:] != 0).any()        # the cancelling triples do exercise the residual
    assert (got[n:2 * n] != (ta * tb + tc)).any()                                           # and the ties a double rounding gets wrong


def test_oracle_agrees_with_an_independent_fp64_formulation():
    """the contract's fp32 chain and torch's own fp32 convolutions are two fp32 orders of one sum: the oracle's error against fp64 may be at
    most 4 x that of torch in fp32 (4 covers the luck of the order).  Measured: e_chain 7.32e-08, e_torch32 4.61e-08."""
    sd = LR.weights()
    e_chain, e_t32 = 0.0, 0.0
    for H, W in LR.SIZES:
        a, b = LR.pair(H, W)
        for norm in LP.NORMS:
            ref = LR.torch_score(sd, a, b, norm, torch.float64)
            s = LR.oracle(H, W, norm)[3]
            t32 = LR.torch_score(sd, a, b, norm, torch.float32)
            assert ref > 1e-3
            e_chain, e_t32 = max(e_chain, abs(s - ref) / ref), max(e_t32, abs(t32 - ref) / ref)
            print(f"[lpips] {H}x{W} {norm}: fp64 {ref:.9f}, oracle rel err {abs(s - ref) / ref:.2e}, torch fp32 rel err {abs(t32 - ref) / ref:.2e}")
    print(f"[lpips] e_chain {e_chain:.3e}, e_torch32 {e_t32:.3e}")
    assert e_chain <= 4 * e_t32


def test_oracle_tap_sizes_and_identical_images():
    fa, _, vs, _ = LR.oracle(31, 31)
    assert [v.shape for v in vs] == [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]
    assert [f.shape[-1] for f in fa] == [64, 192, 384, 256, 256]
    sd = {k: v.numpy() for k, v in LR.weights().items()}
    a, _ = LR.pair(31, 31)
    for norm in LP.NORMS:
        _, _, vs, score = LO.lpips(sd, a, a.copy(), norm)
        assert score == 0.0 and all((v == 0).all() for v in vs)


def test_synthetic_weights_are_seeded_and_shaped():
    a, b, c = LP.synth_lpips_state_dict(3), LP.synth_lpips_state_dict(3), LP.synth_lpips_state_dict(4)
    assert list(a) == list(LP.schema()) and all(tuple(a[k].shape) == s and a[k].dtype == torch.float32 for k, s in LP.schema().items())
    assert all(torch.equal(a[k], b[k]) for k in a) and not torch.equal(a["features.0.weight"], c["features.0.weight"])
    assert float(a["lin2.model.1.weight"].min()) >= 0 and float(a["lin2.model.1.weight"].max()) < 1 / 384
    assert abs(float(a["features.6.weight"].std()) - (2 / (192 * 9)) ** 0.5) < 1e-3


def _spellings(sd):
    tv = {k: v for k, v in sd.items() if k.startswith("features.")}
    tv["classifier.1.weight"] = torch.zeros(4, 4)
    tv["classifier.1.bias"] = torch.zeros(4)
    lin_a = {k: v for k, v in sd.items() if k.startswith("lin")}
    lin_b = {f"lins.{l}.model.1.weight": sd[f"lin{l}.model.1.weight"] for l in range(5)}
    sl = {f"net.slice{s}.{i}.{p}": sd[f"features.{i}.{p}"] for i, s in ((0, 1), (3, 2), (6, 3), (8, 4), (10, 5)) for p in ("weight", "bias")}
    return tv, lin_a, lin_b, sl


def test_loader_accepts_every_spelling_and_merges_files(tmp_path):
    from safetensors.torch import save_file
    sd = LR.weights()
    tv, lin_a, lin_b, sl = _spellings(sd)
    torch.save(tv, tmp_path / "alexnet.pth")
    torch.save(lin_a, tmp_path / "alex.pth")
    save_file({"module." + k: v.contiguous() for k, v in lin_b.items()}, str(tmp_path / "lins.safetensors"))
    save_file({k: v.contiguous() for k, v in {**sl, **lin_a}.items()}, str(tmp_path / "all.safetensors"))
    torch.save({"state_dict": {"module.net." + k: v for k, v in {**tv, **lin_b}.items()}}, tmp_path / "wrapped.pth")
    for files in (("alexnet.pth", "alex.pth"), ("alexnet.pth", "lins.safetensors"), ("all.safetensors",), ("wrapped.pth",)):
        got = LP.load_lpips_weights(*[tmp_path / f for f in files])
        assert list(got) == list(sd) and all(torch.equal(got[k], sd[k]) for k in sd), files
    with pytest.raises(ValueError, match=r"lin0\.model\.1\.weight is missing"):
        LP.load_lpips_weights(tmp_path / "alexnet.pth")
    bad = dict(lin_a)
    bad["lin3.model.1.weight"] = torch.zeros(1, 384, 1, 1)
    torch.save(bad, tmp_path / "bad.pth")
    with pytest.raises(ValueError, match=r"lin3\.model\.1\.weight has shape \(1, 384, 1, 1\)"):
        LP.load_lpips_weights(tmp_path / "alexnet.pth", tmp_path / "bad.pth")
    with pytest.raises(FileNotFoundError):
        LP.load_lpips_weights(tmp_path / "nowhere.pth")


def test_loader_reads_pth_files_weights_only(tmp_path):
    """a pickle that would run code on loading is refused, not executed"""
    import pickle

    class Boom:
        def __reduce__(self):
            return (os.mkdir, (str(tmp_path / "ran"),))
    with open(tmp_path / "evil.pth", "wb") as f:
        pickle.dump({"features.0.weight": Boom()}, f)
    with pytest.raises(Exception):
        LP.load_lpips_weights(tmp_path / "evil.pth")
    assert not (tmp_path / "ran").exists()


def test_lpips_refuses_cpu_tensors_bad_shapes_and_bad_weights():
    L = LP.LPIPS(LR.weights())
    a = torch.rand(3, 40, 40)
    with pytest.raises(ValueError, match="GPU"):
        L(a, a)
    with pytest.raises(ValueError, match="GPU"):
        L.maps(a[None], a[None])
    sd = dict(LR.weights())
    sd["lin1.model.1.weight"] = torch.zeros(1, 64, 1, 1)
    with pytest.raises(ValueError, match=r"lin1\.model\.1\.weight has shape"):
        LP.LPIPS(sd)
    with pytest.raises(ValueError, match="norm"):
        LP.LPIPS(LR.weights(), norm="vgg")
    with pytest.raises(ValueError):
        LP.LPIPS(LR.weights(), device="cpu")
