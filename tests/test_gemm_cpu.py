"""CPU: the GEMM case table (tests/gemm_cases.py) reaches every kernel instance the launchers can launch, cut3r_gemm_tile_for keeps its
documented thresholds, and the fp64 oracle (tests/gemm_oracle.py) is right, tight enough to reject the named mutants, and excludes nothing.

`python -m tests.test_gemm_cpu census` prints the codes every case reaches in THIS process (the ring-depth census runs it in a child with
CUT3R_GEMM64_STAGES set: gemm.hip reads that variable once per process).

Ratio table (test_emulation_inside_the_bound_and_mutants_outside prints it): worst |value - fp64| / bound over all elements of all cases
the row applies to, and the case where it occurs.
    emulation       0.995     t128_e1_210tiles      (fp16 outputs: the 2^-11 rounding of the store is a sharp bound; fp32 outputs: 0.29, t256_relu_in)
    tanh_gelu       156       t256_fast_gelu32
    k_tail          8.42e+05  t16_m64_k40_z2
    bias_f16        822       t256_relu_in
    acc_f16         897       t256_relu_in
    no_res2         1.11e+06  t16_m17_k40_res2
    pad_neighbour   7.04e+04  t256_conv64_relu_in_e4
    stride_origin   8.12e+04  t256_conv96_s2
    image_border    7.56e+04  t256_conv64_relu_in_e4
    relu_w          1.25e+06  t256_relu_in
    shuf_swap       8.14e+05  t256_convT
    bias_batch0     1.1e+06   t16_m64_k40_z2
"""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

from cut3r_slam_amd import _lib
from tests import gemm_cases as GC
from tests import gemm_oracle as GO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MUTANT_FACTOR = 10.0            # every mutant must leave the bound by at least an order of magnitude somewhere (measured: the table above)


def _ring_depth():
    e = os.environ.get("CUT3R_GEMM64_STAGES")
    return int(e) if e in ("4", "6") else 3


def census():
    """-> (count, {case name: (code reached, code named)}) in this process"""
    lib = _lib.load()
    depth = _ring_depth()
    return lib.cut3r_gemm_kernel_count(), {c.name: (GC.kernel_for(lib, c, GC.placed(c)), c.code_at(depth)) for c in GC.CASES}


def _check_census(count, reached, what):
    wrong = {n: v for n, v in reached.items() if v[0] != v[1]}
    assert not wrong, f"{what}: cases that do not reach the instance they name (reached, named): {wrong}"
    codes = {v[0] for v in reached.values()}
    assert 0 not in codes
    assert len(codes) == count, f"{what}: the table reaches {len(codes)} instances, the launchers can launch {count}"


def test_census_every_case_reaches_its_instance_and_every_instance_has_a_case():
    count, reached = census()
    _check_census(count, reached, "default environment")
    # every instance has a ragged case: a last row tile or a last column tile that is partly filled
    ragged = set()
    for c in GC.CASES:
        BM, BN = GC.TILE_DIMS[c.tile]
        if any(p["M"] % BM for p in GC.operands(c.name)) or c.N % BN:
            ragged.add(c.code)
    assert ragged == {c.code for c in GC.CASES}, sorted({c.code for c in GC.CASES} - ragged)


@pytest.mark.parametrize("depth", [4, 6])
def test_census_of_the_environment_selected_ring_depths(depth):
    """the 64 x 64 instances that exist only under CUT3R_GEMM64_STAGES = 4 | 6, queried (and counted) in a fresh process"""
    env = dict(os.environ, CUT3R_GEMM64_STAGES=str(depth))
    r = subprocess.run([sys.executable, "-m", "tests.test_gemm_cpu", "census"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    reached = {k: tuple(v) for k, v in got["reached"].items()}
    _check_census(got["count"], reached, f"CUT3R_GEMM64_STAGES={depth}")
    ring = {v[0] for n, v in reached.items() if GC.BY_NAME[n].ring}
    assert ring and all((code // 1000) % 10 == depth for code in ring), ring
    assert got["count"] == _lib.load().cut3r_gemm_kernel_count()          # one instance per ring-depth instance of the default


def test_refused_descriptors_name_no_instance():
    lib = _lib.load()
    for name, base, fields in GC.REFUSED:
        c, ts = GC.refused(name, base, fields)
        assert GC.kernel_for(lib, c, ts) == 0, name
    assert lib.cut3r_gemm_kernel_for(None) == 0 and lib.cut3r_gemm_pair_kernel_for(None, None) == 0


def _tile_for(**kw):
    d = _lib.GemmDesc()
    for k, v in kw.items():
        setattr(d, k, v)
    return _lib.load().cut3r_gemm_tile_for(C.byref(d))


def test_auto_tile_selection_at_its_thresholds():
    T = _tile_for
    # 128 tiles of 256 x 256 (N a multiple of 256) -> 256; one fewer -> 128 x 128 tiles
    assert T(M=256 * 8, N=256 * 16) == 256 and T(M=256 * 8 - 256, N=256 * 16) == 128
    assert T(M=256 * 127, N=256) == 128 and T(M=256 * 128, N=256) == 256
    assert T(M=256 * 8, N=256 * 16 + 128) == 128                              # N not a multiple of 256
    assert T(M=256 * 4, N=256 * 16, batch=2) == 256 and T(M=256 * 4, N=256 * 16) == 128      # the batch multiplies the grid
    # beyond one round of 256 workgroups the last round must be 85 % full: 2 * 256 * 0.85 = 435.2 tiles
    assert T(M=256 * 109, N=1024) == 256 and T(M=256 * 87, N=1280) == 128       # 436 and 435 tiles
    assert T(M=256 * 64, N=1024) == 256 and T(M=256 * 75, N=1024) == 128        # 256 tiles (one full round), 300 tiles
    # 128 tiles of 128 x 128 -> 128, fewer -> 64
    assert T(M=128 * 16, N=128 * 8 - 124) == 128 and T(M=128 * 16 - 128, N=128 * 8 - 124) == 64
    assert T(M=127 * 128 + 1, N=128) == 128 and T(M=127 * 128, N=128) == 64
    # 3x3 convolutions: 512 tiles of 192 x 128 -> 192128 (256 first where it fills), fewer -> by fill; a pixel shuffle never
    assert T(M=192 * 512, N=128, conv_k=3) == 192128 and T(M=192 * 512 - 192, N=128, conv_k=3) == 128
    assert T(M=192 * 256, N=256, conv_k=3) == 256 and T(M=192 * 512, N=128) == 128
    assert T(M=192 * 512, N=128, conv_k=3, shuf=2) == 128 and T(M=256 * 128, N=256, shuf=2) == 128
    # 48-wide RoPE heads: the 128 x 192 tile, whatever the size; 64-wide heads by fill; an explicit tile is kept
    assert T(M=70, N=240, rope_pos=4096, rope_cols=240, rope_d=48) == 128192 and T(M=256 * 128, N=768, rope_pos=4096, rope_cols=768, rope_d=48) == 128192
    assert T(M=256 * 64, N=1024, rope_pos=4096, rope_cols=1024, rope_d=64) == 256 and T(M=70, N=240, rope_pos=4096, rope_cols=192, rope_d=64) == 64
    assert T(M=70, N=240, tile=12864) == 12864 and _lib.load().cut3r_gemm_tile_for(None) == 0


@pytest.fixture(scope="module")
def oracle():
    """(reference, bound) of every problem of every case, computed once"""
    return {c.name: [GO.reference(p, c.nwave) for p in GC.operands(c.name)] for c in GC.PINNED}


def test_reference_equals_torch_fp64_operators(oracle):
    for c in GC.PINNED:
        for p, (ref, bound) in zip(GC.operands(c.name), oracle[c.name]):
            t = GO.torch_reference(p)
            assert t.shape == ref.shape, c.name
            err = float((t - ref).abs().max())
            assert err <= 1e-12 * max(1.0, float(ref.abs().max())), f"{c.name}: {err:.3e}"
            assert bool((bound > 0).all()) and bool(torch.isfinite(bound).all())


EXCLUDED_CAP = 0                # there is no ambiguity mask: no case may take any element out of the comparison


def test_no_element_is_excluded_from_the_comparison(oracle):
    """every element of every output has a finite, positive bound (so `|got - ref| <= bound` is decided everywhere), and the bound is a
    rounding-sized quantity: below 2^-9 of |ref| + S-scale for fp16 outputs, 2^-12 for fp32 ones (K <= 2304)"""
    for c in GC.PINNED:
        for p, (ref, bound) in zip(GC.operands(c.name), oracle[c.name]):
            excluded = int((~torch.isfinite(bound) | ~(bound > 0) | ~torch.isfinite(ref)).sum())
            assert excluded <= EXCLUDED_CAP, f"{c.name}: {excluded} elements without a usable bound"
            assert bound.numel() == ref.numel() == p["M"] * c.N * c.Z
            scale = ref.abs() + 8.0                                   # S <= ~ 0.64 sqrt(K) < 32; bias and residuals of order 1
            assert float((bound / scale).max()) <= (2.0 ** -9 if p["out"] == GC.F16 else 2.0 ** -12), c.name


def test_emulation_inside_the_bound_and_mutants_outside(oracle):
    rows = {m: (0.0, "-") for m in (None, *GO.MUTANTS)}
    for c in GC.PINNED:
        for p, (ref, bound) in zip(GC.operands(c.name), oracle[c.name]):
            if c.name == "t128_e1_210tiles":                                  # (3.2 M elements: the emulation only)
                muts = (None,)
            else:
                muts = (None, *[m for m in GO.MUTANTS if GO.applies(m, p)])
            for m in muts:
                r, _ = GO.worst_ratio(GO.emulate(p, c.nwave, m), ref, bound)
                if m is None:
                    assert r <= 1.0, f"{c.name}: the emulation leaves the bound, worst ratio {r:.3f}"
                if r > rows[m][0]:
                    rows[m] = (r, c.name)
    for m, (r, name) in rows.items():
        print(f"    {m or 'emulation':15s} {r:<9.3g} {name}")
    for m in GO.MUTANTS:
        assert rows[m][0] >= MUTANT_FACTOR, f"mutant {m} ({GO.MUTANTS[m]}) stays within {rows[m][0]:.2f} x the bound on every case"


def test_tanh_gelu_mutant_is_rejected_in_every_gelu_case(oracle):
    """the tanh form must fail in EVERY case with a GELU (so that swapping erff for it in one epilogue fails exactly that epilogue's cases)"""
    for c in GC.PINNED:
        if c.act != 1:
            continue
        for p, (ref, bound) in zip(GC.operands(c.name), oracle[c.name]):
            r, _ = GO.worst_ratio(GO.emulate(p, c.nwave, "tanh_gelu"), ref, bound)
            assert r > 2.0, f"{c.name}: tanh-GELU stays within {r:.2f} x the bound"


if __name__ == "__main__":
    if sys.argv[1:] == ["census"]:
        n, reached = census()
        print(json.dumps({"count": n, "reached": reached}))
