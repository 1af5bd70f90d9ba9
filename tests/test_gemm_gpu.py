"""GPU: every kernel instance of csrc/gemm.hip that cut3r_gemm_f16 / cut3r_gemm_f16_pair can launch, named (cut3r_gemm_kernel_for) and
pinned per element to an fp64 reference with a derived fp32 error bound (tests/gemm_oracle.py), at the rows of tests/gemm_cases.py;
tests/test_gemm_cpu.py shows on the host that those rows reach ALL instances.  Per row: tests/gemm_instances_child.py (run_case).

The RoPE-epilogue and LayerNorm-fold instances of the 256 x 256 tile get no bound of their own: they must give the bits of the unfused
sequence, whose GEMM is pinned above -- projection then the stand-alone rope_2d kernel; the fold with slab statistics that make the
row's rstd exactly 1 and its mean exactly 0 (sum 0, m2 32 per slab, eps 0.5) is the plain projection; with real statistics the rows
equal those of the 128 x 128 tile's folded kernel.

The two ring depths that only CUT3R_GEMM64_STAGES selects run in one child process each; the last test prints the worst err / bound
per instance (the table in DESIGN.md)."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from cut3r_slam_amd import _lib, ops  # noqa: E402
from tests import gemm_cases as GC  # noqa: E402
from tests import gemm_instances_child as GI  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = GI.DEV
F16, F32 = torch.float16, torch.float32
# a child: interpreter start, import of torch, opening the GPU (2 - 3 s measured for tests/gemm_forms_child.py) + 16 small rows; the limit
# leaves room for a cold page cache
CHILD_TIMEOUT = 60
WORST = {}                      # (instance code, output type) -> (worst err / bound, case), filled by the tests of this file as they run


def _record(code, out, ratio, name):
    if ratio >= WORST.get((code, out), (0.0, ""))[0]:
        WORST[(code, out)] = (ratio, name)


@pytest.mark.parametrize("code", sorted({c.code for c in GC.PINNED}))
def test_instance_is_named_and_every_element_is_inside_its_bound(code):
    """every row of the table that names this instance (one test per instance, not per row: the per-test clean-up of the GPU fixtures
    costs more than a row does); a failure names its row"""
    for c in GC.PINNED:
        if c.code == code:
            reached, ratio = GI.run_case(c.name)
            assert reached == c.code_at(GI.ring_depth())
            _record(reached, c.out, ratio, c.name)


def test_refused_descriptors_launch_nothing():
    for name, base, fields in GC.REFUSED:
        c, ts = GC.refused(name, base, fields, DEV)
        assert GC.kernel_for(_lib.load(), c, ts) == 0, name
        assert GI.launch(c, ts) == 1, name
        torch.cuda.synchronize()
        for t in ts:
            assert bool(torch.isnan(t["out"]).all()), f"{name}: a refused launch wrote to its output"
            GI.guards_untouched(name, t)


# ------------------------------------------------------------------------------------------------ RoPE epilogue, LayerNorm fold
def _special(name, seed):
    """the row placed on the GPU with its table of angles and random positions (beyond the 48 table rows the kernel keeps in LDS too)"""
    c = GC.BY_NAME[name]
    ts = GC.placed(c, DEV)
    t = ts[0]
    assert GC.kernel_for(_lib.load(), c, ts) == c.code, f"{name}: reaches {GC.kernel_for(_lib.load(), c, ts)}, the table names {c.code}"
    g = torch.Generator().manual_seed(seed)
    if c.rope:
        t["table"].copy_(ops.rope_table(DEV, 100.0, 1.0, c.rope[1]))
        t["pos"].copy_(torch.randint(-1, 60, tuple(t["pos"].shape), generator=g, dtype=torch.int64))
    if c.ln:                        # rstd = 1 / sqrt(32 nslab / K + 0.5) = 1 and mu = 0, exactly; any column sums (multiplied by rstd mu = 0)
        t["stats"][..., 0] = 0.0
        t["stats"][..., 1] = 32.0
        t["colsum"].copy_(torch.randn(c.N, generator=g))
    return c, ts, t


def _run(c, ts, name):
    t = ts[0]
    assert GI.launch(c, ts) == 0, name
    torch.cuda.synchronize()
    GI.guards_untouched(name, t)
    got = t["out"][0].clone()
    assert bool(torch.isfinite(got).all()), f"{name}: elements never written"
    t["out"].fill_(float("nan"))
    assert GI.launch(c, ts) == 0
    torch.cuda.synchronize()
    assert torch.equal(GI.bits(t["out"][0]), GI.bits(got)), f"{name}: a second launch gives other bits"
    return got


def _plain(c, t, tile=256):
    """the unfused projection of the row: the same operands, fp16 output, no RoPE, no fold -> the pinned instance it runs on, its output"""
    M = t["desc"].M
    ref = torch.empty(M, c.N, dtype=F16, device=DEV)
    d = ops._linear_desc(t["A"][0], t["W"][0], ref, t["bias"][0], c.act, None, tile)
    code = _lib.load().cut3r_gemm_kernel_for(C.byref(d))
    ops.linear(t["A"][0], t["W"][0], ref, t["bias"][0], c.act, tile=tile)
    return code, ref


def _rope_after(c, t, ref):
    cols, hd = c.rope
    ops.rope_2d(ref.view(1, ref.shape[0], c.N // hd, hd)[:, :, :cols // hd], t["pos"].view(1, -1, 2), 100.0, 1.0)
    torch.cuda.synchronize()
    return ref


def test_rope_epilogue_instance_gives_the_bits_of_projection_then_rope_kernel():
    c, ts, t = _special("t256_rope", 1)
    got = _run(c, ts, c.name)
    code, ref = _plain(c, t)
    assert code == 300110                       # the unfused projection runs on an instance pinned per element above
    before = ref.clone()
    ref = _rope_after(c, t, ref)
    assert torch.equal(got, ref), f"{int((got != ref).sum())} elements differ from projection + rope_2d"
    assert not torch.equal(ref[:, :c.rope[0]], before[:, :c.rope[0]]) and torch.equal(ref[:, c.rope[0]:], before[:, c.rope[0]:])


@pytest.mark.parametrize("name,plain_code", [("t256_ln_e1", 300110), ("t256_ln_e2", 300120), ("t256_ln_rope", 300110)])
def test_fold_instances_with_unit_statistics_give_the_bits_of_the_plain_projection(name, plain_code):
    c, ts, t = _special(name, 2)
    got = _run(c, ts, name)
    code, ref = _plain(c, t)
    assert code == plain_code
    if c.rope:
        ref = _rope_after(c, t, ref)
    torch.cuda.synchronize()
    assert torch.equal(got, ref), f"{name}: {int((got != ref).sum())} elements differ from the unfused sequence"


@pytest.mark.parametrize("name", ["t256_ln_e1", "t256_ln_e2", "t256_ln_rope"])
def test_fold_instances_with_real_statistics_give_the_rows_of_the_128_tile(name):
    """the statistics path (slab combination, rstd, the mean's correction): residual-stream-like rows through the fold's producer, then
    the consumer at tile 256 (the instance under test) and at tile 128 (its run-time / compile-time epilogues in gemm_tile_body)"""
    c = GC.BY_NAME[name]
    M, N, K = c.M, c.N, c.K
    g = torch.Generator().manual_seed(3)
    x = torch.randn(M, K, generator=g) + 0.5 * torch.randn(M, 1, generator=g)
    x[::3, 7] += 300.0
    out, x16 = torch.empty(M, K, dtype=F32, device=DEV), torch.empty(M, K, dtype=F16, device=DEV)
    st = torch.full((K // 64, M, 2), float("nan"), dtype=F32, device=DEV)
    ops.linear(torch.zeros(M, 64, dtype=F16, device=DEV), torch.zeros(K, 64, dtype=F16, device=DEV), out, torch.zeros(K, device=DEV),
               res1=x.to(DEV), tile=64, emit=(st, x16))
    Wf = (torch.randn(N, K, generator=g) / K ** 0.5).half().to(DEV)
    d, cs = torch.randn(N, generator=g).to(DEV), Wf.double().sum(1).float()
    rope = None
    if c.rope:
        rope = (torch.randint(-1, 60, (M, 2), generator=g, dtype=torch.int64).to(DEV), c.rope[0], 100.0, c.rope[1])
    res = {}
    for tile in (256, 128):
        o = torch.full((M, N), float("nan"), dtype=F16, device=DEV)
        desc = ops._linear_desc(x16, Wf, o, d, c.act, None, tile, rope, (st, cs, 1e-6))
        code = _lib.load().cut3r_gemm_kernel_for(C.byref(desc))
        assert code == (c.code if tile == 256 else (122310 if rope else 122311 + c.act)), (tile, code)
        ops.linear(x16, Wf, o, d, c.act, tile=tile, rope=rope, ln=(st, cs, 1e-6))
        torch.cuda.synchronize()
        res[tile] = o
    assert bool(torch.isfinite(res[256]).all())
    assert torch.equal(res[256], res[128]), f"{name}: {int((res[256] != res[128]).sum())} elements differ between the 256 and the 128 tile"
    xd = x16.double().cpu()                                    # and the value: LayerNorm (no affine part) + projection in fp64
    ln = (xd - x.double().mean(1, keepdim=True)) / torch.sqrt(x.double().var(1, unbiased=False, keepdim=True) + 1e-6)
    y = ln @ Wf.double().cpu().T + d.double().cpu()
    if c.act == 1:
        y = torch.nn.functional.gelu(y)
    if not c.rope:
        err = float((res[256].double().cpu() - y).abs().max() / y.abs().max())
        assert err < 3e-3, err                                 # (the bound of tests/test_lnfold_gpu.py; the pin is the bit equality above)


# ------------------------------------------------------------------------------------------------ environment-selected ring depths
def test_ring_depths_selected_by_the_environment_in_fresh_processes():
    """CUT3R_GEMM64_STAGES = 4, then 6: every `ring` row in a new process (the variable is read once per process), one child at a time,
    each under its own time limit; the first child that does not exit 0 ends the test and nothing further is started"""
    for depth in (4, 6):
        env = dict(os.environ, CUT3R_GEMM64_STAGES=str(depth))
        t0 = time.time()
        try:
            r = subprocess.run([sys.executable, "-m", "tests.gemm_instances_child"], cwd=ROOT, env=env, timeout=CHILD_TIMEOUT,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        except subprocess.TimeoutExpired as e:
            out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
            pytest.fail(f"ring depth {depth}: the child was killed at its time limit of {CHILD_TIMEOUT} s; its output:\n{out[-4000:]}")
        if r.returncode < 0:
            pytest.fail(f"ring depth {depth}: the child was killed by signal {-r.returncode}; its output:\n{r.stdout[-4000:]}")
        assert r.returncode == 0, f"ring depth {depth}: the child exited {r.returncode}; its output:\n{r.stdout[-4000:]}"
        worst = json.loads(r.stdout.strip().splitlines()[-1])
        assert worst and all((int(key.split(":")[0]) // 1000) % 10 == depth for key in worst), worst
        for key, (ratio, name) in worst.items():
            _record(int(key.split(":")[0]), key.split(":")[1], ratio, name)
        print(f"[gemm instances] CUT3R_GEMM64_STAGES={depth}: {len(worst)} instances ({time.time() - t0:.1f} s)")


def test_print_the_worst_ratio_per_instance():
    """(last in the file) the worst err / bound of every instance the tests above pinned per element, over its rows with an fp16 output
    (where the fp16 rounding of the store, a sharp bound, is nearly all of it) and over its rows with an fp32 output"""
    for code in sorted({k[0] for k in WORST}):
        cols = [f"{WORST[(code, o)][0]:.3f} {WORST[(code, o)][1]:28s}" if (code, o) in WORST else f"{'-':34s}" for o in ("f16", "f32")]
        print(f"    {code}  fp16 out {cols[0]}  fp32 out {cols[1]}")
    pinned = {c.code for c in GC.PINNED}
    if pinned <= {k[0] for k in WORST}:                        # (the whole file ran: every pinned instance has its figure, and it holds)
        assert max(v[0] for v in WORST.values()) <= 1.0
