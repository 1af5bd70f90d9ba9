"""One row of tests/gemm_cases.py on the GPU (tests/test_gemm_gpu.py), written so that the rows whose instance depends on
CUT3R_GEMM64_STAGES also run in a FRESH process: `python -m tests.gemm_instances_child` -- gemm.hip reads that variable once per process.
Not collected by pytest.  The child runs every `ring` row under its environment, prints one JSON line {"code:output type": [worst err / bound, case]}
and exits 0; on the first row that fails it prints the failure and exits 1.

run_case makes, per row: the instance code (cut3r_gemm_kernel_for / cut3r_gemm_pair_kernel_for), one launch through the C ABI into a
NaN-filled payload inside a sentinel-filled buffer (guard rows above and below, guard columns, a guard batch), |got - ref| <= bound on EVERY
element (fp64 reference and derived bound: tests/gemm_oracle.py), untouched guards, and the same bits from a second launch."""
import ctypes as C
import functools
import json
import os
import sys

import torch

from cut3r_slam_amd import _lib, ops
from tests import gemm_cases as GC
from tests import gemm_oracle as GO

DEV = "cuda:0"


def ring_depth():
    e = os.environ.get("CUT3R_GEMM64_STAGES")
    return int(e) if e in ("4", "6") else 3


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(reference, bound) of the row's problems: computed once per process, shared, never modified"""
    c = GC.BY_NAME[name]
    return [GO.reference(p, c.nwave) for p in GC.operands(name)]


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def launch(c, ts):
    lib = _lib.load()
    if c.pair:
        return lib.cut3r_gemm_f16_pair(C.byref(ts[0]["desc"]), C.byref(ts[1]["desc"]), ops._stream())
    return lib.cut3r_gemm_f16(C.byref(ts[0]["desc"]), ops._stream())


def guards_untouched(name, t):
    """every element of the buffer outside the payload still holds the sentinel's bits"""
    c = t["buf"].clone()
    v = t["out"]
    torch.as_strided(c, v.size(), v.stride(), v.storage_offset()).fill_(GC.SENT)
    bad = bits(c) != bits(torch.full((1,), GC.SENT, dtype=c.dtype, device=c.device))
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} guard elements overwritten, first at {bad.nonzero()[:4].tolist()} of a {tuple(c.shape)} buffer"


def run_case(name):
    """-> (code, worst err / bound over every element of every problem of the row)"""
    c = GC.BY_NAME[name]
    lib = _lib.load()
    ts = GC.placed(c, DEV)
    code = GC.kernel_for(lib, c, ts)
    assert code == c.code_at(ring_depth()), f"{name}: reaches instance {code}, the table names {c.code_at(ring_depth())}"
    assert launch(c, ts) == 0, f"{name}: the launch was refused"
    torch.cuda.synchronize()
    first, worst = [], 0.0
    for i, (t, (ref, bound)) in enumerate(zip(ts, oracle(name))):
        got = t["out"].cpu()
        first.append(got)
        guards_untouched(name, t)
        ratio, at = GO.worst_ratio(got.reshape(ref.shape), ref, bound)
        worst = max(worst, ratio)
        print(f"[gemm instance {code}] {name} problem {i}: worst err / bound {ratio:.3f}")
        if not ratio <= 1.0:
            n_out = int(((got.reshape(ref.shape).double() - ref).abs() > bound).sum())
            raise AssertionError(f"{name} problem {i} (instance {code}): err / bound = {ratio:.3f} at flat element {at}: got "
                                 f"{float(got.reshape(-1)[at]):.8g}, fp64 {float(ref.reshape(-1)[at]):.8g}, bound {float(bound.reshape(-1)[at]):.3g}; "
                                 f"{n_out} of {ref.numel()} elements outside their bound")
    for t in ts:
        t["out"].fill_(float("nan"))
    assert launch(c, ts) == 0
    torch.cuda.synchronize()
    for i, (t, g0) in enumerate(zip(ts, first)):
        assert torch.equal(bits(t["out"].cpu()), bits(g0)), f"{name} problem {i}: a second launch gives other bits"
        guards_untouched(name, t)
    return code, worst


def main():
    worst = {}
    for c in GC.PINNED:
        if not c.ring:
            continue
        try:
            code, r = run_case(c.name)
        except AssertionError as e:
            print(f"FAILED under CUT3R_GEMM64_STAGES={os.environ.get('CUT3R_GEMM64_STAGES')}: {e}", flush=True)
            return 1
        key = f"{code}:{c.out}"
        if r >= worst.get(key, [0.0, ""])[0]:
            worst[key] = [r, c.name]
    print(json.dumps(worst), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
