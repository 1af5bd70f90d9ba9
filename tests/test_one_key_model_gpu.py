"""GPU: the decoder with the one-key attention work left out, the view tail in one launch, the head inputs read in place and q / k RoPE of
the 48-wide cross attention in one launch (CUT3R_ONE_KEY=1, the default) against the launches it replaces (CUT3R_ONE_KEY=0).

Every replaced step is exact -- a softmax over one key is 1, a skinny-kernel output column does not depend on the other columns, the
LayerNorm row body is shared, a GEMM row is the same bits in every tile kernel, RoPE is per element -- so every prediction, every state
tap and every memory tap must be torch.equal.  One fresh child process per setting (tests/one_key_child.py): the model reads its
switches from the environment when it is built.
"""
import os
import subprocess
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 240


def _children(tmp_path, extra):
    """both settings of the switch side by side, each in its own process"""
    procs = []
    for one_key in ("1", "0"):
        env = dict(os.environ)
        env.update(extra)
        env["CUT3R_ONE_KEY"] = one_key
        path = str(tmp_path / f"one_key_{one_key}.pt")
        procs.append((one_key, path, subprocess.Popen([sys.executable, "-m", "tests.one_key_child", path], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                                                      stderr=subprocess.STDOUT, text=True)))
    res = {}
    for one_key, path, p in procs:
        try:
            out, _ = p.communicate(timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            for _, _, q in procs:
                q.kill()
            out, _ = p.communicate()
            pytest.fail(f"the CUT3R_ONE_KEY={one_key} child was killed at its time limit of {CHILD_TIMEOUT} s; its output:\n{(out or '')[-4000:]}")
        assert p.returncode == 0, f"the CUT3R_ONE_KEY={one_key} child exited {p.returncode}; its output:\n{out[-4000:]}"
        res[one_key] = torch.load(path)
    return res["1"], res["0"]


@pytest.mark.parametrize("extra", [{}, {"CUT3R_GRAPHS": "0"}, {"CUT3R_PAIR_ROWS": "1000000000"}], ids=["default", "no-graphs", "pair-rows"])
def test_one_key_on_and_off_give_the_same_bits(tmp_path, extra):
    t0 = time.time()
    on, off = _children(tmp_path, extra)
    print(f"[one key model] {extra or 'default'}: {len(on)} tensors per child, {time.time() - t0:.1f} s")
    assert set(on) == set(off)
    # (both configurations, minimal and full; predictions of the window and of the batched windows, state and memory taps)
    for part in ("tiny.minimal", "tiny.full", "wide.minimal", "wide.full"):
        for kind in (".window.view2.camera_pose", ".window.state2", ".window.mem2", ".windows.pts3d_in_self_view"):
            assert part + kind in on, part + kind
    assert "wide.full.window.view0.pts3d_in_other_view" in on and "tiny.full.windows.rgb" in on
    bad = [k for k in sorted(on) if not torch.equal(on[k], off[k])]
    for k in bad:
        print(f"[one key model] {k}: differs at {int((on[k] != off[k]).sum())} / {on[k].numel()}, max |diff| {float((on[k].double() - off[k].double()).abs().max()):.3e}")
    assert not bad, bad
