"""GPU, end to end: demo.py --mesh with the clean-up flags (a cleaned PLY next to unchanged outputs) and the command line of
cut3r_slam_amd.mesh_clean as a fresh process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cut3r_slam_amd import mesh_clean as MC  # noqa: E402
from cut3r_slam_amd import tsdf as T  # noqa: E402
from tests import mesh_clean_oracle as MO  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _same_mesh(a, b):
    assert a.vertices.shape == b.vertices.shape and a.faces.shape == b.faces.shape
    assert np.array_equal(a.vertices.view(np.uint32), b.vertices.view(np.uint32)) and np.array_equal(a.colors, b.colors)
    assert np.array_equal(a.faces, b.faces)


def test_demo_writes_a_cleaned_mesh_and_leaves_its_other_outputs_unchanged(tmp_path, monkeypatch):
    import demo
    from cut3r_slam_amd import stream
    from tests.test_stream_gpu import _write_sequence
    d = tmp_path / "colors"
    d.mkdir()
    _write_sequence(str(d), 36)
    calib = tmp_path / "calib.txt"
    calib.write_text("600.0 600.0 320.0 240.0")
    base = ["--imagedir", str(d), "--calib", str(calib), "--kf_every", "2", "--synthetic-weights", "--small", "--seed", "1"]
    seen = []
    real = stream.save_trajectory

    def spy(slam, *a, **k):
        seen.append(slam)
        return real(slam, *a, **k)

    monkeypatch.setattr(stream, "save_trajectory", spy)
    assert demo.main(base + ["--output", str(tmp_path / "plain")]) == 0
    # the random network's depth scale sets the voxel: 64 voxels over the largest extent of the fused points
    kf = seen[0].keyframes
    n = kf.counter.value - 1
    dep = kf.depth[:n]
    depth_max = float(dep[(dep > 0) & torch.isfinite(dep)].max())
    lo, hi = T.depth_bounds(dep, kf.w2c[:n], kf.intrinsic[:n].to(DEV), depth_max)
    voxel = float(np.max(hi - lo)) / 64
    mesh_args = ["--mesh", "--voxel-size", repr(voxel), "--depth-max", repr(depth_max)]
    raw, out = tmp_path / "raw", tmp_path / "clean"
    assert demo.main(base + ["--output", str(raw)] + mesh_args) == 0
    cell, min_faces = 2.5 * voxel, 8
    assert demo.main(base + ["--output", str(out)] + mesh_args + ["--mesh-simplify", repr(cell), "--mesh-min-faces", str(min_faces)]) == 0
    for name in ("traj_kf.txt", "tsdf_mesh_w1.0.ply"):
        assert (out / name).read_bytes() == (raw / name).read_bytes(), name
    assert sorted(os.listdir(out)) == sorted(os.listdir(raw) + ["tsdf_mesh_w1.0_clean.ply"])
    mesh = T.read_ply(out / "tsdf_mesh_w1.0.ply")
    cleaned = T.read_ply(out / "tsdf_mesh_w1.0_clean.ply")
    print(f"demo mesh: {len(mesh.vertices)} vertices, {len(mesh.faces)} faces -> cleaned {len(cleaned.vertices)}, {len(cleaned.faces)}")
    assert len(mesh.faces) >= 1 and len(cleaned.faces) <= len(mesh.faces) and len(cleaned.vertices) < len(mesh.vertices)
    if len(cleaned.faces):
        assert np.array_equal(np.unique(cleaned.faces), np.arange(len(cleaned.vertices)))      # only referenced vertices
    else:
        assert len(cleaned.vertices) == 0
    _same_mesh(cleaned, MC.clean(mesh, cell=cell, min_faces=min_faces)[0])
    want = MO.clean(mesh.vertices, mesh.colors, mesh.faces, cell=cell, min_faces=min_faces)
    _same_mesh(cleaned, T.Mesh(*want))


def test_command_line_round_trip(tmp_path):
    v, c, f = MO.sphere_mesh()
    src, dst = tmp_path / "in.ply", tmp_path / "out.ply"
    T.write_ply(src, T.Mesh(v, c, f))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "cut3r_slam_amd.mesh_clean", str(src), str(dst), "--cell", "0.1", "--keep-largest", "1"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    _same_mesh(T.read_ply(dst), T.Mesh(*MO.clean(v, c, f, cell=0.1, keep_largest=1)))
    # both filters at once are refused by the parser, and nothing is written
    for bad in (["--min-faces", "3", "--keep-largest", "1"], []):
        with pytest.raises(SystemExit):
            MC.main([str(src), str(tmp_path / "no.ply")] + bad)
    assert not (tmp_path / "no.ply").exists()
