"""CPU: the standard 3DGS PLY of cut3r_slam_amd/gs_ply.py -- the layout of hislam2/gaussian/scene/gaussian_model.py:433-470 as read off its
source (parity with a file the reference wrote is UNPINNED): literal header, bit-exact round trips, reading by property name, refusals,
and the channel-major order of f_rest."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cut3r_slam_amd import gs_ply  # noqa: E402

HEADER_K1 = ("ply\nformat binary_little_endian 1.0\nelement vertex 2\n"
             "property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n"
             "property float f_dc_0\nproperty float f_dc_1\nproperty float f_dc_2\nproperty float opacity\n"
             "property float scale_0\nproperty float scale_1\nproperty float scale_2\n"
             "property float rot_0\nproperty float rot_1\nproperty float rot_2\nproperty float rot_3\nend_header\n")


def _cloud(P, K, seed=0):
    """raw parameters with the awkward values: negative zero, subnormals, 1e30"""
    g = np.random.default_rng(seed)
    d = {"xyz": g.standard_normal((P, 3)), "f_dc": g.standard_normal((P, 3)), "f_rest": g.standard_normal((P, K - 1, 3)),
         "opacity": g.standard_normal((P, 1)), "scaling": g.standard_normal((P, 3)), "rotation": g.standard_normal((P, 4))}
    d = {k: v.astype(np.float32) for k, v in d.items()}
    special = np.array([-0.0, 1e-45, -3e-39, 1e30, -1e30], np.float32)
    for v in d.values():
        flat = v.reshape(-1)
        n = min(len(special), flat.size)
        flat[:n] = special[:n]
    return d


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _write(path, d):
    gs_ply.write_gaussian_ply(path, d["xyz"], d["f_dc"], d["f_rest"], d["opacity"], d["scaling"], d["rotation"])


def test_header_is_the_literal_text_and_the_body_has_17_floats_a_vertex(tmp_path):
    path = str(tmp_path / "a.ply")
    _write(path, _cloud(2, 1))
    data = open(path, "rb").read()
    assert data[:len(HEADER_K1)] == HEADER_K1.encode("ascii")
    assert len(data) - len(HEADER_K1) == 2 * 17 * 4
    assert gs_ply.attribute_names(4)[9:18] == [f"f_rest_{i}" for i in range(9)] and len(gs_ply.attribute_names(16)) == 17 + 45


@pytest.mark.parametrize("K", [1, 4, 16])
@pytest.mark.parametrize("P", [0, 1, 5, 1000])
def test_round_trip_is_bit_exact(tmp_path, P, K):
    path = str(tmp_path / "a.ply")
    d = _cloud(P, K, seed=P + K)
    _write(path, d)
    r = gs_ply.read_gaussian_ply(path)
    assert r["K"] == K
    for k, v in d.items():
        assert r[k].shape == v.shape and r[k].dtype == np.float32, k
        assert np.array_equal(_bits(r[k]), _bits(v)), k
    width = 17 + 3 * (K - 1)
    body = np.frombuffer(open(path, "rb").read()[-P * width * 4:] if P else b"", "<f4").reshape(P, width)
    assert not body[:, 3:6].any()                                         # the normals are zeros


def _handmade(path, names, types, rows, fmt="binary_little_endian", count=None, extra_element=False):
    """a PLY written here byte by byte, independently of gs_ply: names / types per property, rows of python numbers"""
    code = {"float": "f", "double": "d", "uchar": "B", "int": "i"}
    head = f"ply\nformat {fmt} 1.0\ncomment written by the test\nelement vertex {len(rows) if count is None else count}\n"
    head += "".join(f"property {t} {n}\n" for n, t in zip(names, types))
    if extra_element:
        head += "element face 0\nproperty list uchar int vertex_indices\n"
    head += "end_header\n"
    with open(path, "wb") as fh:
        fh.write(head.encode("ascii"))
        for row in rows:
            for v, t in zip(row, types):
                fh.write(struct.pack("<" + code[t], v))


def test_shuffled_order_an_extra_property_and_no_normals_read_equal(tmp_path):
    K, P = 4, 7
    d = _cloud(P, K, seed=3)
    ours = [n for n in gs_ply.attribute_names(K) if n not in ("nx", "ny", "nz")]
    cols = {"x": d["xyz"][:, 0], "y": d["xyz"][:, 1], "z": d["xyz"][:, 2], "opacity": d["opacity"][:, 0]}
    for i in range(3):
        cols[f"f_dc_{i}"], cols[f"scale_{i}"] = d["f_dc"][:, i], d["scaling"][:, i]
    for i in range(4):
        cols[f"rot_{i}"] = d["rotation"][:, i]
    for c in range(3):
        for j in range(K - 1):
            cols[f"f_rest_{c * (K - 1) + j}"] = d["f_rest"][:, j, c]
    order = list(np.random.default_rng(1).permutation(len(ours)))
    names = [ours[i] for i in order]
    names.insert(5, "label")                                              # an unknown property of another type in the middle
    types = ["uchar" if n == "label" else "float" for n in names]
    rows = [[(200 if n == "label" else float(cols[n][p])) for n in names] for p in range(P)]
    path = str(tmp_path / "b.ply")
    _handmade(path, names, types, rows, extra_element=True)
    r = gs_ply.read_gaussian_ply(path)
    assert r["K"] == K
    for k, v in d.items():
        assert np.array_equal(_bits(r[k]), _bits(v)), k


def test_refusals(tmp_path):
    names = [n for n in gs_ply.attribute_names(1)]
    row = [[0.5] * len(names)]
    p = lambda s: str(tmp_path / s)
    _handmade(p("ok.ply"), names, ["float"] * len(names), row)
    assert gs_ply.read_gaussian_ply(p("ok.ply"))["xyz"].shape == (1, 3)
    open(p("ascii.ply"), "w").write("ply\nformat ascii 1.0\nelement vertex 0\n" + "".join(f"property float {n}\n" for n in names) + "end_header\n")
    _handmade(p("big.ply"), names, ["float"] * len(names), row, fmt="binary_big_endian")
    _handmade(p("missing.ply"), [n for n in names if n != "rot_3"], ["float"] * (len(names) - 1), [[0.5] * (len(names) - 1)])
    _handmade(p("double.ply"), names, ["double" if n == "opacity" else "float" for n in names], row)
    _handmade(p("rest.ply"), names + ["f_rest_0", "f_rest_1"], ["float"] * (len(names) + 2), [[0.5] * (len(names) + 2)])
    k3 = names + [f"f_rest_{i}" for i in range(6)]                       # 3 (K - 1) = 6: K = 3 is no SH degree
    _handmade(p("k3.ply"), k3, ["float"] * len(k3), [[0.5] * len(k3)])
    _handmade(p("short.ply"), names, ["float"] * len(names), row, count=2)
    open(p("nothing.ply"), "wb").write(b"not a ply at all")
    for bad in ("ascii", "big", "missing", "double", "rest", "k3", "short", "nothing"):
        with pytest.raises(ValueError):
            gs_ply.read_gaussian_ply(p(bad + ".ply"))
    d = _cloud(3, 1)
    with pytest.raises(ValueError):                                       # K - 1 = 2 is refused on the way out as well
        gs_ply.write_gaussian_ply(p("w.ply"), d["xyz"], d["f_dc"], np.zeros((3, 2, 3), np.float32), d["opacity"], d["scaling"], d["rotation"])


@pytest.mark.parametrize("K", [4, 9, 16])
def test_f_rest_is_channel_major(tmp_path, K):
    names = gs_ply.attribute_names(K)
    value = {f"f_rest_{c * (K - 1) + j}": 100.0 * c + j for c in range(3) for j in range(K - 1)}
    rows = [[value.get(n, 0.0 if n in ("nx", "ny", "nz") else 0.25) for n in names] for _ in range(3)]
    path = str(tmp_path / "c.ply")
    _handmade(path, names, ["float"] * len(names), rows)
    r = gs_ply.read_gaussian_ply(path)
    for c in range(3):
        for j in range(K - 1):
            assert (r["f_rest"][:, j, c] == 100.0 * c + j).all()
    # the same through the frozen container: features[:, j + 1, c], DC first; and out again through the writer
    import torch
    cloud = gs_ply.GaussianCloud.from_ply(path, "cpu")
    assert cloud.sh_degree == {4: 1, 9: 2, 16: 3}[K] and tuple(cloud.features.shape) == (3, K, 3)
    for c in range(3):
        for j in range(K - 1):
            assert bool((cloud.features[:, j + 1, c] == 100.0 * c + j).all())
    assert bool((cloud.features[:, 0] == 0.25).all())
    assert torch.equal(cloud.get_opacity, torch.sigmoid(torch.full((3, 1), 0.25))) and torch.equal(cloud.get_scaling, torch.exp(torch.full((3, 3), 0.25)))
    with pytest.raises(AttributeError):
        cloud.xyz = None
    cloud.save_ply(str(tmp_path / "d.ply"))
    assert open(str(tmp_path / "d.ply"), "rb").read() == open(path, "rb").read().replace(b"comment written by the test\n", b"")
