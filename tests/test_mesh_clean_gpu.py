"""GPU: csrc/mesh_clean.hip (vertex clustering, small-component removal) against the numpy oracle: every array bit for bit, every count
equal."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cut3r_slam_amd import mesh_clean as MC  # noqa: E402
from cut3r_slam_amd import ops  # noqa: E402
from cut3r_slam_amd.tsdf import Mesh  # noqa: E402
from tests import mesh_clean_oracle as MO  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COUNTS = ("clusters", "degenerate", "duplicate", "unreferenced")


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what):
    if want is None:
        assert got is None, what
        return
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} against {want.shape} {want.dtype}"
    assert np.array_equal(_bits(got), _bits(want)), f"{what}: {np.count_nonzero(_bits(got) != _bits(want))} entries differ"


def _check_cluster(v, c, f, cell, got=None):
    """GPU against the oracle; returns the oracle's info"""
    want = MO.simplify_vertex_clustering(v, c, f, cell)
    mesh, info = MC.simplify_vertex_clustering(Mesh(v, c, f), cell) if got is None else got
    _same(mesh.vertices, want[0], "vertices")
    _same(mesh.colors, want[1], "colors")
    _same(mesh.faces, want[2], "faces")
    _same(info["vertex_map"], want[3]["vertex_map"], "vertex_map")
    _same(info["face_map"], want[3]["face_map"], "face_map")
    for k in COUNTS:
        assert info[k] == want[3][k], f"{k}: {info[k]} against {want[3][k]}"
    return want[3]


def _check_components(v, c, f, got=None, **opt):
    want = MO.remove_small_components(v, c, f, **opt)
    mesh, info = MC.remove_small_components(Mesh(v, c, f), **opt) if got is None else got
    _same(mesh.vertices, want[0], "vertices")
    _same(mesh.colors, want[1], "colors")
    _same(mesh.faces, want[2], "faces")
    for k in ("labels", "components", "vertex_map", "face_map"):
        _same(info[k], want[3][k], k)
    assert info["n_components"] == want[3]["n_components"] and info["rounds"] == want[3]["rounds"]
    return want[3]


def _soup(V=3000, F=6000, seed=0):
    g = np.random.default_rng(seed)
    return g.random((V, 3)).astype(np.float32), g.integers(0, 256, (V, 3), dtype=np.uint8), g.integers(0, V, (F, 3)).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- vertex clustering
@pytest.mark.parametrize("cell", [0.04, 0.1, 0.25])
def test_clustering_of_the_sphere_matches_the_oracle(cell):
    v, c, f = MO.sphere_mesh()
    info = _check_cluster(v, c, f, cell)
    print(f"cell {cell}: {len(v)} -> {info['clusters']} clusters, " + ", ".join(f"{k} {info[k]}" for k in COUNTS[1:]))
    assert all(info[k] > 0 for k in COUNTS)                  # all three rules fire on a real extraction


@pytest.mark.parametrize("cell", [0.25, 0.5])
def test_clustering_of_a_random_soup_matches_the_oracle(cell):
    v, c, f = _soup()
    info = _check_cluster(v, c, f, cell)
    assert info["degenerate"] > 0 and info["duplicate"] > 0
    _check_cluster(v, None, f, cell)                         # no colours


@pytest.mark.parametrize("V", [1, 255, 256, 257, 511, 513])
def test_clustering_at_block_edges(V):
    for F in (1, 255, 256, 257, 511, 513):
        v, c, f = _soup(V, F, seed=V * 1000 + F)
        _check_cluster(v, c, f, 0.2)


def test_clustering_on_cell_boundaries():
    # multiples of 0.125 with cell 0.25: (p - lo) / cell is exact and half of the vertices sit on a cell face
    g = np.random.default_rng(1)
    v = (g.integers(-16, 17, (2000, 3)) * 0.125).astype(np.float32)
    f = g.integers(0, 2000, (4000, 3)).astype(np.int32)
    q =(v.astype(np.float64) - (v.min(0).astype(np.float64) - 0.125)) / 0.25
    assert np.array_equal(q * 2, np.round(q * 2)) and 0.3 < np.mean(q == np.floor(q)) < 0.7
    _check_cluster(v, None, f, 0.25)


def test_orientation_is_kept_and_the_first_duplicate_wins():
    v = np.asarray([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    a, b, c = 0, 1, 2
    f = np.asarray([[a, b, c], [b, c, a], [a, c, b], [a, b, c]], np.int32)
    mesh, info = MC.simplify_vertex_clustering(Mesh(v, None, f), 0.5)
    assert info["face_map"].tolist() == [0, 2] and info["duplicate"] == 2 and info["degenerate"] == 0
    _check_cluster(v, None, f, 0.5, got=(mesh, info))
    assert mesh.faces.tolist() == [[0, 2, 1], [0, 1, 2]] or mesh.faces.tolist() == [[0, 1, 2], [0, 2, 1]]


def test_total_collapse_gives_an_empty_mesh():
    v, c, f = _soup(300, 500)
    mesh, info = MC.simplify_vertex_clustering(Mesh(v, c, f), 10.0)
    assert mesh.vertices.shape == (0, 3) and mesh.colors.shape == (0, 3) and mesh.faces.shape == (0, 3)
    assert info["clusters"] == 1 and info["degenerate"] == 500 and info["unreferenced"] == 1 and np.all(info["vertex_map"] == -1)
    _check_cluster(v, c, f, 10.0, got=(mesh, info))
    out, _ = MC.clean(Mesh(v, c, f), cell=10.0, min_faces=3)     # nothing left to filter: returned as it is
    assert len(out.faces) == 0


@pytest.mark.parametrize("cell", [0.1, 0.25])
def test_clusters_are_the_voxels_of_the_downsample(cell):
    v, c, f = MO.sphere_mesh()
    mesh, info = MC.simplify_vertex_clustering(Mesh(v, c, f), cell)
    dv, dc, _ = ops.voxel_downsample(torch.from_numpy(v).to(DEV), cell, torch.from_numpy(c).to(DEV))
    dv, dc = dv.cpu().numpy(), dc.cpu().numpy()
    cid, M = MO.cluster_ids(v, cell)
    assert len(dv) == M == info["clusters"]
    vm = info["vertex_map"]
    src = np.flatnonzero(vm >= 0)
    # every kept output vertex is the row of its cluster in the downsample of the same vertices, and the dropped clusters are the rest
    assert np.array_equal(mesh.vertices[vm[src]].view(np.uint32), dv[cid[src]].view(np.uint32))
    assert np.array_equal(mesh.colors[vm[src]], dc[cid[src]])
    assert len(np.unique(cid[src])) == len(mesh.vertices) == M - info["unreferenced"]


def test_one_and_two_sort_passes_give_the_same_bits():
    v, c, f = _soup()
    g = lambda a, dt: torch.from_numpy(a).to(DEV, dt)
    one = ops.mesh_cluster(g(v, torch.float32), g(c, torch.uint8), g(f, torch.int32), 0.25, passes=1)
    two = ops.mesh_cluster(g(v, torch.float32), g(c, torch.uint8), g(f, torch.int32), 0.25, passes=2)
    assert one["duplicate"] > 0
    for k in ("vertices", "colors", "faces", "vertex_map", "face_map"):
        assert torch.equal(one[k], two[k]), k
    _check_cluster(v, c, f, 0.25, got=(Mesh(two["vertices"], two["colors"], two["faces"]), two))
    sv, sc, sf = MO.sphere_mesh()
    two = ops.mesh_cluster(g(sv, torch.float32), g(sc, torch.uint8), g(sf, torch.int32), 0.04, passes=2)
    _check_cluster(sv, sc, sf, 0.04, got=(Mesh(two["vertices"], two["colors"], two["faces"]), two))


# ------------------------------------------------------------------------------------------------------------ connected components
def test_component_thresholds_on_the_sphere():
    v, c, f = MO.sphere_mesh()
    L, _ = MO.component_labels(f, len(v))
    size = np.bincount(L[f[:, 0]])
    sizes = sorted(size[size > 0].tolist())
    assert sizes == [22] + [24] * 16 + [48, 26280]
    kept = {}
    for n in (22, 23, 24, 25, 48, 49, 26280, 26281):
        info = _check_components(v, c, f, min_faces=n)
        kept[n] = len(info["components"])
        assert sorted(info["components"][:, 1].tolist()) == [s for s in sizes if s >= n]
    assert kept == {22: 19, 23: 18, 24: 18, 25: 2, 48: 2, 49: 1, 26280: 1, 26281: 0}
    mesh, info = MC.remove_small_components(Mesh(v, c, f), min_faces=26281)
    assert mesh.vertices.shape == (0, 3) and mesh.faces.shape == (0, 3) and len(info["face_map"]) == 0 and np.all(info["vertex_map"] == -1)
    for k in (1, 2, 3):
        info = _check_components(v, c, f, keep_largest=k)
        assert info["components"][:, 1].tolist() == [26280, 48, 24][:k]
    assert info["components"][2, 0] == min(l for l in np.flatnonzero(size) if size[l] == 24)      # the 24-face component of smallest label


def test_components_of_a_random_soup():
    v, c, f = _soup()
    f = f[:700]
    info = _check_components(v, c, f, min_faces=2)
    assert info["n_components"] > 50 and info["components"][0, 1] > 300
    _check_components(v, None, f, keep_largest=5)
    assert (info["vertex_map"] == -1).sum() > 1000           # vertices in no face are dropped


@pytest.mark.parametrize("V", [1, 255, 256, 257, 511, 513])
def test_components_at_block_edges(V):
    for F in (1, 255, 256, 257, 511, 513):
        v, c, f = _soup(V, F, seed=V * 1000 + F)
        _check_components(v, c, f, min_faces=2)


def test_descending_chain_converges_within_the_cap():
    n = 4096
    V = n + 2
    a = np.arange(n)
    f = np.stack([V - 1 - a, V - 2 - a, V - 3 - a], 1).astype(np.int32)          # the smallest index sits at the far end of the strip
    v = np.random.default_rng(3).random((V, 3)).astype(np.float32)
    want, want_rounds = MO.component_labels(f, V)
    assert np.all(want == 0)
    labels, rounds = ops.mesh_labels(torch.from_numpy(f).to(DEV), V)
    print(f"descending strip of {n} triangles: {rounds} labelling rounds (oracle {want_rounds}), cap {V}")
    assert np.array_equal(labels.cpu().numpy(), want.astype(np.int32)) and 1 <= rounds <= V
    _check_components(v, None, f, keep_largest=1)
    # a strip in random vertex order: chains that do not descend along the strip
    p = np.random.default_rng(4).permutation(V).astype(np.int32)
    labels, rounds = ops.mesh_labels(torch.from_numpy(p[f]).to(DEV), V)
    print(f"the same strip with shuffled vertex indices: {rounds} labelling rounds")
    assert np.array_equal(labels.cpu().numpy(), MO.component_labels(p[f], V)[0].astype(np.int32)) and rounds <= V


# -------------------------------------------------------------------------------------------------------- determinism, kinds, refusals
def test_two_runs_give_the_same_bits_and_tensors_give_tensors():
    v, c, f = MO.sphere_mesh()
    tv, tc, tf = torch.from_numpy(v).to(DEV), torch.from_numpy(c).to(DEV), torch.from_numpy(f).to(DEV)
    for run, args, kw in ((MC.simplify_vertex_clustering, (0.1,), {}), (MC.remove_small_components, (), {"min_faces": 25}),
                          (MC.clean, (), {"cell": 0.1, "keep_largest": 1})):
        a_mesh, a_info = run(Mesh(v, c, f), *args, **kw)
        b_mesh, b_info = run(Mesh(v, c, f), *args, **kw)
        t_mesh, t_info = run(Mesh(tv, tc, tf), *args, **kw)
        assert all(isinstance(x, np.ndarray) for x in a_mesh) and all(isinstance(x, torch.Tensor) and x.is_cuda for x in t_mesh)
        for x, y, z in zip(a_mesh, b_mesh, t_mesh):
            assert np.array_equal(_bits(x), _bits(y)) and np.array_equal(_bits(x), _bits(z.cpu().numpy()))
        if run is MC.clean:
            a_info, b_info, t_info = a_info["components"], b_info["components"], t_info["components"]
        for k, x in a_info.items():
            if isinstance(x, np.ndarray):
                assert np.array_equal(x, b_info[k]) and isinstance(t_info[k], torch.Tensor) and np.array_equal(x, t_info[k].cpu().numpy()), k
            else:
                assert x == b_info[k] == t_info[k], k
    want = MO.clean(v, c, f, cell=0.1, keep_largest=1)
    for x, y in zip(a_mesh, want):
        assert np.array_equal(_bits(x), _bits(y))


def test_refusals_raise_and_a_valid_call_still_works():
    v, c, f = _soup(300, 500)
    M = lambda vv=v, cc=c, ff=f: Mesh(vv, cc, ff)
    bad_hi, bad_lo = f.copy(), f.copy()
    bad_hi[499, 2] = 300
    bad_lo[0, 0] = -1
    nan_v, inf_v = v.copy(), v.copy()
    nan_v[7, 1] = np.nan
    inf_v[299, 0] = np.inf
    wide = v.copy()
    wide[0, 0] = 3.0e6                                       # 3e6 / 1 > 2^21 cells
    empty_v, empty_f = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    refused = [lambda: MC.simplify_vertex_clustering(M(ff=bad_hi), 0.2), lambda: MC.simplify_vertex_clustering(M(ff=bad_lo), 0.2),
               lambda: MC.remove_small_components(M(ff=bad_hi), min_faces=2), lambda: MC.remove_small_components(M(ff=bad_lo), min_faces=2),
               lambda: MC.simplify_vertex_clustering(M(vv=nan_v), 0.2), lambda: MC.simplify_vertex_clustering(M(vv=inf_v), 0.2),
               lambda: MC.remove_small_components(M(vv=nan_v), min_faces=2),
               lambda: MC.simplify_vertex_clustering(M(), 0.0), lambda: MC.simplify_vertex_clustering(M(), -1.0),
               lambda: MC.simplify_vertex_clustering(M(), float("nan")), lambda: MC.simplify_vertex_clustering(M(), float("inf")),
               lambda: MC.simplify_vertex_clustering(M(vv=wide), 1.0),
               lambda: MC.simplify_vertex_clustering(Mesh(empty_v, None, f), 0.2), lambda: MC.simplify_vertex_clustering(Mesh(v, c, empty_f), 0.2),
               lambda: MC.remove_small_components(Mesh(v, c, empty_f), min_faces=1),
               lambda: MC.remove_small_components(M(), min_faces=0), lambda: MC.remove_small_components(M(), keep_largest=0),
               lambda: MC.remove_small_components(M(), min_faces=-3),
               lambda: MC.remove_small_components(M(), min_faces=2, keep_largest=1), lambda: MC.remove_small_components(M()),
               lambda: MC.clean(M(), cell=0.2, min_faces=2, keep_largest=1), lambda: MC.clean(M())]
    tv, tc, tf = torch.from_numpy(v).to(DEV), torch.from_numpy(c).to(DEV), torch.from_numpy(f).to(DEV)
    refused += [lambda: ops.mesh_cluster(tv, tc, tf, 0.2, capacity=(1, 10 ** 6)), lambda: ops.mesh_cluster(tv, tc, tf, 0.2, capacity=(10 ** 6, 1)),
                lambda: ops.mesh_components(tv, tc, tf, min_faces=1, capacity=(1, 10 ** 6)),
                lambda: ops.mesh_cluster(tv, tc[:10], tf, 0.2), lambda: ops.mesh_cluster(tv.double(), tc, tf, 0.2),
                lambda: ops.mesh_cluster(tv, tc, tf.long(), 0.2), lambda: ops.mesh_cluster(tv.cpu(), tc, tf, 0.2)]
    for k, call in enumerate(refused):
        with pytest.raises(ValueError):
            call()
        if k % 8 == 0:                                       # a valid call after a refused one
            _check_cluster(v, c, f, 0.2)
    _check_cluster(v, c, f, 0.2)
    _check_components(v, c, f, min_faces=2)
    big = ops.mesh_cluster(tv, tc, tf, 0.2, capacity=(1000, 1000))       # more room than needed is fine
    _check_cluster(v, c, f, 0.2, got=(Mesh(big["vertices"], big["colors"], big["faces"]), big))


def test_the_c_entry_points_refuse_with_a_status():
    import ctypes as C
    from cut3r_slam_amd import _lib
    lib = _lib.load()
    v, c, f = _soup(300, 500)
    tv, tf = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    n = lib.cut3r_mesh_cluster_workspace_bytes(300, 500)
    assert n > 0 and lib.cut3r_mesh_cluster_workspace_bytes(0, 500) == -1 and lib.cut3r_mesh_components_workspace_bytes(300, 0) == -1
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    tot = torch.zeros(4, dtype=torch.int64, device=DEV)
    lo, hi = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    assert lib.cut3r_mesh_cluster_count(p(tv), 300, 500, 0.0, lo, hi, p(ws), n, p(tot), None) == 1          # cell
    assert lib.cut3r_mesh_cluster_count(p(tv), 300, 500, 0.2, hi, lo, p(ws), n, p(tot), None) == 1          # reversed bounds
    assert lib.cut3r_mesh_cluster_count(p(tv), 300, 500, 1e-7, lo, hi, p(ws), n, p(tot), None) == 1         # 2^21 cells or more
    assert lib.cut3r_mesh_cluster_count(p(tv), 300, 500, 0.2, lo, hi, p(ws), n - 1, p(tot), None) == 1      # workspace
    assert lib.cut3r_mesh_cluster_faces(p(tf), 300, 500, 301, 0, p(ws), n, p(tot), None, None) == 1         # M > V
    assert lib.cut3r_mesh_cluster_faces(p(tf), 300, 500, 10, 3, p(ws), n, p(tot), None, None) == 1          # passes
    assert lib.cut3r_mesh_faces_check(p(tf), 0, 300, p(tot), None) == 1
    assert lib.cut3r_mesh_components_count(p(tf), 300, 500, p(tf), 2, 1, p(ws), n, p(tot), None) == 1       # both options
    assert lib.cut3r_mesh_components_count(p(tf), 300, 500, p(tf), 0, 0, p(ws), n, p(tot), None) == 1       # neither
    assert lib.cut3r_mesh_label_round(p(tf), 300, 500, None, None, None, None) == 1
    torch.cuda.synchronize()
    _check_cluster(v, c, f, 0.2)
