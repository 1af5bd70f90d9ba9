"""CPU: the numpy oracle of the mesh clean-up (tests/mesh_clean_oracle.py) against a dictionary-and-loop restatement on hand-made meshes,
against scipy's connected components, and its properties on the extracted sphere."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import mesh_clean_oracle as MO  # noqa: E402


# ------------------------------------------------------------------------------------------------ brute force: dictionaries and loops
def _brute_cluster(v, c, f, cell):
    v = np.asarray(v, np.float32)
    lo = [float(v[:, a].min()) - cell / 2 for a in range(3)]
    cells = {}
    for i, p in enumerate(v):
        key = tuple(int(math.floor((float(p[a]) - lo[a]) / cell)) for a in range(3))
        cells.setdefault(key, []).append(i)
    order = sorted(cells)
    cid = {i: m for m, key in enumerate(order) for i in cells[key]}
    pos, col = [], []
    for key in order:
        s, sc = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
        for i in cells[key]:
            for a in range(3):
                s[a] += float(v[i, a])
                if c is not None:
                    sc[a] += float(c[i, a])
        n = len(cells[key])
        pos.append([np.float32(s[a] / n) for a in range(3)])
        col.append([int(math.floor(sc[a] / n + 0.5)) for a in range(3)])
    seen, faces, face_map, deg, dup = set(), [], [], 0, 0
    for k, (a, b, cc) in enumerate(np.asarray(f).tolist()):
        t = (cid[a], cid[b], cid[cc])
        if len(set(t)) < 3:
            deg += 1
            continue
        while t[0] != min(t):
            t = (t[1], t[2], t[0])
        if t in seen:
            dup += 1
            continue
        seen.add(t)
        faces.append(t)
        face_map.append(k)
    used = sorted({m for t in faces for m in t})
    new = {m: n for n, m in enumerate(used)}
    return (np.asarray([pos[m] for m in used], np.float32).reshape(-1, 3), np.asarray([col[m] for m in used], np.uint8).reshape(-1, 3),
            np.asarray([[new[m] for m in t] for t in faces], np.int32).reshape(-1, 3),
            {"vertex_map": np.asarray([new.get(cid[i], -1) for i in range(len(v))], np.int32), "face_map": np.asarray(face_map, np.int32),
             "clusters": len(order), "degenerate": deg, "duplicate": dup, "unreferenced": len(order) - len(used)})


def _brute_labels(f, V):
    lab = list(range(V))
    again = True
    while again:                                             # the smallest index floods every component
        again = False
        for t in np.asarray(f).tolist():
            m = min(lab[i] for i in t)
            for i in t:
                if lab[i] != m:
                    lab[i], again = m, True
    return np.asarray(lab)


def _brute_components(v, f, min_faces=None, keep_largest=None):
    lab = _brute_labels(f, len(v))
    size = {}
    for t in np.asarray(f).tolist():
        size[lab[t[0]]] = size.get(lab[t[0]], 0) + 1
    order = sorted(size, key=lambda l: (-size[l], l))
    kept = [l for l in order if size[l] >= min_faces] if min_faces is not None else order[:keep_largest]
    face_map = [k for k, t in enumerate(np.asarray(f).tolist()) if lab[t[0]] in kept]
    used = sorted({i for k in face_map for i in np.asarray(f)[k].tolist()})
    new = {i: n for n, i in enumerate(used)}
    return (np.asarray(v, np.float32)[used].reshape(-1, 3), np.asarray([[new[i] for i in np.asarray(f)[k].tolist()] for k in face_map], np.int32).reshape(-1, 3),
            {"labels": lab, "components": [(l, size[l]) for l in kept], "face_map": face_map,
             "vertex_map": [new.get(i, -1) for i in range(len(v))]})


def _hand_meshes():
    g = np.random.default_rng(5)
    out = []
    for V, F in ((3, 1), (5, 4), (8, 12), (12, 20), (12, 6)):
        v = (g.integers(-4, 5, (V, 3)) * 0.3 + g.uniform(-0.05, 0.05, (V, 3))).astype(np.float32)
        out.append((v, g.integers(0, 256, (V, 3), dtype=np.uint8), g.integers(0, V, (F, 3)).astype(np.int32)))
    # two triangles sharing an edge, a far triangle, an isolated vertex, a face given three times in its rotations and once flipped
    v = np.asarray([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [5, 5, 5], [6, 5, 5], [5, 6, 5], [9, 9, 9]], np.float32)
    f = np.asarray([[0, 1, 2], [1, 3, 2], [4, 5, 6], [1, 2, 0], [2, 0, 1], [0, 2, 1]], np.int32)
    out.append((v, np.arange(24, dtype=np.uint8).reshape(8, 3), f))
    return out


@pytest.mark.parametrize("cell", [0.2, 0.7, 1.5, 20.0])
def test_clustering_oracle_equals_the_brute_force(cell):
    for v, c, f in _hand_meshes():
        want = _brute_cluster(v, c, f, cell)
        got = MO.simplify_vertex_clustering(v, c, f, cell)
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])
        assert np.array_equal(got[2], want[2])
        for k in want[3]:
            assert np.array_equal(got[3][k], want[3][k]), k


def test_components_oracle_equals_the_brute_force():
    for v, c, f in _hand_meshes():
        L, rounds = MO.component_labels(f, len(v))
        assert np.array_equal(L, _brute_labels(f, len(v))) and 1 <= rounds <= len(v)
        for opt in ({"min_faces": 1}, {"min_faces": 2}, {"min_faces": 100}, {"keep_largest": 1}, {"keep_largest": 2}, {"keep_largest": 50}):
            bv, bf, bi = _brute_components(v, f, **opt)
            ov, oc, of, oi = MO.remove_small_components(v, c, f, **opt)
            assert np.array_equal(ov, bv) and np.array_equal(of, bf) and np.array_equal(oc, c[np.asarray(bi["vertex_map"]) >= 0])
            assert [tuple(r) for r in oi["components"].tolist()] == bi["components"]
            assert oi["face_map"].tolist() == bi["face_map"] and oi["vertex_map"].tolist() == bi["vertex_map"]


def test_labels_agree_with_scipy():
    sp = pytest.importorskip("scipy.sparse")
    cg = pytest.importorskip("scipy.sparse.csgraph")
    g = np.random.default_rng(0)
    v, _, f = MO.sphere_mesh()
    for faces, V in ((f, len(v)), (g.integers(0, 3000, (700, 3)), 3000), (g.integers(0, 50, (20, 3)), 50)):
        faces = np.asarray(faces, np.int64)
        e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
        n, part = cg.connected_components(sp.coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(V, V)), directed=False)
        L, _ = MO.component_labels(faces, V)
        assert len(np.unique(L)) == n
        # the same partition: one label per scipy part and one part per label; and the label is the part's smallest index
        assert len(np.unique(np.stack([L, part], 1), axis=0)) == n
        first = np.full(n, V)
        np.minimum.at(first, part, np.arange(V))
        assert np.array_equal(L, first[part])


@pytest.mark.parametrize("cell", [0.04, 0.1, 0.25])
def test_clustering_properties_on_the_sphere(cell):
    v, c, f = MO.sphere_mesh()
    ov, oc, of, info = MO.simplify_vertex_clustering(v, c, f, cell)
    assert len(of) > 0 and of.min() >= 0 and of.max() < len(ov)
    # every output vertex inside the closed box of its cell
    # every output vertex inside the closed box of its cell: between the smallest and the largest coordinate of the cluster's own
    # vertices, which lie in the cell by the definition of the index (the mean of fp32 values, rounded to fp32, cannot leave their range)
    idx, _ = MO.CO.voxel_keys(v, cell)
    vm, fm = info["vertex_map"], info["face_map"]
    src = np.flatnonzero(vm >= 0)
    assert all(len(np.unique(idx[src][vm[src] == n], axis=0)) == 1 for n in range(0, len(ov), 7))       # one cell per output vertex
    cmin, cmax = np.full((len(ov), 3), np.inf, np.float32), np.full((len(ov), 3), -np.inf, np.float32)
    np.minimum.at(cmin, vm[src], v[src])
    np.maximum.at(cmax, vm[src], v[src])
    assert np.all(ov >= cmin) and np.all(ov <= cmax)
    # no degenerate face, no repeated rotated triple, every vertex referenced
    assert np.all((of[:, 0] != of[:, 1]) & (of[:, 1] != of[:, 2]) & (of[:, 0] != of[:, 2]))
    assert np.all(of[:, 0] < of[:, 1]) and np.all(of[:, 0] < of[:, 2])
    assert len(np.unique(of, axis=0)) == len(of)
    assert np.array_equal(np.unique(of), np.arange(len(ov)))
    # the maps: survivors in input order, each the image of its input face; vertices of one cluster share an output vertex
    assert np.all(np.diff(fm) > 0) and np.array_equal(MO.rotate_smallest_first(vm[f[fm]]), of)
    assert info["clusters"] - info["unreferenced"] == len(ov) and len(f) - info["degenerate"] - info["duplicate"] == len(of)
    assert np.array_equal(np.unique(vm[vm >= 0]), np.arange(len(ov))) and (vm == -1).sum() > 0
    assert np.array_equal(ov.view(np.uint32), info["cluster_vertices"][np.unique(info["cluster_of_vertex"][src])].view(np.uint32))


def test_component_removal_properties_on_the_sphere():
    v, c, f = MO.sphere_mesh()
    ov, oc, of, info = MO.remove_small_components(v, c, f, min_faces=25)
    assert [r[1] for r in info["components"].tolist()] == [26280, 48] and info["n_components"] == 19
    vm, fm = info["vertex_map"], info["face_map"]
    assert np.array_equal(vm[f[fm]], of) and np.array_equal(np.unique(of), np.arange(len(ov)))
    assert np.array_equal(ov, v[vm >= 0]) and np.array_equal(oc, c[vm >= 0])
