"""numpy restatement of csrc/mesh_clean.hip: vertex clustering of a mesh on the voxel downsample of tests/cloud_oracle.py, and removal of
small connected components by plain propagate-and-jump.  Every array matches the GPU bit for bit, the round count included."""
import numpy as np

from tests import cloud_oracle as CO


def cluster_ids(vertices, cell):
    """(cid int64 [V], M): the cluster of every vertex, clusters numbered in ascending key order"""
    _, key = CO.voxel_keys(vertices, cell)
    uniq, cid = np.unique(key, return_inverse=True)
    return cid.reshape(-1), len(uniq)


def rotate_smallest_first(t):
    """rows of [n,3] rotated cyclically so that the smallest entry leads"""
    k = np.argmin(t, axis=1)
    r = np.arange(len(t))
    return np.stack([t[r, (k + j) % 3] for j in range(3)], 1)


def simplify_vertex_clustering(vertices, colors, faces, cell):
    """(vertices f32 [V',3], colors u8 [V',3] | None, faces i32 [F',3], info)"""
    v = np.asarray(vertices, np.float32)
    f = np.asarray(faces, np.int64)
    cv, cc, _ = CO.voxel_downsample(v, cell, colors)         # the clusters before the unreferenced ones are dropped
    cid, M = cluster_ids(v, cell)
    assert M == len(cv)
    t = cid[f]
    deg = (t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 0] == t[:, 2])
    idx = np.flatnonzero(~deg)
    rot = rotate_smallest_first(t[idx]) if len(idx) else np.zeros((0, 3), np.int64)
    if len(idx):
        _, first = np.unique(rot, axis=0, return_index=True)  # the first (smallest face index) of every distinct triple
        keep = np.sort(first)
    else:
        keep = np.zeros(0, np.int64)
    face_map = idx[keep]
    tri = rot[keep]
    ref = np.zeros(M, bool)
    ref[tri.reshape(-1)] = True
    newid = np.where(ref, np.cumsum(ref) - 1, -1)
    info = {"vertex_map": newid[cid].astype(np.int32), "face_map": face_map.astype(np.int32), "clusters": M, "degenerate": int(deg.sum()),
            "duplicate": int(len(idx) - len(keep)), "unreferenced": int(M - ref.sum()), "cluster_vertices": cv, "cluster_colors": cc,
            "cluster_of_vertex": cid}
    return cv[ref], None if cc is None else cc[ref], newid[tri].astype(np.int32).reshape(-1, 3), info


def component_labels(faces, V):
    """(labels int64 [V], rounds).  One round: every face lowers its three vertices and the three labels they carry to its smallest
    label (np.minimum.at, from the labels of the round's start), then every vertex jumps to the end of its chain; the loop ends with the
    first round in which no face saw two labels."""
    f = np.asarray(faces, np.int64)
    L = np.arange(V, dtype=np.int64)
    rounds = 0
    while True:
        lab = L[f]
        m = lab.min(1)
        changed = bool((lab != m[:, None]).any())
        new = L.copy()
        for k in range(3):
            np.minimum.at(new, f[:, k], m)
            np.minimum.at(new, lab[:, k], m)
        while True:
            j = new[new]
            if np.array_equal(j, new):
                break
            new = j
        L = new
        rounds += 1
        if not changed:
            return L, rounds


def remove_small_components(vertices, colors, faces, min_faces=None, keep_largest=None):
    """(vertices, colors, faces, info)"""
    assert (min_faces is None) != (keep_largest is None)
    v = np.asarray(vertices, np.float32)
    f = np.asarray(faces, np.int64)
    V = len(v)
    L, rounds = component_labels(f, V)
    size = np.bincount(L[f[:, 0]], minlength=V)
    labels = np.flatnonzero(size)
    order = labels[np.lexsort((labels, -size[labels]))]      # size descending, label ascending
    kept = order[size[order] >= min_faces] if min_faces is not None else order[:keep_largest]
    mark = np.zeros(V, bool)
    mark[kept] = True
    fkeep = mark[L[f[:, 0]]]
    ref = np.zeros(V, bool)
    ref[f[fkeep].reshape(-1)] = True
    newid = np.where(ref, np.cumsum(ref) - 1, -1)
    info = {"labels": L.astype(np.int32), "components": np.stack([kept, size[kept]], 1).astype(np.int32).reshape(-1, 2),
            "n_components": len(labels), "vertex_map": newid.astype(np.int32), "face_map": np.flatnonzero(fkeep).astype(np.int32),
            "rounds": rounds}
    return v[ref], None if colors is None else np.asarray(colors, np.uint8)[ref], newid[f[fkeep]].astype(np.int32).reshape(-1, 3), info


def clean(vertices, colors, faces, cell=None, min_faces=None, keep_largest=None):
    v, c, f = vertices, colors, faces
    if cell is not None:
        v, c, f, _ = simplify_vertex_clustering(v, c, f, cell)
    if (min_faces is not None or keep_largest is not None) and len(f):
        v, c, f, _ = remove_small_components(v, c, f, min_faces, keep_largest)
    return v, c, f


_SPHERE = []


def sphere_mesh():
    """the raw extraction of the small sphere scene of tests/tsdf_oracle.py (12 views of 48x64, voxel 0.04), computed once and shared:
    (vertices f32 [V,3], colors u8 [V,3], faces i32 [F,3]); nobody writes into it"""
    if not _SPHERE:
        from tests import tsdf_oracle as O
        depth, rgb, w2c, K = O.sphere_scene(n_views=12, H=48, W=64, f=55.0)
        origin, dims, trunc = O.sphere_grid(voxel=0.04)
        vol = O.integrate(O.new_volume(dims), origin, 0.04, depth, w2c, K, trunc, 5.0, rgb=rgb)
        v, c, f = O.extract(vol, origin, 0.04, 1.0)
        _SPHERE.append((v, c, f))
    return _SPHERE[0]
