"""Mesh clean-up after the extraction, on the gfx950 kernels of csrc/mesh_clean.hip: what a user of the reference does with Open3D after
tsdf_integrate.py (simplify_vertex_clustering; cluster_connected_triangles + remove_triangles_by_mask), with every step in a fixed order
so that the result is one definite set of bits (tests/mesh_clean_oracle.py restates both in numpy).

  simplify_vertex_clustering(mesh, cell)                  one vertex per occupied cell of the voxel downsample's grid, faces remapped,
                                                          degenerate and duplicate faces and unreferenced clusters dropped
  remove_small_components(mesh, min_faces | keep_largest) connected components by min-label hooking and pointer jumping, small ones dropped
  clean(mesh, cell, min_faces | keep_largest)             the first, then the second: clustering can merge a fragment into the surface

A mesh is a tsdf.Mesh of numpy arrays (uploaded, cleaned on the GPU, downloaded) or the same three arrays as contiguous GPU tensors
(vertices fp32 [V,3], colors u8 [V,3] or None, faces int32 [F,3]); the result and the arrays of `info` are of the kind of the input.

  python -m cut3r_slam_amd.mesh_clean IN.ply OUT.ply [--cell C] [--min-faces N | --keep-largest K]
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .tsdf import Mesh, read_ply, write_ply

DEVICE = "cuda:0"


def _to_device(mesh):
    """(vertices, colors, faces as GPU tensors, was_numpy)"""
    v, c, f = mesh
    if isinstance(v, torch.Tensor):
        return v, c, f, False
    v = torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(DEVICE)
    f = torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(DEVICE)
    c = None if c is None else torch.from_numpy(np.ascontiguousarray(c, np.uint8)).to(DEVICE)
    return v, c, f, True


def _result(r, names, as_numpy):
    conv = (lambda t: None if t is None else t.cpu().numpy()) if as_numpy else (lambda t: t)
    mesh = Mesh(conv(r["vertices"]), conv(r["colors"]), conv(r["faces"]))
    return mesh, {k: (conv(r[k]) if isinstance(r[k], torch.Tensor) else r[k]) for k in names}


@torch.no_grad()
def simplify_vertex_clustering(mesh, cell, timing=None):
    """(Mesh, info).  1. the frame of ops.voxel_downsample over ALL vertices (lo = (double)min - cell / 2, index floor(((double)p - lo) /
    cell), key ix << 42 | iy << 21 | iz); 2. the clusters are the occupied cells in ascending key order; 3. a cluster's position is the
    fp64 sum of its vertices in ascending vertex index divided by their number, rounded once to fp32, its colour the same mean,
    floor(mean + 0.5): the rows of ops.voxel_downsample; 4. a face becomes the triple of its clusters, is dropped when two are equal
    (degenerate), else rotated so that the smallest id leads (orientation kept), and of equal triples the smallest input face index stays
    (duplicate); survivors in input order; 5. clusters no survivor references are dropped, the rest renumbered in order.
    info: vertex_map int32 [V] (new index of the vertex's cluster, or -1), face_map int32 [F'] (input index of each survivor), clusters,
    degenerate, duplicate, unreferenced.  An empty result is valid.  ValueError: see ops.mesh_cluster."""
    v, c, f, as_numpy = _to_device(mesh)
    r = ops.mesh_cluster(v, c, f, cell, timing=timing)
    return _result(r, ("vertex_map", "face_map", "clusters", "degenerate", "duplicate", "unreferenced"), as_numpy)


@torch.no_grad()
def remove_small_components(mesh, min_faces=None, keep_largest=None, timing=None):
    """(Mesh, info).  Two vertices are connected when a face holds both; label(v) is the smallest vertex index of v's component; a face
    belongs to the component of its first vertex and a component's size is its number of faces.  min_faces=n keeps the components of size
    >= n, keep_largest=k the first k by (size descending, label ascending); exactly one of the two.  Faces stay in input order, vertices
    no kept face references (those in no face included) are dropped, the rest keep their order.
    info: labels int32 [V], components int32 [K,2] = (label, size) of the kept ones by (size descending, label ascending), n_components,
    vertex_map, face_map, rounds (labelling rounds run).  ValueError: see ops.mesh_components."""
    v, c, f, as_numpy = _to_device(mesh)
    r = ops.mesh_components(v, c, f, min_faces=min_faces, keep_largest=keep_largest, timing=timing)
    return _result(r, ("labels", "components", "n_components", "vertex_map", "face_map", "rounds"), as_numpy)


@torch.no_grad()
def clean(mesh, cell=None, min_faces=None, keep_largest=None):
    """(Mesh, info): simplify_vertex_clustering when `cell` is given, then remove_small_components when one of its options is; info =
    {"cluster": ..., "components": ...} of the steps that ran.  A mesh the clustering empties is returned as it is."""
    if min_faces is not None and keep_largest is not None:
        raise ValueError("at most one of min_faces and keep_largest")
    if cell is None and min_faces is None and keep_largest is None:
        raise ValueError("clean: nothing asked (cell, min_faces or keep_largest)")
    info = {}
    if cell is not None:
        mesh, info["cluster"] = simplify_vertex_clustering(mesh, cell)
    if (min_faces is not None or keep_largest is not None) and len(mesh.faces):
        mesh, info["components"] = remove_small_components(mesh, min_faces=min_faces, keep_largest=keep_largest)
    return mesh, info


def main(argv=None) -> int:
    import argparse
    p = argparse.ArgumentParser(description="vertex clustering and small-component removal of a PLY mesh on the GPU")
    p.add_argument("input")
    p.add_argument("output")
    p.add_argument("--cell", type=float, default=None, help="vertex-clustering cell size in scene units")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--min-faces", type=int, default=None, help="drop connected components of fewer faces")
    g.add_argument("--keep-largest", type=int, default=None, help="keep only this many of the largest connected components")
    a = p.parse_args(argv)
    if a.cell is None and a.min_faces is None and a.keep_largest is None:
        p.error("nothing asked: --cell, --min-faces or --keep-largest")
    mesh = read_ply(a.input)
    out, info = clean(mesh, cell=a.cell, min_faces=a.min_faces, keep_largest=a.keep_largest)
    write_ply(a.output, out)
    print(f"{a.input}: {len(mesh.vertices)} vertices, {len(mesh.faces)} faces -> {a.output}: {len(out.vertices)} vertices, {len(out.faces)} faces")
    if "cluster" in info:
        i = info["cluster"]
        print(f"  clustering at {a.cell:g}: {i['clusters']} clusters ({i['unreferenced']} unreferenced), {i['degenerate']} degenerate and "
              f"{i['duplicate']} duplicate faces dropped")
    if "components" in info:
        i = info["components"]
        print(f"  components: {len(i['components'])} of {i['n_components']} kept, {i['rounds']} labelling rounds")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
