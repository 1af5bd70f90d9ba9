"""The standard 3DGS PLY file, out and in: what hislam2/gaussian/scene/gaussian_model.py:433-470 (`construct_list_of_attributes`, `save_ply`)
writes and every splat viewer opens.  `binary_little_endian 1.0`, one `vertex` element, every property a `float`, in the order

    x y z  nx ny nz  f_dc_0..2  f_rest_0..(3 (K - 1) - 1)  opacity  scale_0..2  rot_0..3

with the RAW parameters: opacity logit, log scale, unnormalised quaternion (r, x, y, z), SH coefficients; the normals are zeros.  f_rest is
channel-major as in `save_ply` (features_rest [P,K-1,3] transposed to [P,3,K-1], then flattened): f_rest_{c (K - 1) + j} is coefficient j + 1
of channel c.  numpy structured arrays, like tsdf.write_ply; `plyfile` is not a dependency.  The layout is read off the reference's source;
parity with a file the reference itself wrote is UNPINNED (its backend cannot run here)."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

SH_C0 = 0.28209479177387814
_REQUIRED = ("x", "y", "z", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3")
_PLY_SIZES = {"char": 1, "int8": 1, "uchar": 1, "uint8": 1, "short": 2, "int16": 2, "ushort": 2, "uint16": 2, "int": 4, "int32": 4, "uint": 4,
              "uint32": 4, "float": 4, "float32": 4, "double": 8, "float64": 8}
_FLOAT = ("float", "float32")


def attribute_names(K):
    """construct_list_of_attributes (gaussian_model.py:433-445) for K SH coefficients per channel"""
    return (["x", "y", "z", "nx", "ny", "nz"] + [f"f_dc_{i}" for i in range(3)] + [f"f_rest_{i}" for i in range(3 * (K - 1))] + ["opacity"]
            + [f"scale_{i}" for i in range(3)] + [f"rot_{i}" for i in range(4)])


def _host(t, cols):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).reshape(-1, cols) if cols else np.ascontiguousarray(a, np.float32)


def write_gaussian_ply(path, xyz, f_dc, f_rest, opacity, scaling, rotation):
    """xyz [P,3], f_dc [P,3] or [P,1,3], f_rest [P,K-1,3] (None or K = 1: no f_rest properties), opacity [P] or [P,1] (logit), scaling [P,3]
    (log), rotation [P,4] (r, x, y, z; as stored); tensors or arrays, written as fp32 bit for bit"""
    xyz = _host(xyz, 3)
    P = xyz.shape[0]
    f_dc, opacity, scaling, rotation = _host(f_dc, 3), _host(opacity, 1), _host(scaling, 3), _host(rotation, 4)
    rest = np.zeros((P, 0, 3), np.float32) if f_rest is None else _host(f_rest, 0)
    if rest.ndim != 3 or rest.shape[0] != P or rest.shape[2] != 3:
        raise ValueError(f"f_rest: [P,K-1,3], got {list(rest.shape)}")
    K = rest.shape[1] + 1
    if K not in (1, 4, 9, 16):
        raise ValueError(f"f_rest: K - 1 = {K - 1} coefficients per channel; K must be 1, 4, 9 or 16")
    for name, a in (("f_dc", f_dc), ("opacity", opacity), ("scaling", scaling), ("rotation", rotation)):
        if a.shape[0] != P:
            raise ValueError(f"{name}: {a.shape[0]} rows for {P} Gaussians")
    names = attribute_names(K)
    cols = np.concatenate([xyz, np.zeros((P, 3), np.float32), f_dc, rest.transpose(0, 2, 1).reshape(P, 3 * (K - 1)), opacity, scaling, rotation], 1)
    vert = np.empty(P, np.dtype([(n, "<f4") for n in names]))
    for i, n in enumerate(names):
        vert[n] = cols[:, i]
    header = "ply\nformat binary_little_endian 1.0\n" + f"element vertex {P}\n" + "".join(f"property float {n}\n" for n in names) + "end_header\n"
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(vert.tobytes())


def read_gaussian_ply(path):
    """-> dict of fp32 arrays xyz [P,3], f_dc [P,3], f_rest [P,K-1,3], opacity [P,1], scaling [P,3], rotation [P,4] and K.  Properties are
    found by NAME in any order, unknown ones (and other elements after the vertices) are skipped, nx ny nz may be missing.  ValueError:
    not a PLY, ascii or big-endian, no vertex element first, a list property among the vertices, a required property missing or not a
    float, a number of f_rest_* properties that is not 3 (K - 1) with K in {1, 4, 9, 16} (or names that are not f_rest_0 .. f_rest_{n-1}),
    a body shorter than the header promises."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    lines = [ln.split() for ln in data[:end].decode("ascii", "replace").splitlines()]
    fmt = [ln for ln in lines if ln[:1] == ["format"]]
    if len(fmt) != 1 or fmt[0][1:] != ["binary_little_endian", "1.0"]:
        raise ValueError(f"{path}: only binary_little_endian 1.0 PLY is read (format line: {' '.join(fmt[0]) if fmt else 'none'})")
    count, props, seen = None, [], 0
    for ln in lines:
        if ln[:1] == ["element"]:
            seen += 1
            if seen == 1:
                if len(ln) != 3 or ln[1] != "vertex":
                    raise ValueError(f"{path}: the first element must be `vertex`")
                count = int(ln[2])
        elif ln[:1] == ["property"] and seen == 1:
            if ln[1] == "list" or len(ln) != 3 or ln[1] not in _PLY_SIZES:
                raise ValueError(f"{path}: vertex property `{' '.join(ln[1:])}` is not a scalar of a known type")
            props.append((ln[2], ln[1]))
    if count is None or count < 0:
        raise ValueError(f"{path}: no vertex element")
    types = dict(props)
    if len(types) != len(props):
        raise ValueError(f"{path}: a vertex property is declared twice")
    for n in _REQUIRED:
        if n not in types:
            raise ValueError(f"{path}: required property {n} is missing")
    rest = [n for n in types if n.startswith("f_rest_")]
    n_rest = len(rest)
    K = n_rest // 3 + 1
    if n_rest % 3 or K not in (1, 4, 9, 16) or set(rest) != {f"f_rest_{i}" for i in range(n_rest)}:
        raise ValueError(f"{path}: {n_rest} f_rest properties; 3 (K - 1) with K in 1, 4, 9, 16 are read, named f_rest_0 .. f_rest_{{n-1}}")
    for n in _REQUIRED + tuple(rest):
        if types[n] not in _FLOAT:
            raise ValueError(f"{path}: property {n} is {types[n]}, not float")
    dt = np.dtype([(n, "<f4" if t in _FLOAT else f"V{_PLY_SIZES[t]}") for n, t in props])
    off = end + len(b"end_header\n")
    if len(data) - off < dt.itemsize * count:
        raise ValueError(f"{path}: body of {len(data) - off} bytes, the header promises {count} x {dt.itemsize}")
    arr = np.frombuffer(data, dt, count, off)
    col = lambda names: np.stack([arr[n] for n in names], 1).astype(np.float32) if names else np.zeros((count, 0), np.float32)
    f_rest = col([f"f_rest_{i}" for i in range(n_rest)]).reshape(count, 3, K - 1).transpose(0, 2, 1)
    return {"xyz": col(["x", "y", "z"]), "f_dc": col(["f_dc_0", "f_dc_1", "f_dc_2"]), "f_rest": np.ascontiguousarray(f_rest),
            "opacity": col(["opacity"]), "scaling": col(["scale_0", "scale_1", "scale_2"]), "rotation": col([f"rot_{i}" for i in range(4)]),
            "K": K}


class GaussianCloud:
    """A frozen, inference-only set of Gaussians of any SH degree 0..3 (a file of another trainer, or a GaussianMap at degree 0) with the
    activations of GaussianMap: what gs_view.render_cloud rasterises.  xyz [P,3], features [P,K,3] (DC first), opacity [P,1] (logit),
    scaling [P,3] (log), rotation [P,4] (r, x, y, z; unnormalised)."""
    __slots__ = ("xyz", "features", "opacity", "scaling", "rotation", "sh_degree")

    def __init__(self, xyz, features, opacity, scaling, rotation):
        K = int(features.shape[1])
        if K not in (1, 4, 9, 16):
            raise ValueError(f"features: [P,K,3] with K in 1, 4, 9, 16, got K = {K}")
        dev = xyz.device
        fix = lambda t, *s: t.detach().to(dev, torch.float32).reshape(*s).contiguous()
        P = xyz.shape[0]
        for name, t in (("xyz", fix(xyz, P, 3)), ("features", fix(features, P, K, 3)), ("opacity", fix(opacity, P, 1)),
                        ("scaling", fix(scaling, P, 3)), ("rotation", fix(rotation, P, 4)), ("sh_degree", math.isqrt(K) - 1)):
            object.__setattr__(self, name, t)

    def __setattr__(self, name, value):
        raise AttributeError("GaussianCloud is frozen")

    def __len__(self):
        return self.xyz.shape[0]

    @property
    def get_xyz(self):
        return self.xyz

    @property
    def get_features(self):
        return self.features

    @property
    def get_opacity(self):
        return torch.sigmoid(self.opacity)

    @property
    def get_scaling(self):
        return torch.exp(self.scaling)

    @property
    def get_rotation(self):
        return F.normalize(self.rotation, dim=-1)

    @classmethod
    def from_ply(cls, path, device="cuda:0"):
        d = read_gaussian_ply(path)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        return cls(t(d["xyz"]), torch.cat([t(d["f_dc"])[:, None, :], t(d["f_rest"])], 1), t(d["opacity"]), t(d["scaling"]), t(d["rotation"]))

    @classmethod
    def from_map(cls, gaussian_map):
        th = gaussian_map.theta.detach()
        return cls(th[:, 0:3], th[:, None, 3:6], th[:, 6:7], th[:, 7:10], th[:, 10:14])

    def save_ply(self, path):
        write_gaussian_ply(path, self.xyz, self.features[:, 0], self.features[:, 1:], self.opacity, self.scaling, self.rotation)
