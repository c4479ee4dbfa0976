"""Mesh export: a density function sampled on a lattice -> a welded, oriented, indexed triangle mesh on the device
(kernels.mesh_extract: marching tetrahedra, csrc/mesh.hip) -> PLY / OBJ files.

The surface is the level set density = threshold; face and vertex normals point towards lower density, the convention
of InstantNGP.normals.  Marching tetrahedra emits roughly 2-3 times the triangles of marching cubes at the same
resolution, and a lattice value exactly on the threshold gives zero-area triangles; both are kept as they are (no
simplification, no degenerate removal), so the connectivity is always closed inside the box.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence, Union

import numpy as np
import torch

from . import kernels as K

__all__ = ["Mesh", "density_lattice", "extract_mesh"]


class Mesh:
    """vertices (V,3) float32, faces (F,3) int32, optional per-vertex normals (V,3) float32; device or host tensors."""

    def __init__(self, vertices, faces, normals=None):
        if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
            raise ValueError(f"vertices (V,3) and faces (F,3) expected, got {tuple(vertices.shape)}, {tuple(faces.shape)}")
        if normals is not None and tuple(normals.shape) != tuple(vertices.shape):
            raise ValueError(f"normals must be {tuple(vertices.shape)}, got {tuple(normals.shape)}")
        self.vertices, self.faces, self.normals = vertices, faces, normals

    def __repr__(self):
        return (f"Mesh(V={self.vertices.shape[0]}, F={self.faces.shape[0]}, normals={self.normals is not None}, "
                f"device={self.vertices.device})")

    def cpu(self) -> "Mesh":
        return Mesh(self.vertices.cpu(), self.faces.cpu(), None if self.normals is None else self.normals.cpu())

    def _host(self):
        v = self.vertices.detach().cpu().numpy().astype("<f4")
        f = self.faces.detach().cpu().numpy().astype("<i4")
        n = None if self.normals is None else self.normals.detach().cpu().numpy().astype("<f4")
        return v, f, n

    def save_ply(self, path) -> None:
        """Binary little-endian PLY: float x y z [nx ny nz] per vertex, `list uchar int vertex_indices` per face."""
        v, f, n = self._host()
        props = ["x", "y", "z"] + (["nx", "ny", "nz"] if n is not None else [])
        header = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}"]
        header += [f"property float {p}" for p in props]
        header += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
        rec = np.empty(f.shape[0], dtype=[("n", "u1"), ("v", "<i4", (3,))])
        rec["n"], rec["v"] = 3, f
        with open(path, "wb") as fh:
            fh.write(("\n".join(header) + "\n").encode("ascii"))
            fh.write(np.ascontiguousarray(v if n is None else np.concatenate([v, n], 1)).tobytes())
            fh.write(rec.tobytes())

    def save_obj(self, path) -> None:
        """Wavefront OBJ: v lines, vn lines when there are normals, 1-based f lines (a//a with normals); %.9g keeps
        every float32 exactly."""
        v, f, n = self._host()
        with open(path, "w") as fh:
            for x in v.tolist():
                fh.write("v %.9g %.9g %.9g\n" % tuple(x))
            if n is not None:
                for x in n.tolist():
                    fh.write("vn %.9g %.9g %.9g\n" % tuple(x))
            fmt = "f %d//%d %d//%d %d//%d\n" if n is not None else "f %d %d %d\n"
            for a, b, c in (f + 1).tolist():
                fh.write(fmt % ((a, a, b, b, c, c) if n is not None else (a, b, c)))


def _box(lo, hi):
    lo = [float(x) for x in (lo.reshape(-1).tolist() if isinstance(lo, torch.Tensor) else lo)]
    hi = [float(x) for x in (hi.reshape(-1).tolist() if isinstance(hi, torch.Tensor) else hi)]
    if len(lo) != 3 or len(hi) != 3 or not all(a < b for a, b in zip(lo, hi)):
        raise ValueError(f"lo / hi must be 3 floats each with lo < hi, got {lo} vs {hi}")
    return lo, hi


def _resolution(resolution):
    r = (int(resolution),) * 3 if isinstance(resolution, int) else tuple(int(v) for v in resolution)
    if len(r) != 3 or min(r) < 2:
        raise ValueError(f"resolution must be an int or a triple, every entry >= 2, got {resolution!r}")
    return r


def density_lattice(density_fn: Callable, lo, hi, resolution: Union[int, Sequence[int]], chunk: int = 2 ** 20,
                    device=None) -> torch.Tensor:
    """density_fn((M,3) world points) -> (M,1) evaluated at the lattice lo + (ix,iy,iz) (hi - lo) / (n - 1), in chunks
    of ``chunk`` points generated on the device: (nx,ny,nz) float32, contiguous.  Every point is evaluated on its own,
    so the result does not depend on ``chunk`` for a density_fn that treats its rows independently."""
    lo, hi = _box(lo, hi)
    nx, ny, nz = _resolution(resolution)
    if chunk < 1:
        raise ValueError(f"chunk must be positive, got {chunk}")
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    P = nx * ny * nz
    lo_t = torch.tensor(lo, dtype=torch.float32, device=device)
    h = (torch.tensor(hi, dtype=torch.float32, device=device) - lo_t) / torch.tensor(
        [nx - 1, ny - 1, nz - 1], dtype=torch.float32, device=device)
    out = torch.empty(P, dtype=torch.float32, device=device)
    with torch.no_grad():
        for s in range(0, P, chunk):
            p = torch.arange(s, min(s + chunk, P), device=device)
            r = torch.div(p, nz, rounding_mode="floor")
            idx = torch.stack([torch.div(r, ny, rounding_mode="floor"), r % ny, p % nz], -1)
            sig = density_fn(lo_t + idx.to(torch.float32) * h)
            out[s:s + p.numel()] = sig.reshape(-1).to(torch.float32)
    return out.view(nx, ny, nz)


def extract_mesh(density_fn: Callable, lo, hi, resolution: Union[int, Sequence[int]], threshold: float,
                 normals: Union[str, None, Callable] = "grid", chunk: int = 2 ** 20, device=None) -> Mesh:
    """The level set density_fn = threshold inside the box [lo, hi] as a Mesh on the device.  normals: "grid" (the
    lattice's central differences, from the extraction kernel), None, or a callable evaluated at the vertices
    ((V,3) -> (V,3))."""
    if not (normals is None or normals == "grid" or callable(normals)):
        raise ValueError(f"normals must be 'grid', None or a callable, got {normals!r}")
    lo, hi = _box(lo, hi)
    field = density_lattice(density_fn, lo, hi, resolution, chunk=chunk, device=device)
    if normals == "grid":
        return Mesh(*K.mesh_extract(field, threshold, lo, hi, normals=True))
    verts, faces = K.mesh_extract(field, threshold, lo, hi)
    nrm: Optional[torch.Tensor] = None
    if callable(normals):
        nrm = normals(verts) if verts.shape[0] else torch.empty_like(verts)
    return Mesh(verts, faces, nrm)
