"""Mesh export: a density function sampled on a lattice -> a welded, oriented, indexed triangle mesh on the device
(kernels.mesh_extract: marching tetrahedra, csrc/mesh.hip) -> PLY / OBJ files.

The surface is the level set density = threshold; face and vertex normals point towards lower density, the convention
of InstantNGP.normals.  Marching tetrahedra emits roughly 2-3 times the triangles of marching cubes at the same
resolution, and a lattice value exactly on the threshold gives zero-area triangles; the extractor keeps both as they
are, so its connectivity is always closed inside the box.

extract_mesh(method="dual") extracts by dual contouring instead (csrc/mesh_dual.hip): one vertex per
sign-changing cell, placed by the plane quadric of the cell's crossing points and normals so that it can sit on a crease
or a corner of the level set, and one quad per sign-changing lattice edge, about a third of the triangles.  The crossing
points can be refined by bisection and the normals can come from the field itself.  The surface is open at the box, and
a cell that two sheets cross still gets one vertex, so a noisy field can give edges shared by more than two triangles.

Clean-up on the device (csrc/mesh_clean.hip): Mesh.components labels the connected components,
Mesh.filter_components keeps whole components by their number of faces (the small detached blobs of a trained density
field go), Mesh.select_faces compacts to any subset of the faces; normals and colours ride along.

Simplification on the device (csrc/mesh_simplify.hip): Mesh.simplify clusters the vertices on a grid
of cells (one vertex per occupied cell, collapsed and duplicated faces dropped); a tiny cell welds coincident vertices
and removes the zero-area triangles.

Smoothing on the device (csrc/mesh_smooth.hip): Mesh.smooth runs Taubin (or plain Laplacian) passes
over a CSR vertex adjacency built once, with open boundaries held fixed by default; Mesh.compute_normals derives
area-weighted vertex normals from the faces.

Metrics on the device (csrc/mesh_metrics.hip, nerf_amd/mesh_metrics.py): Mesh.face_areas / area,
Mesh.sample_surface draws points uniformly by area, Mesh.distance_to reports Chamfer, Hausdorff, F-score and normal
consistency against another mesh.  Mesh.closest_points and distance_to(exact=True) measure against the triangles
themselves (csrc/mesh_distance.hip).

Ray casting on the device (csrc/mesh_raycast.hip): Mesh.ray_cast returns the nearest face every ray
hits, through the same face grid, and Mesh.render the depth, mask, face, normal and colour images of a pinhole view,
with depth in the ray parameter of ray_rendering.render_image.

Texture baking on the device (csrc/mesh_texture.hip): Mesh.atlas gives every texel of a per-face
texture atlas its surface point and normal, Mesh.bake_texture fills the texture from any colour function,
Mesh.sample_texture and the "texture" image of Mesh.render fetch it by (face, barycentric pair), and save_obj writes a
textured OBJ with its MTL and PNG: the colour detail no longer falls with the triangle count.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence, Union

import numpy as np
import torch

from . import kernels as K

__all__ = ["Mesh", "density_lattice", "extract_mesh"]


class Mesh:
    """vertices (V,3) float32, faces (F,3) int32, optional per-vertex normals (V,3) float32 and colours (V,3) float32
    in [0,1]; device or host tensors.  Optionally a texture (T,T,3) float32 in [0,1] over the per-face atlas of
    (F, texels), with texels the side of an atlas cell; bake_texture sets both."""

    def __init__(self, vertices, faces, normals=None, colors=None, texture=None, texels=None):
        if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
            raise ValueError(f"vertices (V,3) and faces (F,3) expected, got {tuple(vertices.shape)}, {tuple(faces.shape)}")
        if normals is not None and tuple(normals.shape) != tuple(vertices.shape):
            raise ValueError(f"normals must be {tuple(vertices.shape)}, got {tuple(normals.shape)}")
        if colors is not None and tuple(colors.shape) != tuple(vertices.shape):
            raise ValueError(f"colors must be {tuple(vertices.shape)}, got {tuple(colors.shape)}")
        if (texture is None) != (texels is None):
            raise ValueError("texture and texels go together")
        self.vertices, self.faces, self.normals, self.colors = vertices, faces, normals, colors
        self.texture, self.texels = texture, texels
        if texture is not None:
            self._texture_side()

    def __repr__(self):
        colors = "" if self.colors is None else ", colors=True"  # a mesh without colours prints as it always has
        texture = "" if self.texture is None else f", texture={self.texture.shape[0]}"  # and one without a texture too
        return (f"Mesh(V={self.vertices.shape[0]}, F={self.faces.shape[0]}, normals={self.normals is not None}"
                f"{colors}{texture}, device={self.vertices.device})")

    def cpu(self) -> "Mesh":
        return Mesh(self.vertices.cpu(), self.faces.cpu(), None if self.normals is None else self.normals.cpu(),
                    None if self.colors is None else self.colors.cpu(),
                    None if self.texture is None else self.texture.cpu(), self.texels)

    def _host(self):
        v = self.vertices.detach().cpu().numpy().astype("<f4")
        f = self.faces.detach().cpu().numpy().astype("<i4")
        n = None if self.normals is None else self.normals.detach().cpu().numpy().astype("<f4")
        return v, f, n

    def _host_colors(self):
        return None if self.colors is None else self.colors.detach().cpu().numpy().astype("<f4")

    def save_ply(self, path) -> None:
        """Binary little-endian PLY: float x y z [nx ny nz] [uchar red green blue = round(clamp(c,0,1) 255)] per
        vertex, `list uchar int vertex_indices` per face."""
        v, f, n = self._host()
        c = self._host_colors()
        props = ["x", "y", "z"] + (["nx", "ny", "nz"] if n is not None else [])
        header = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}"]
        header += [f"property float {p}" for p in props]
        if c is not None:
            header += [f"property uchar {p}" for p in ("red", "green", "blue")]
        header += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
        rec = np.empty(f.shape[0], dtype=[("n", "u1"), ("v", "<i4", (3,))])
        rec["n"], rec["v"] = 3, f
        xyz = np.ascontiguousarray(v if n is None else np.concatenate([v, n], 1))
        with open(path, "wb") as fh:
            fh.write(("\n".join(header) + "\n").encode("ascii"))
            if c is None:
                fh.write(xyz.tobytes())
            else:
                vrec = np.empty(v.shape[0], dtype=[("f", "<f4", (xyz.shape[1],)), ("c", "u1", (3,))])
                vrec["f"] = xyz
                vrec["c"] = np.rint(np.clip(np.nan_to_num(c, nan=0.0), 0.0, 1.0) * 255.0).astype(np.uint8)
                fh.write(vrec.tobytes())
            fh.write(rec.tobytes())

    def save_obj(self, path) -> None:
        """Wavefront OBJ: v lines (`v x y z r g b` with colours, the common extension), vn lines when there are normals,
        1-based f lines (a//a with normals); %.9g keeps every float32 exactly.  A textured mesh also gets vt lines,
        three per face in the faces' order (u = x / T, v = 1 - y / T of atlas_uv), f lines a/t/n (a/t without normals),
        `mtllib` and `usemtl`, and beside the OBJ a .mtl that names a .png of the same stem with the texture as
        round(clamp(c,0,1) 255), row 0 on top."""
        if self.texture is not None:
            return self._save_textured_obj(path)
        v, f, n = self._host()
        c = self._host_colors()
        with open(path, "w") as fh:
            if c is None:
                for x in v.tolist():
                    fh.write("v %.9g %.9g %.9g\n" % tuple(x))
            else:
                for x in np.concatenate([v, c], 1).tolist():
                    fh.write("v %.9g %.9g %.9g %.9g %.9g %.9g\n" % tuple(x))
            if n is not None:
                for x in n.tolist():
                    fh.write("vn %.9g %.9g %.9g\n" % tuple(x))
            fmt = "f %d//%d %d//%d %d//%d\n" if n is not None else "f %d %d %d\n"
            for i, j, k in (f + 1).tolist():
                fh.write(fmt % ((i, i, j, j, k, k) if n is not None else (i, j, k)))

    def _save_textured_obj(self, path) -> None:
        import os

        from PIL import Image
        T = self._texture_side()
        v, f, n = self._host()
        c = self._host_colors()
        uv = self.atlas_uv().detach().cpu().numpy().astype(np.float64).reshape(-1, 2)
        path = os.fspath(path)
        stem = os.path.splitext(path)[0]
        name = os.path.basename(stem)
        tex = self.texture.detach().cpu().numpy().astype("<f4")
        png = np.rint(np.clip(np.nan_to_num(tex, nan=0.0), 0.0, 1.0) * 255.0).astype(np.uint8)
        Image.fromarray(np.ascontiguousarray(png)).save(stem + ".png")
        with open(stem + ".mtl", "w") as fh:
            fh.write(f"newmtl {name}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {name}.png\n")
        with open(path, "w") as fh:
            fh.write(f"mtllib {name}.mtl\n")
            if c is None:
                for x in v.tolist():
                    fh.write("v %.9g %.9g %.9g\n" % tuple(x))
            else:
                for x in np.concatenate([v, c], 1).tolist():
                    fh.write("v %.9g %.9g %.9g %.9g %.9g %.9g\n" % tuple(x))
            for x, y in uv.tolist():
                fh.write("vt %.9g %.9g\n" % (x / T, 1.0 - y / T))
            if n is not None:
                for x in n.tolist():
                    fh.write("vn %.9g %.9g %.9g\n" % tuple(x))
            fh.write(f"usemtl {name}\n")
            fmt = "f %d/%d/%d %d/%d/%d %d/%d/%d\n" if n is not None else "f %d/%d %d/%d %d/%d\n"
            for t, (i, j, k) in enumerate((f + 1).tolist()):
                t = 3 * t + 1
                fh.write(fmt % ((i, t, i, j, t + 1, j, k, t + 2, k) if n is not None else (i, t, j, t + 1, k, t + 2)))

    # ---- texture baking on the device (kernels.mesh_atlas_texels / mesh_texture_lookup)

    def _texture_side(self) -> int:
        """T of the mesh's own texture, after checking it against the atlas of (F, texels)."""
        if self.texture is None:
            raise ValueError("the mesh has no texture (Mesh.bake_texture)")
        t = self.texture
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 3 or t.shape[2] != 3:
            raise ValueError("texture must be a (T,T,3) float32 tensor")
        if t.shape[0] != t.shape[1]:
            raise ValueError(f"texture must be square, got {tuple(t.shape)}")
        if t.device != self.vertices.device:
            raise ValueError("texture must be on the mesh's device")
        if isinstance(self.texels, bool) or not isinstance(self.texels, int) or self.texels < K.ATLAS_MIN_TEXELS:
            raise ValueError(f"texels must be an int >= {K.ATLAS_MIN_TEXELS}, got {self.texels!r}")
        if t.shape[0] % self.texels:
            raise ValueError(f"texels = {self.texels} does not divide the texture's side {t.shape[0]}")
        T = K.atlas_layout(self.faces.shape[0], self.texels)[1]
        if t.shape[0] != T:
            raise ValueError(f"the atlas of {self.faces.shape[0]} faces at {self.texels} texels is {T} x {T}, the "
                             f"texture is {t.shape[0]} x {t.shape[0]}")
        return T

    def atlas(self, texels, normals=True) -> dict:
        """kernels.mesh_atlas_texels on this mesh: for every texel [y, x] of the T x T atlas of (F, texels) the owning
        "face" (-1: nobody's), the barycentric pair "bary", the surface "position" and (``normals``) the "normal"
        there (the mix of the mesh's vertex normals if it has them, else the face's own), and "texels", "cols", "T"."""
        return K.mesh_atlas_texels(self.vertices, self.faces, texels,
                                   vertex_normals=self.normals if normals else None, normals=normals)

    def atlas_uv(self, texels=None) -> torch.Tensor:
        """(F,3,2) float32: the UV corners of every face in texel units of its atlas (x right, y down), for
        ``texels`` (default: the mesh's own).  Small integers, a function of (F, texels) alone: the even face of a
        cell has (1,1), (S-3,1), (1,S-3), the odd one (S-1,S-1), (3,S-1), (S-1,3), plus the cell's origin."""
        S = self.texels if texels is None else texels
        if S is None:
            raise ValueError("the mesh has no texture: give texels")
        F = int(self.faces.shape[0])
        cols, _ = K.atlas_layout(F, S)
        dev = self.faces.device
        f = torch.arange(F, dtype=torch.int64, device=dev)
        cell, odd = torch.div(f, 2, rounding_mode="floor"), (f % 2)[:, None]
        origin = torch.stack([cell % cols, torch.div(cell, cols, rounding_mode="floor")], 1) * S  # (F, 2)
        even = torch.tensor([[1, 1], [S - 3, 1], [1, S - 3]], dtype=torch.int64, device=dev)
        local = torch.where(odd[:, :, None] == 1, S - even[None], even[None])  # (F, 3, 2)
        return (local + origin[:, None, :]).to(torch.float32)

    def bake_texture(self, color_fn: Callable, texels: int = 8, normals: bool = True) -> "Mesh":
        """Fill this mesh's texture: ``color_fn``(points (M,3), normals (M,3)) -> (M,3) colours in [0,1] is called
        once, on the surface points of the texels that a face owns (in the atlas's row order) and the normals there
        (None with ``normals`` = False); the result is scattered into a (T,T,3) float32 texture, unowned texels are 0.
        Sets .texture and .texels and returns self.  Gutter texels hold the colour of a nearby boundary point of
        their own face, so a bilinear fetch anywhere on a face blends that face's colours only."""
        a = self.atlas(texels, normals=normals)
        T = a["T"]
        idx = torch.nonzero(a["face"].reshape(-1) >= 0).reshape(-1)
        texture = torch.zeros((T * T, 3), dtype=torch.float32, device=self.vertices.device)
        if idx.numel():
            pts = a["position"].reshape(-1, 3)[idx]
            nrm = a["normal"].reshape(-1, 3)[idx] if normals else None
            col = color_fn(pts, nrm)
            if not isinstance(col, torch.Tensor) or tuple(col.shape) != (idx.numel(), 3):
                raise ValueError(f"color_fn must return a tensor ({idx.numel()},3)")
            texture[idx] = col.detach().to(device=texture.device, dtype=torch.float32)
        self.texture, self.texels = texture.view(T, T, 3), texels
        return self

    def sample_texture(self, face, bary) -> torch.Tensor:
        """kernels.mesh_texture_lookup on the mesh's own texture: face (N,) int32 and bary (N,2) float32 as ray_cast
        returns them -> (N,3) float32, the bilinear fetch at the point's UV; zeros where face < 0."""
        self._texture_side()
        return K.mesh_texture_lookup(self.texture, self.texels, self.faces.shape[0], face, bary)

    # ---- clean-up on the device (kernels.mesh_components / mesh_compact)

    def components(self):
        """(labels (V,) int32, face_count (V,) int32): labels[v] = the smallest vertex index of v's connected
        component, face_count[l] = the faces of the component labelled l (0 where l is no label)."""
        return K.mesh_components(self.faces, self.vertices.shape[0])

    def _compacted(self, keep, labels=None, ranges_checked=False) -> "Mesh":
        attrs = [a for a in (self.normals, self.colors) if a is not None]
        v, f, out = K.mesh_compact(self.vertices, self.faces, keep, attrs, labels=labels,
                                   ranges_checked=ranges_checked)
        out = iter(out)
        return Mesh(v, f, None if self.normals is None else next(out), None if self.colors is None else next(out))

    def select_faces(self, keep_face) -> "Mesh":
        """The mesh of the faces with keep_face ((F,) bool or uint8) set: faces and used vertices keep their order,
        the vertices are renumbered densely, normals and colours ride along."""
        if not isinstance(keep_face, torch.Tensor) or tuple(keep_face.shape) != (self.faces.shape[0],):
            raise ValueError(f"keep_face must be a ({self.faces.shape[0]},) tensor")
        return self._compacted(keep_face)

    def component_selection(self, min_faces=None, keep_largest=None):
        """(labels, face_count, keep): keep (V,) bool is set at the labels of the components that
        filter_components(min_faces, keep_largest) keeps.  The selection is a few torch ops on the device."""
        if (min_faces is None) == (keep_largest is None):
            raise ValueError("give exactly one of min_faces and keep_largest")
        if int(min_faces if keep_largest is None else keep_largest) < 0:
            raise ValueError("min_faces / keep_largest must be >= 0")
        labels, count = self.components()
        V = labels.shape[0]
        is_label = labels == torch.arange(V, dtype=torch.int32, device=labels.device)
        if min_faces is not None:
            keep = is_label & (count >= int(min_faces))
        else:
            # a stable descending sort of the face counts over the vertices in ascending order, non-labels last: a tie
            # goes to the smaller label
            key = torch.where(is_label, count, torch.full_like(count, -1))
            order = torch.sort(key, descending=True, stable=True).indices[:min(int(keep_largest), V)]
            keep = torch.zeros(V, dtype=torch.bool, device=labels.device)
            keep[order] = True
            keep &= is_label
        return labels, count, keep

    def filter_components(self, min_faces=None, keep_largest=None) -> "Mesh":
        """Keep whole connected components by their number of faces: every component with at least ``min_faces``, or
        the ``keep_largest`` components with the most faces (a tie goes to the component with the smaller label; more
        than there are keeps all).  Exactly one of the two is given."""
        labels, _, keep = self.component_selection(min_faces, keep_largest)
        return self._compacted(keep, labels=labels, ranges_checked=True)

    # ---- simplification on the device (kernels.mesh_cluster_*)

    def simplify(self, cell_size, *, origin=None, placement="mean", tol=1e-3) -> "Mesh":
        """Vertex clustering: snap the vertices to a grid of cubic cells of edge ``cell_size`` (world units) whose
        corner is ``origin`` (3 floats; default: the minimum of the vertices), replace every occupied cell by one
        vertex at the mean of its members (normals: the normalised sum, colours: the mean), rewrite the faces, and
        drop the faces that collapsed and the later copies of a face.  Kept faces stay in their order, the surviving
        vertices are ordered by the smallest vertex index of their cell; cells and vertices that no surviving face
        uses are dropped.  A tiny cell welds coincident vertices and removes zero-area triangles.  ``placement``:
        "mean" (the default) or "quadric".  "quadric" moves every cluster's vertex to the point that minimises the
        summed plane quadrics of the original faces that touch the cluster (kernels.mesh_cluster_quadric), solved from
        the mean and only along the directions whose eigenvalue exceeds ``tol`` (in (0, 1)) times the largest: flat
        regions stay in their plane, edges and corners are kept, a convex surface does not shrink; a vertex never
        leaves its cell, and a cluster without a usable solution keeps the mean.  Faces, normals and colours are the
        same for both placements.  Bitwise reproducible.  ValueError on a ``cell_size`` that is not a finite positive
        float, on another ``placement``, on a ``tol`` outside (0, 1), on non-finite vertices, and on a grid of more
        than 2^20 cells along an axis."""
        if placement not in ("mean", "quadric"):
            raise ValueError(f'placement must be "mean" or "quadric", got {placement!r}')
        tol = K._tol_arg(tol)
        with np.errstate(all="ignore"):
            cell = np.float32(cell_size)
            inv = np.float32(1.0) / cell
        if not (np.isfinite(cell) and cell > 0 and np.isfinite(inv) and inv > 0):
            raise ValueError(f"cell_size must be a finite positive float, got {cell_size!r}")
        lo = None if origin is None else np.asarray(K._box3(origin, "origin"), np.float32)
        if lo is not None and not np.isfinite(lo).all():
            raise ValueError(f"origin must be finite, got {origin!r}")
        v, f = self.vertices, self.faces
        if v.shape[0] == 0 or f.shape[0] == 0:
            return Mesh(v.new_empty((0, 3)), f.new_empty((0, 3)),
                        None if self.normals is None else self.normals.new_empty((0, 3)),
                        None if self.colors is None else self.colors.new_empty((0, 3)))
        K.need(v, "vertices")
        K._faces_arg(f, v.shape[0])  # the index range, before anything is launched on these faces
        # one read of the box; a full reduction per column (one along dim 0 of the (V,3) tensor took 1.5 ms at
        # V = 1.3 M, three times the labelling kernels); aminmax propagates a NaN
        mm = [torch.aminmax(v[:, c]) for c in range(3)]
        box = np.asarray(torch.stack([m.min for m in mm] + [m.max for m in mm]).tolist(), np.float32)
        if not np.isfinite(box).all():
            raise ValueError("vertices must be finite")
        if lo is None:
            lo = box[:3]
        with np.errstate(all="ignore"):
            cells = np.floor((box[3:] - lo) * inv)  # fp32, like the kernel's cell index of the largest coordinate
        if not np.isfinite(cells).all() or cells.max() + 1 > 2 ** 20:
            raise ValueError(f"cell_size {cell_size!r} gives more than 2^20 cells along an axis")
        dims = [max(1, int(c) + 1) for c in cells]  # an origin above the vertices: one border cell
        labels = K.mesh_cluster_labels(v, lo.tolist(), cell, dims)
        cv, cn, cc = K.mesh_cluster_reduce(v, labels, lo.tolist(), cell, dims, normals=self.normals, colors=self.colors,
                                           ranges_checked=True)
        faces, keep = K.mesh_cluster_faces(f, labels, ranges_checked=True)
        if placement == "quadric":
            row_off, col = K.mesh_vertex_faces(faces, v.shape[0], ranges_checked=True)
            cv, _ = K.mesh_cluster_quadric(v, f, labels, row_off, col, cv, lo.tolist(), cell, dims, tol=tol,
                                           ranges_checked=True)
        ov, of, out = K.mesh_compact(cv, faces, keep, [a for a in (cn, cc) if a is not None], ranges_checked=True)
        out = iter(out)
        return Mesh(ov, of, None if cn is None else next(out), None if cc is None else next(out))

    # ---- smoothing on the device (kernels.mesh_adjacency / mesh_smooth_pass / mesh_vertex_normals)

    def adjacency(self):
        """(row_off (V+1,) int32, col (E,) int32): row v = col[row_off[v]:row_off[v+1]] lists, ascending and once
        each, the vertices that share a face with v."""
        return K.mesh_adjacency(self.faces, self.vertices.shape[0])

    def boundary_vertices(self) -> torch.Tensor:
        """(V,) bool: the vertices of an edge that exactly one face uses.  A closed surface has none."""
        return K.mesh_adjacency(self.faces, self.vertices.shape[0], boundary=True)[2].to(torch.bool)

    def _face_normals(self, vertices, ranges_checked=False):
        row_off, col = K.mesh_vertex_faces(self.faces, vertices.shape[0], ranges_checked=ranges_checked)
        return K.mesh_vertex_normals(vertices, self.faces, row_off, col, ranges_checked=True)

    def compute_normals(self) -> "Mesh":
        """The mesh with unit vertex normals derived from its faces: the normalised sum of the cross products of the
        faces around a vertex (area-weighted), by the faces' winding, which for an extracted mesh points to lower
        density like every normal here; zeros at a vertex without a face.  Vertices, faces, colours and the texture
        are the same tensors."""
        K._vertices_arg(self.vertices)
        return Mesh(self.vertices, self.faces, self._face_normals(self.vertices), self.colors, self.texture, self.texels)

    def smooth(self, iterations=10, lam=0.5, mu=-0.53, fix_boundary=True, fixed=None) -> "Mesh":
        """Taubin smoothing: ``iterations`` times a Jacobi pass v += lam (mean of the neighbours - v) followed by one
        with ``mu`` < -lam, which undoes the shrinkage of the first; ``mu=None`` gives plain Laplacian smoothing, one
        pass per iteration.  The neighbours are the vertices that share a face (uniform weights); the adjacency is
        built once.  ``fixed``: a (V,) bool or uint8 mask of vertices that do not move; with ``fix_boundary`` the
        vertices of open edges (boundary_vertices) are added to it.  Faces and colours are returned unchanged, the
        vertex count and order too; normals, if the mesh has them, are replaced by those of compute_normals on the
        result.  ``iterations == 0`` returns the mesh's data unchanged.  Bitwise reproducible.  ValueError before any
        launch on ``iterations`` that is no int >= 0, ``lam`` no finite float32 in (0, 1], ``mu`` neither None nor a
        finite float32 below -lam, a ``fixed`` of the wrong shape or dtype, non-finite vertices, 6 F >= 2^31."""
        if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or iterations < 0:
            raise ValueError(f"iterations must be an int >= 0, got {iterations!r}")
        with np.errstate(all="ignore"):
            try:
                lam32 = np.float32(lam)
                mu32 = None if mu is None else np.float32(mu)
            except (TypeError, ValueError):
                raise ValueError(f"lam and mu must be floats, got {lam!r}, {mu!r}") from None
        if not (np.isfinite(lam32) and 0 < lam32 <= 1):
            raise ValueError(f"lam must be a finite float32 in (0, 1], got {lam!r}")
        if mu32 is not None and not (np.isfinite(mu32) and mu32 < -lam32):
            raise ValueError(f"mu must be None or a finite float32 below -lam = {-lam32}, got {mu!r}")
        v, f = self.vertices, self.faces
        V, F = int(v.shape[0]), int(f.shape[0])
        if fixed is not None:
            if (not isinstance(fixed, torch.Tensor) or fixed.dtype not in (torch.bool, torch.uint8)
                    or tuple(fixed.shape) != (V,)):
                raise ValueError(f"fixed must be a ({V},) bool or uint8 tensor")
        if 6 * F >= 2 ** 31:
            raise ValueError(f"6 * F must be below 2^31, got F = {F}")
        if iterations == 0 or V == 0 or F == 0:
            return Mesh(v, f, self.normals, self.colors)
        K._vertices_arg(v)
        K._faces_arg(f, V)  # the index range, before anything is launched on these faces
        if fixed is not None:
            fixed = K.need(fixed.view(torch.uint8) if fixed.dtype == torch.bool else fixed, "fixed", torch.uint8)
        if not bool(torch.isfinite(v).all()):
            raise ValueError("vertices must be finite")
        if fix_boundary:
            row_off, col, boundary = K.mesh_adjacency(f, V, boundary=True, ranges_checked=True)
            fixed = boundary if fixed is None else (fixed != 0).to(torch.uint8) | boundary
        else:
            row_off, col = K.mesh_adjacency(f, V, ranges_checked=True)
        cur, bufs, i = v, [None, None], 0  # two buffers swapped between the passes; the input is never written
        for _ in range(int(iterations)):
            for s in (lam32,) if mu32 is None else (lam32, mu32):
                if bufs[i] is None:
                    bufs[i] = torch.empty_like(v)
                cur = K.mesh_smooth_pass(cur, row_off, col, s, fixed=fixed, out=bufs[i], ranges_checked=True)
                i ^= 1
        normals = None if self.normals is None else self._face_normals(cur, ranges_checked=True)
        return Mesh(cur, f, normals, self.colors)

    # ---- metrics on the device (kernels.mesh_face_areas / mesh_sample_surface, mesh_metrics)

    def face_areas(self) -> torch.Tensor:
        """(F,) float64: the area of every face, computed in double; exactly 0 for a face with a repeated index.
        ValueError on non-finite vertices and out-of-range indices."""
        return K.mesh_face_areas(self.vertices, self.faces)

    def area(self) -> float:
        """The surface area: the float64 torch sum of face_areas()."""
        return float(self.face_areas().sum())

    def sample_surface(self, n, seed=0, normals=None):
        """``n`` points distributed uniformly by area over the faces: (points (n,3) float32, face_idx (n,) int32), and
        with ``normals`` = "face" (the sampled face's unit normal, by its winding) or "vertex" (the barycentric mix of
        the mesh's vertex normals, normalised; the mesh must have normals) also (n,3) float32 unit normals.  Sample i
        depends on (seed, i) and the mesh alone: bitwise reproducible.  Faces of zero area, and faces more than 2^32
        times smaller than the largest, are never chosen.  ValueError before the sampling launch on ``n`` that is no
        int >= 0, a bad ``seed`` or ``normals``, non-finite vertices, out-of-range indices, and a mesh without area."""
        if normals == "vertex" and self.normals is None:
            raise ValueError("normals='vertex' needs a mesh with vertex normals (Mesh.compute_normals)")
        return K.mesh_sample_surface(self.vertices, self.faces, n, seed=seed, normals=normals,
                                     vertex_normals=self.normals if normals == "vertex" else None)

    def distance_to(self, other, n_samples=2 ** 18, seed=0, thresholds=(), normals=False, exact=False) -> dict:
        """mesh_metrics.mesh_distance(self, other, ...): Chamfer, Hausdorff, precision / recall / F-score at
        ``thresholds`` and (``normals``) normal consistency between ``n_samples`` area-uniform samples of each mesh,
        as a dict of floats with self as a and other as b.  The point-set distance: it overestimates the distance
        between the surfaces by up to the sampling spacing, about sqrt(area / n_samples).  ``exact``: measure every
        sample against the other mesh's triangles instead of its samples: no sampling floor."""
        from .mesh_metrics import mesh_distance
        if not isinstance(other, Mesh):
            raise ValueError(f"other must be a Mesh, got {type(other).__name__}")
        return mesh_distance(self, other, n_samples=n_samples, seed=seed, thresholds=thresholds, normals=normals,
                             exact=exact)

    def closest_points(self, query, cell_size=None):
        """mesh_metrics.nearest_on_mesh(query, self, cell_size): for every row of ``query`` (n,3) float32 the squared
        distance in double to the nearest triangle, that face's index (the smallest on equal distance) and the closest
        point on it: (d2 (n,) float64, face (n,) int32, closest (n,3) float32), a brute-force search's result bit for
        bit."""
        from .mesh_metrics import nearest_on_mesh
        return nearest_on_mesh(query, self, cell_size)

    # ---- ray casting on the device (kernels.mesh_ray_cast)

    def ray_cast(self, rays, cell_size=None, cull_backfaces=False, grid=None):
        """mesh_metrics.ray_cast_mesh(rays, self, ...): for every row [o, d, near, far] of ``rays`` (n,8) float32 the
        nearest face the ray o + t d hits with near <= t <= far: (t (n,) float64, +inf on a miss; face (n,) int32, -1 on
        a miss; bary (n,2) float32 = (u, v), the hit point being (1 - u - v) a + u b + v c), the result of testing every
        face, bit for bit.  t is the ray's own parameter: d is not normalised."""
        from .mesh_metrics import ray_cast_mesh
        return ray_cast_mesh(rays, self, cell_size=cell_size, cull_backfaces=cull_backfaces, grid=grid)

    # ---- containment on the device (kernels.mesh_point_crossings)

    def contains(self, points, rule="parity", cell_size=None, grid=None, beta=3.0, exact=False, bricks=None):
        """mesh_metrics.points_in_mesh(points, self, ...): (n,) bool, whether every row of ``points`` (n,3) float32 lies
        inside this mesh, by the parity of the faces the vertical ray from the point crosses (``rule`` = "winding":
        by their winding number).  Exact except within rounding of the surface; meaningful for a closed mesh only,
        unless rule="generalized": winding_number(points, beta, exact, bricks) > 0.5, which answers for open and
        broken meshes too."""
        from .mesh_metrics import points_in_mesh
        return points_in_mesh(points, self, rule=rule, cell_size=cell_size, grid=grid, beta=beta, exact=exact,
                              bricks=bricks)

    def signed_distance(self, points, rule="parity", cell_size=None, grid=None, beta=3.0, exact=False, bricks=None):
        """mesh_metrics.signed_distance_to_mesh(points, self, ...): (sd (n,) float64, face (n,) int32, closest (n,3)
        float32), the distance of closest_points with a negative sign inside; meaningful for a closed mesh only,
        unless rule="generalized" (the sign is then that of winding_number > 0.5)."""
        from .mesh_metrics import signed_distance_to_mesh
        return signed_distance_to_mesh(points, self, rule=rule, cell_size=cell_size, grid=grid, beta=beta, exact=exact,
                                       bricks=bricks)

    def winding_number(self, points, beta=3.0, exact=False, bricks=None):
        """mesh_metrics.winding_number(points, self, ...): (n,) float64, the generalised winding number of every row of
        ``points`` (n,3) float32: the signed solid angles of the faces over 4 pi, 1 inside and 0
        outside a closed mesh wound outwards, a real number that falls smoothly across the holes of an open one.
        ``exact``: every face; otherwise a dipole per brick of faces farther than ``beta`` brick radii.  ``bricks``: a
        kernels.mesh_winding_bricks of this mesh built before.  ON the surface: deterministic, not meaningful."""
        from .mesh_metrics import winding_number
        return winding_number(points, self, beta=beta, exact=exact, bricks=bricks)

    def volume(self) -> float:
        """The signed volume: the float64 torch sum of a . (b x c) / 6 over the faces (the divergence theorem).
        Positive for a closed mesh whose normals point outwards, which is the extractor's convention.  For an open
        mesh it means nothing: the value then depends on where the origin lies.  ValueError on out-of-range indices."""
        K._faces_arg(self.faces, K._vertices_arg(self.vertices))
        if self.faces.shape[0] == 0:
            return 0.0
        p = self.vertices.to(torch.float64)
        f = self.faces.to(torch.int64)
        a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
        return float((a * torch.linalg.cross(b, c)).sum() / 6.0)

    def iou(self, other, n_samples=2 ** 20, seed=0, rule="parity", cell_size=None, beta=3.0, exact=False,
            bricks=None) -> dict:
        """mesh_metrics.volume_iou(self, other, ...): the Monte Carlo volumetric intersection over union of two closed
        meshes (open ones too with rule="generalized") and the volumes it rests on, as a dict with self as a and
        other as b."""
        from .mesh_metrics import volume_iou
        if not isinstance(other, Mesh):
            raise ValueError(f"other must be a Mesh, got {type(other).__name__}")
        return volume_iou(self, other, n_samples=n_samples, seed=seed, rule=rule, cell_size=cell_size, beta=beta,
                          exact=exact, bricks=bricks)

    def render(self, H, W, fx, fy, cx, cy, c2w, near=0.0, far=float("inf"), cull_backfaces=False, grid=None) -> dict:
        """The mesh seen from a pinhole camera, through the rays of ray_sampling.rays_for_camera (pixel centres, the
        camera looking along its -z axis, unit directions): a dict of device tensors,
          depth  (H,W) float32   the hit's t in the ray parameter of render_image's depth, +inf where nothing is hit
          mask   (H,W) bool      a face is hit
          face   (H,W) int32     the face, -1 where nothing is hit
          normal (H,W,3) float32 with vertex normals their barycentric mix, normalised; without them the unit normal of
                                 the face by its winding; zeros where nothing is hit
          color  (H,W,3) float32 only for a mesh with colours: their barycentric mix, zeros where nothing is hit
          texture (H,W,3) float32 only for a textured mesh: sample_texture at the hit, zeros where nothing is hit.
        The cast is Mesh.ray_cast; the gathers and mixes are a few float64 torch ops, rounded to fp32 at the end."""
        from .ray_sampling import rays_for_camera
        H, W = int(H), int(W)
        if H < 1 or W < 1:
            raise ValueError(f"H and W must be positive, got {H}, {W}")
        if not isinstance(c2w, torch.Tensor):
            raise ValueError("c2w must be a (3,4) or (4,4) tensor")
        K._vertices_arg(self.vertices)
        dev = self.vertices.device
        rays = rays_for_camera(H, W, fx, fy, cx, cy, c2w.to(dev), near=float(near), far=float(far))
        t, face, bary = self.ray_cast(rays, cull_backfaces=cull_backfaces, grid=grid)
        hit = face >= 0
        if self.faces.shape[0] == 0:
            out = {"depth": t.to(torch.float32).view(H, W), "mask": hit.view(H, W), "face": face.view(H, W),
                   "normal": torch.zeros((H, W, 3), dtype=torch.float32, device=dev)}
            if self.colors is not None:
                out["color"] = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
            if self.texture is not None:
                out["texture"] = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
            return out
        corners = self.faces[face.clamp(min=0).to(torch.int64)].to(torch.int64)  # (n, 3); face 0 stands in at a miss
        u, v = bary[:, 0].to(torch.float64), bary[:, 1].to(torch.float64)
        weights = torch.stack([(1.0 - u) - v, u, v], 1)  # (n, 3)

        def mix(attr):
            return (attr[corners].to(torch.float64) * weights[:, :, None]).sum(1)

        if self.normals is not None:
            normal = mix(self.normals)
        else:
            p = self.vertices[corners].to(torch.float64)  # (n, 3 corners, 3)
            normal = torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        normal = normal / torch.linalg.norm(normal, dim=1, keepdim=True).clamp_min(1e-300)
        out = {"depth": t.to(torch.float32).view(H, W), "mask": hit.view(H, W), "face": face.view(H, W),
               "normal": (normal * hit[:, None]).to(torch.float32).view(H, W, 3)}
        if self.colors is not None:
            c = self.colors[corners]  # (n, 3 corners, 3): the mix stays between the corners' values per channel
            color = torch.minimum(torch.maximum(mix(self.colors).to(torch.float32), c.amin(1)), c.amax(1))
            out["color"] = (color * hit[:, None]).view(H, W, 3)
        if self.texture is not None:
            out["texture"] = self.sample_texture(face, bary).view(H, W, 3)  # a miss has face -1: zeros
        return out


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


def _refine_crossings(density_fn, record, keys, steps):
    """``steps`` bisection steps of every crossing point along its own lattice edge (torch ops only): the bracket
    starts at the edge's two lattice points (from ``keys`` = 3 p + a), the midpoint replaces the end whose
    ``> threshold`` bit it shares, and the result is the last bracket's midpoint: (E,3) float32, exactly on the edge."""
    field = record.field
    nx, ny, nz = (int(n) for n in field.shape)
    dev = field.device
    lo_t = torch.tensor(record.lo, dtype=torch.float32, device=dev)
    h = (torch.tensor(record.hi, dtype=torch.float32, device=dev) - lo_t) / torch.tensor(
        [nx - 1, ny - 1, nz - 1], dtype=torch.float32, device=dev)
    k = keys.to(torch.int64)
    p, a = torch.div(k, 3, rounding_mode="floor"), k % 3
    r = torch.div(p, nz, rounding_mode="floor")
    idx = torch.stack([torch.div(r, ny, rounding_mode="floor"), r % ny, p % nz], -1)
    rows = torch.arange(k.numel(), device=dev)
    pts = lo_t + idx.to(torch.float32) * h
    A = pts[rows, a]
    B = lo_t[a] + (idx[rows, a] + 1).to(torch.float32) * h[a]
    inside_a = field.reshape(-1)[p] > record.iso
    with torch.no_grad():
        for _ in range(int(steps)):
            mid = 0.5 * (A + B)
            pts[rows, a] = mid
            same = (density_fn(pts).reshape(-1).to(torch.float32) > record.iso) == inside_a
            A, B = torch.where(same, mid, A), torch.where(same, B, mid)
    pts[rows, a] = 0.5 * (A + B)
    return pts


def _extract_dual(density_fn, field, threshold, lo, hi, cell_normals, placement, tol, hermite, refine) -> "Mesh":
    record, points, nrm, keys = K.mesh_dual_hermite(field, threshold, lo, hi, normals=(hermite == "grid"))
    if refine and record.E:
        points = _refine_crossings(density_fn, record, keys, refine)
    if callable(hermite):
        nrm = hermite(points) if record.E else torch.empty_like(points)
        if not isinstance(nrm, torch.Tensor) or tuple(nrm.shape) != tuple(points.shape):
            raise ValueError(f"hermite must return a tensor {tuple(points.shape)}")
        nrm = nrm.detach().to(torch.float32).contiguous()
    return Mesh(*K.mesh_dual_vertices(record, points, nrm, placement=placement, tol=tol, vertex_normals=cell_normals))


def extract_mesh(density_fn: Callable, lo, hi, resolution: Union[int, Sequence[int]], threshold: float,
                 normals: Union[str, None, Callable] = "grid", chunk: int = 2 ** 20, device=None,
                 min_faces: Optional[int] = None, keep_largest: Optional[int] = None,
                 simplify: Optional[float] = None, smooth: Optional[int] = None,
                 simplify_placement: str = "mean", method: str = "tets", placement: str = "qef", tol: float = 1e-3,
                 hermite: Union[str, Callable] = "grid", refine: int = 0) -> Mesh:
    """The level set density_fn = threshold inside the box [lo, hi] as a Mesh on the device.  normals: "grid" (the
    lattice's central differences, from the extraction kernel), None, or a callable evaluated at the vertices
    ((V,3) -> (V,3)).  min_faces / keep_largest (at most one): Mesh.filter_components on the extracted surface, before
    a callable ``normals`` is evaluated, so that it runs on the surviving vertices only.  simplify: a cell size in
    world units for Mesh.simplify, applied after the component filter and also before a callable ``normals``; "grid"
    normals are averaged per cell by the clustering kernel.  simplify_placement: "mean" or "quadric", the ``placement``
    of Mesh.simplify (quadric-error vertices keep edges, corners and volume; faces and attributes are the same).
    smooth: a number of Taubin iterations for Mesh.smooth with its defaults, applied after ``simplify`` and also before a callable ``normals``; "grid" normals are then replaced
    by the face-derived normals of the smoothed mesh (Mesh.compute_normals).  None returns the surface unsmoothed.

    method: "tets" (marching tetrahedra, kernels.mesh_extract: vertices on lattice edges, 2-3 times the triangles of
    marching cubes) or "dual" (dual contouring, kernels.mesh_dual_hermite / mesh_dual_vertices, DESIGN §3.11.11: one
    vertex per sign-changing cell and one quad per sign-changing lattice edge, about a third of the triangles, and
    vertices that can sit on creases and corners of the level set).  The other options below are "dual"'s.
    placement: "qef" (the vertex minimises the plane quadric of the cell's crossing points and normals; ``tol`` in
    (0, 1) truncates its small eigenvalues as Mesh.simplify's does) or "mean" (surface nets).  hermite: "grid" (normals
    of the lattice's central differences) or a callable (E,3) crossing points -> (E,3) normals, for a field that knows
    its own gradient.  refine: bisection steps of every crossing point along its own lattice edge, each one call of
    density_fn on (E,3) points, before a callable ``hermite`` is evaluated.  normals="grid" gives the normalised sum of
    each cell's edge normals.  Every later option works on the result unchanged.  A cell that two sheets of the level
    set cross still gets one vertex, so a noisy field can give edges shared by more than two triangles; the surface
    is open at the box, as marching tetrahedra's is."""
    if not (normals is None or normals == "grid" or callable(normals)):
        raise ValueError(f"normals must be 'grid', None or a callable, got {normals!r}")
    if smooth is not None and (isinstance(smooth, bool) or not isinstance(smooth, (int, np.integer)) or smooth < 0):
        raise ValueError(f"smooth must be None or an int >= 0, got {smooth!r}")
    if min_faces is not None and keep_largest is not None:
        raise ValueError("give at most one of min_faces and keep_largest")
    if simplify_placement not in ("mean", "quadric"):
        raise ValueError(f'simplify_placement must be "mean" or "quadric", got {simplify_placement!r}')
    if method not in ("tets", "dual"):
        raise ValueError(f'method must be "tets" or "dual", got {method!r}')
    if placement not in ("qef", "mean"):
        raise ValueError(f'placement must be "qef" or "mean", got {placement!r}')
    if not 0.0 < float(tol) < 1.0:
        raise ValueError(f"tol must be in (0, 1), got {tol!r}")
    if not (hermite == "grid" or callable(hermite)):
        raise ValueError(f"hermite must be 'grid' or a callable, got {hermite!r}")
    if isinstance(refine, bool) or not isinstance(refine, (int, np.integer)) or refine < 0:
        raise ValueError(f"refine must be an int >= 0, got {refine!r}")
    if method == "tets" and (callable(hermite) or refine):
        raise ValueError('hermite and refine belong to method="dual"')
    lo, hi = _box(lo, hi)
    field = density_lattice(density_fn, lo, hi, resolution, chunk=chunk, device=device)
    if method == "dual":
        mesh = _extract_dual(density_fn, field, threshold, lo, hi, normals == "grid", placement, tol, hermite, refine)
    else:
        mesh = Mesh(*K.mesh_extract(field, threshold, lo, hi, normals=(normals == "grid")))
    if min_faces is not None or keep_largest is not None:
        mesh = mesh.filter_components(min_faces=min_faces, keep_largest=keep_largest)
    if simplify is not None:
        mesh = mesh.simplify(simplify, placement=simplify_placement)
    if smooth is not None:
        mesh = mesh.smooth(smooth)
    if callable(normals):
        mesh.normals = normals(mesh.vertices) if mesh.vertices.shape[0] else torch.empty_like(mesh.vertices)
    return mesh
