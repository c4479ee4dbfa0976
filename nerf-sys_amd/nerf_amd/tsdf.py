"""TSDF fusion: depth views fused into a truncated signed distance volume on the device (kernels.tsdf_integrate,
csrc/tsdf.hip), and its zero level as a Mesh.

The surface a set of cameras saw, not a level set of the density: depth images (ray_rendering.render_image's depth over
acc, or Mesh.render's depth) are fused view by view; the zero level of the fused field is meshed by
kernels.mesh_extract, and the triangles of cells that no view fully observed are dropped (kernels.tsdf_face_observed),
which removes the sheet at -trunc behind every surface and everything the cameras never looked at.

With color=True the volume also fuses the colour of the pixel each depth came from (kernels.tsdf_integrate_color,
DESIGN §3.11.9), and extract_mesh(colors="fused") samples it at the final vertices (kernels.tsdf_sample_color): vertex
colours for any source of views, with no model to query.  bake_texture fills a mesh's texture atlas from the same
volume (Mesh.bake_texture), and extract_mesh(texture=TEXELS) does so as its last step.
"""
from __future__ import annotations

from typing import Optional, Sequence, Union

import numpy as np
import torch

from . import kernels as K
from .mesh import Mesh, _box, _resolution

__all__ = ["TSDFVolume"]


class TSDFVolume:
    """tsdf and weight (nx,ny,nz) float32 on the device over the lattice lo + (ix,iy,iz) spacing,
    spacing = (hi - lo) / (n - 1) in fp32 (mesh_extract's lattice).  A fresh volume holds tsdf = 1 (free space) and
    weight = 0; weight counts the views that updated a voxel.  trunc: the truncation distance in world units, default
    3 x the largest axis spacing.  color=True adds .color (nx,ny,nz,4) float32: the fused r, g, b and a colour weight
    per voxel, zeros in a fresh volume; it is None otherwise."""

    def __init__(self, lo, hi, resolution: Union[int, Sequence[int]], trunc: Optional[float] = None, device=None,
                 color: bool = False):
        self.lo, self.hi = _box(lo, hi)
        self.resolution = _resolution(resolution)
        if self.resolution[0] * self.resolution[1] * self.resolution[2] >= 2 ** 31:
            raise ValueError(f"lattice too large: {self.resolution} reaches 2^31 points")
        lo32, hi32 = np.asarray(self.lo, np.float32), np.asarray(self.hi, np.float32)
        self.spacing = tuple(float((hi32[a] - lo32[a]) / np.float32(self.resolution[a] - 1)) for a in range(3))
        if trunc is None:
            trunc = float(np.float32(3.0) * np.float32(max(self.spacing)))
        self.trunc = K._f32_arg(trunc, "trunc", True)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.tsdf = torch.empty(self.resolution, dtype=torch.float32, device=self.device)
        self.weight = torch.empty(self.resolution, dtype=torch.float32, device=self.device)
        self.color = torch.empty(self.resolution + (4,), dtype=torch.float32, device=self.device) if color else None
        self.reset()

    def __repr__(self):
        return f"TSDFVolume(resolution={self.resolution}, trunc={self.trunc:.6g}, device={self.device})"

    def reset(self) -> None:
        self.tsdf.fill_(1.0)
        self.weight.zero_()
        if self.color is not None:
            self.color.zero_()

    def integrate(self, depth, fx, fy, cx, cy, c2w, rgb=None) -> None:
        """Fuse depth (n,H,W) or (H,W) seen from c2w (n,3,4), (n,4,4), (3,4) or (4,4) in one call
        (kernels.tsdf_integrate): ranges along unit ray directions; +inf, NaN, 0 and negative values see nothing.
        rgb (n,H,W,3) or (H,W,3), on a volume with colour only: the views' colours, fused with the depth
        (kernels.tsdf_integrate_color; tsdf and weight are the same bits either way).  Without rgb a volume with colour
        fuses the depth alone and leaves .color as it is."""
        if not isinstance(depth, torch.Tensor) or not isinstance(c2w, torch.Tensor):
            raise ValueError("depth and c2w must be tensors")
        if rgb is None:
            K.tsdf_integrate(self.tsdf, self.weight, self.lo, self.hi, depth, c2w, fx, fy, cx, cy, self.trunc)
            return
        if self.color is None:
            raise ValueError("rgb needs a volume with colour: TSDFVolume(..., color=True)")
        if not isinstance(rgb, torch.Tensor):
            raise ValueError("rgb must be a tensor")
        K.tsdf_integrate_color(self.tsdf, self.weight, self.color, self.lo, self.hi, depth, rgb, c2w, fx, fy, cx, cy,
                               self.trunc)

    def sample_colors(self, points, fill: float = 0.5):
        """The fused colour at points (N,3) -> rgb (N,3) float32 and seen (N,) bool (kernels.tsdf_sample_color): seen
        where at least one corner of the point's cell was coloured (cover > 0); rgb is ``fill`` elsewhere."""
        if self.color is None:
            raise ValueError("sample_colors needs a volume with colour: TSDFVolume(..., color=True)")
        rgb, cover = K.tsdf_sample_color(self.color, self.lo, self.hi, points)
        seen = cover > 0
        return torch.where(seen[:, None], rgb, torch.full_like(rgb, float(fill))), seen

    def extract_mesh(self, min_weight=1, normals: Optional[str] = "grid", min_faces: Optional[int] = None,
                     keep_largest: Optional[int] = None, simplify: Optional[float] = None,
                     smooth: Optional[int] = None, colors: Optional[str] = None,
                     simplify_placement: str = "mean", method: str = "tets", texture: Optional[int] = None) -> Mesh:
        """The zero level of the fused field as a Mesh: mesh_extract(-tsdf, 0) (inside is tsdf < 0, normals point to
        larger tsdf: outwards), then only the faces of cells whose 8 corners all have weight >= min_weight
        (min_weight = 0 keeps every face, the sheet at -trunc behind the surface included), then the options of
        mesh.extract_mesh in its order: min_faces / keep_largest (at most one), simplify, smooth.  colors: None, or
        "fused" on a volume with colour: sample_colors at the final vertices, after the filters, simplify and smooth,
        as Mesh.colors (0.5 where no view coloured a corner of the vertex's cell).  simplify_placement: "mean" or
        "quadric", the ``placement`` of Mesh.simplify.  method: "tets" only; the observed-face filter maps a face to
        the one cell that emitted it, and a quad of dual contouring spans four.  texture: None, or on a volume with
        colour the side in texels of an atlas cell: bake_texture on the final mesh, as the last step."""
        if method != "tets":
            raise ValueError(f'TSDFVolume.extract_mesh supports method="tets" only, got {method!r}: its observed-face '
                             "filter needs one cell per face, and a dual-contouring quad spans four cells")
        if simplify_placement not in ("mean", "quadric"):
            raise ValueError(f'simplify_placement must be "mean" or "quadric", got {simplify_placement!r}')
        if normals not in ("grid", None):
            raise ValueError(f"normals must be 'grid' or None, got {normals!r}")
        if colors not in ("fused", None):
            raise ValueError(f"colors must be 'fused' or None, got {colors!r}")
        if colors == "fused" and self.color is None:
            raise ValueError("colors='fused' needs a volume with colour: TSDFVolume(..., color=True)")
        if texture is not None:
            if self.color is None:
                raise ValueError("texture needs a volume with colour: TSDFVolume(..., color=True)")
            K.atlas_layout(0, texture)  # a bad side fails before the extraction
        if smooth is not None and (isinstance(smooth, bool) or not isinstance(smooth, (int, np.integer)) or smooth < 0):
            raise ValueError(f"smooth must be None or an int >= 0, got {smooth!r}")
        if min_faces is not None and keep_largest is not None:
            raise ValueError("give at most one of min_faces and keep_largest")
        *parts, face_off = K.mesh_extract(-self.tsdf, 0.0, self.lo, self.hi, normals=(normals == "grid"),
                                          face_offsets=True)
        mesh = Mesh(*parts)
        if float(min_weight) > 0.0:
            mesh = mesh.select_faces(K.tsdf_face_observed(face_off, self.weight, min_weight))
        if min_faces is not None or keep_largest is not None:
            mesh = mesh.filter_components(min_faces=min_faces, keep_largest=keep_largest)
        if simplify is not None:
            mesh = mesh.simplify(simplify, placement=simplify_placement)
        if smooth is not None:
            mesh = mesh.smooth(smooth)
        if colors == "fused":
            mesh.colors = self.sample_colors(mesh.vertices)[0]
        if texture is not None:
            self.bake_texture(mesh, texture)
        return mesh

    def bake_texture(self, mesh: Mesh, texels: int = 8, fill: float = 0.5) -> Mesh:
        """Fill ``mesh``'s texture atlas (Mesh.bake_texture, cells of ``texels`` x ``texels`` texels) with the fused
        colour: sample_colors at the surface point of every owned texel, ``fill`` where no view coloured a corner of
        the point's cell.  The colours the cameras saw, for any source of views.  Returns the mesh."""
        if self.color is None:
            raise ValueError("bake_texture needs a volume with colour: TSDFVolume(..., color=True)")
        if not isinstance(mesh, Mesh):
            raise ValueError(f"mesh must be a Mesh, got {type(mesh).__name__}")
        return mesh.bake_texture(lambda p, n: self.sample_colors(p, fill)[0], texels, normals=False)
