"""nerf_amd — MI355X (gfx950) NeRF hot path behind the reference's render_rays / expert API.

Host side in Python/PyTorch-ROCm (device memory, streams, torch.distributed); every compute stage is a
hand-written HIP kernel in libnerf_amd.so reached through the C-ABI of include/nerf_amd.h.
"""
from ._lib import LIB_PATH, lib  # noqa: F401
from .mesh import Mesh, density_lattice, extract_mesh  # noqa: F401
from .mesh_metrics import (mesh_distance, nearest_on_mesh, nearest_points, point_set_metrics,  # noqa: F401
                           points_in_mesh, ray_cast_mesh, signed_distance_to_mesh, volume_iou, winding_number)
from .tsdf import TSDFVolume  # noqa: F401

__all__ = ["LIB_PATH", "lib", "Mesh", "density_lattice", "extract_mesh", "mesh_distance", "nearest_on_mesh",
           "nearest_points", "point_set_metrics", "ray_cast_mesh", "points_in_mesh", "signed_distance_to_mesh",
           "volume_iou", "winding_number", "TSDFVolume"]
