"""Mesh metrics on the device: how far one surface is from another.

Both surfaces are sampled uniformly by area (kernels.mesh_sample_surface) and every sample finds its nearest
neighbour in the other set, exactly, through a uniform grid (kernels.points_grid / points_nearest,
csrc/mesh_metrics.hip).  From the two distance arrays come Chamfer, Hausdorff, precision / recall / F-score at given
thresholds and, with normals, the normal consistency.  The kernels are bitwise reproducible and the reductions are a
few float64 torch ops, so equal inputs give equal dicts.

This is the POINT-SET distance.  The distance from a sample to the nearest SAMPLE of the other surface overestimates
its distance to that surface by up to the sampling spacing (about sqrt(area / n_samples)), so two identical meshes
sampled with different seeds give a small non-zero Chamfer; with the same seed they give exactly 0.

The EXACT path (csrc/mesh_distance.hip) removes that floor: nearest_on_mesh returns, for every query,
the squared distance in double to the nearest TRIANGLE, that face and the closest point on it, through a uniform grid
of the faces (kernels.mesh_face_grid / mesh_nearest_faces), and mesh_distance(..., exact=True) measures the samples of
each mesh against the surface of the other.

RAY CASTING (csrc/mesh_raycast.hip) is the second query over that face grid: ray_cast_mesh returns,
for every ray, the nearest face it hits, the ray's parameter there and the barycentric coordinates of the hit.
"""
from __future__ import annotations

import math

import torch

from . import kernels as K

__all__ = ["nearest_points", "nearest_on_mesh", "ray_cast_mesh", "point_set_metrics", "mesh_distance"]

DEFAULT_SAMPLES = 2 ** 18


def nearest_points(query, ref, cell_size=None):
    """(d2 (n,) float32, idx (n,) int32): for every row of ``query`` (n,3) the squared distance, in fp32 as
    (dx dx + dy dy) + dz dz, to the nearest row of ``ref`` (m,3) and that row's index, the smallest on equal distance:
    a brute-force search's result, bit for bit.  An empty ``ref`` gives +inf and -1.  ``cell_size``: the edge of the
    search grid's cells (default: kernels.points_grid's rule).  ValueError before any launch on CPU tensors, wrong
    dtypes or shapes, non-finite points, and a cell_size that is not finite and positive or that needs more than 1024
    cells along an axis."""
    K._finite_points(query, "query")
    return K.points_nearest(query, K.points_grid(ref, cell_size), finite_checked=True)


def _thresholds(thresholds):
    try:
        taus = [float(t) for t in thresholds]
    except TypeError:
        raise ValueError(f"thresholds must be a sequence of floats, got {thresholds!r}") from None
    if any(not (math.isfinite(t) and t >= 0) for t in taus):
        raise ValueError(f"thresholds must be finite and >= 0, got {thresholds!r}")
    return taus


def _side(d2):
    """(mean, rms, max, mean of d2, d) of one direction, 0-dim float64 tensors; an empty direction gives NaNs."""
    d2 = d2.to(torch.float64)
    d = torch.sqrt(d2)
    if d.numel() == 0:
        nan = torch.full((), float("nan"), dtype=torch.float64, device=d.device)
        return nan, nan, nan, nan, d
    mean2 = d2.mean()
    return d.mean(), torch.sqrt(mean2), d.max(), mean2, d


def point_set_metrics(a, b, thresholds=(), normals_a=None, normals_b=None, cell_size=None):
    """The metrics between two point sets a (n,3) and b (m,3), float32 device tensors, as a dict of Python floats.
    With d_ab = sqrt(float64(d2)) from every point of a to its nearest point of b, and d_ba the other way:

      a_to_b_mean, a_to_b_rms, a_to_b_max, b_to_a_mean, b_to_a_rms, b_to_a_max
      chamfer = (a_to_b_mean + b_to_a_mean) / 2          chamfer_sq = mean d2_ab + mean d2_ba
      hausdorff = max(a_to_b_max, b_to_a_max)
      precision@tau = share of d_ab <= tau, recall@tau = share of d_ba <= tau, fscore@tau = 2PR / (P + R) (0 when
      P + R == 0), for every tau of ``thresholds`` (the key is f"precision@{tau}" of the float)
      normal_consistency (with normals_a (n,3) and normals_b (m,3)): the mean of the mean of |n_a . n_b[idx_ab]| and
      of the mean of |n_b . n_a[idx_ba]|

    The reductions are float64 torch ops.  This is the point-set distance (see the module's docstring).  Both sets
    must be non-empty.  ValueError before any launch on bad arguments (as nearest_points)."""
    n, m = K._points_arg(a, "a"), K._points_arg(b, "b")
    if n == 0 or m == 0:
        raise ValueError("both point sets must be non-empty")
    taus = _thresholds(thresholds)
    if (normals_a is None) != (normals_b is None):
        raise ValueError("give both normals_a and normals_b or neither")
    for t, name, rows in ((normals_a, "normals_a", n), (normals_b, "normals_b", m)):
        if t is not None:
            K.need(t, name)
            if tuple(t.shape) != (rows, 3):
                raise ValueError(f"{name} must be ({rows},3), got {tuple(t.shape)}")
    K._finite_points(a, "a")  # b's check is the box read of its grid, before that grid's first launch
    grid_b = K.points_grid(b, cell_size)
    grid_a = K.points_grid(a, cell_size)
    d2_ab, idx_ab = K.points_nearest(a, grid_b, finite_checked=True)
    d2_ba, idx_ba = K.points_nearest(b, grid_a, finite_checked=True)
    cosines = None
    if normals_a is not None:
        na, nb = normals_a.to(torch.float64), normals_b.to(torch.float64)
        cosines = (na * nb[idx_ab.to(torch.int64)]).sum(1), (nb * na[idx_ba.to(torch.int64)]).sum(1)
    return _report(d2_ab, d2_ba, taus, cosines)


def _report(d2_ab, d2_ba, taus, cosines=None):
    """The dict of point_set_metrics from the two arrays of squared distances (fp32 or float64) and, for
    normal_consistency, the two arrays of cosines between every item's normal and its nearest neighbour's."""
    n, m = d2_ab.shape[0], d2_ba.shape[0]
    ab, ba = _side(d2_ab), _side(d2_ba)
    names = ["a_to_b_mean", "a_to_b_rms", "a_to_b_max", "b_to_a_mean", "b_to_a_rms", "b_to_a_max", "chamfer",
             "chamfer_sq", "hausdorff"]
    vals = [ab[0], ab[1], ab[2], ba[0], ba[1], ba[2], (ab[0] + ba[0]) / 2, ab[3] + ba[3], torch.maximum(ab[2], ba[2])]
    for tau in taus:
        p = (ab[4] <= tau).sum().to(torch.float64) / n
        r = (ba[4] <= tau).sum().to(torch.float64) / m
        f = torch.where(p + r > 0, 2 * p * r / torch.clamp(p + r, min=1e-300), torch.zeros_like(p))
        names += [f"precision@{tau}", f"recall@{tau}", f"fscore@{tau}"]
        vals += [p, r, f]
    if cosines is not None:
        c_ab = cosines[0].abs().mean()
        c_ba = cosines[1].abs().mean()
        names.append("normal_consistency")
        vals.append((c_ab + c_ba) / 2)
    return dict(zip(names, torch.stack(vals).tolist()))  # one host read


def nearest_on_mesh(query, mesh, cell_size=None):
    """(d2 (n,) float64, face (n,) int32, closest (n,3) float32): for every row of ``query`` (n,3) the squared
    distance, in double, to the nearest triangle of ``mesh`` (a Mesh on the device), that face's index, the smallest
    on equal distance, and the closest point on it rounded to fp32: a brute-force search's result over all faces,
    bit for bit (kernels.mesh_nearest_faces).  A face without area counts as its three edges.  A mesh
    without faces gives +inf, -1 and the query itself.  ``cell_size``: the edge of the search grid's cells (default:
    kernels.mesh_face_grid's rule).  ValueError before any launch on CPU tensors, wrong dtypes or shapes, non-finite
    queries or vertices, out-of-range indices, a cell_size that is not finite and positive or that needs more than
    1024 cells along an axis, and before the key launch on a grid of 2^31 keys or more."""
    K._finite_points(query, "query")
    grid = K.mesh_face_grid(mesh.vertices, mesh.faces, cell_size)
    return K.mesh_nearest_faces(query, mesh.vertices, mesh.faces, grid, finite_checked=True)


def ray_cast_mesh(rays, mesh, cell_size=None, cull_backfaces=False, grid=None):
    """(t (n,) float64, face (n,) int32, bary (n,2) float32): for every row [o, d, near, far] of ``rays`` (n,8)
    float32 the nearest face of ``mesh`` (a Mesh on the device) that the ray o + t d hits with near <= t <= far: t in
    the ray's own parameter (d is not normalised), +inf on a miss; the face, the smallest index on equal t, -1 on a
    miss; (u, v) with the hit point (1 - u - v) a + u b + v c, zeros on a miss; the result of testing every face, bit
    for bit (kernels.mesh_ray_cast).  ``cull_backfaces``: only faces whose winding normal points
    against the ray.  ``grid``: a kernels.mesh_face_grid of this mesh built before, to cast many ray sets through one
    grid (``cell_size`` is then ignored); default: built here with ``cell_size``.  ValueError before any launch as
    kernels.mesh_face_grid and kernels.mesh_ray_cast state."""
    if grid is not None:
        return K.mesh_ray_cast(rays, mesh.vertices, mesh.faces, grid, cull_backfaces)
    K._rays_arg(rays)
    grid = K.mesh_face_grid(mesh.vertices, mesh.faces, cell_size)  # it checks the mesh
    return K.mesh_ray_cast(rays, mesh.vertices, mesh.faces, grid, cull_backfaces, finite_checked=True)


def _unit_face_normals(mesh):
    """(F,3) float64: nerf_mm::face_cross of every face in float64 torch ops, divided by its length; zeros for a zero
    cross product."""
    p = mesh.vertices.to(torch.float64)
    f = mesh.faces.to(torch.int64)
    o = p[f[:, 0]]
    a, b = p[f[:, 1]] - o, p[f[:, 2]] - o
    c = torch.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    d = torch.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
    return c / torch.where(d > 0, d, torch.ones_like(d))[:, None]


def mesh_distance(mesh_a, mesh_b, n_samples=DEFAULT_SAMPLES, seed=0, thresholds=(), normals=False, cell_size=None,
                  exact=False):
    """point_set_metrics between ``n_samples`` area-uniform samples of each of two meshes (Mesh.sample_surface with the
    same ``seed`` on both, so a mesh against itself gives exactly 0).  ``normals``: add normal_consistency from the
    faces' own normals.  The point-set distance: sample-to-sample distance overestimates sample-to-surface distance by
    up to the sampling spacing, about sqrt(area / n_samples).  ValueError before any launch on bad arguments, on
    n_samples < 1, and on a mesh without a face of positive area.

    ``exact``: measure the samples of a against the SURFACE of b and the samples of b against the surface of a
    (nearest_on_mesh, float64 squared distances); the same keys with the same definitions, normal_consistency from the
    sample's face normal against the unit normal of the nearest face (0 for a face whose cross product is zero), and
    ``cell_size`` the cell of the two face grids.  No sampling floor: a mesh against itself gives distances of the
    order of the fp32 rounding of the samples, whatever the seeds."""
    K._count_arg(n_samples, "n_samples")
    if n_samples < 1:
        raise ValueError(f"n_samples must be >= 1, got {n_samples!r}")
    taus = _thresholds(thresholds)
    kind = "face" if normals else None
    sa = mesh_a.sample_surface(n_samples, seed=seed, normals=kind)
    sb = mesh_b.sample_surface(n_samples, seed=seed, normals=kind)
    if not exact:
        return point_set_metrics(sa[0], sb[0], thresholds, sa[2] if normals else None, sb[2] if normals else None,
                                 cell_size=cell_size)
    # the samples are finite (finite vertices) and sample_surface has checked both meshes
    grid_b = K.mesh_face_grid(mesh_b.vertices, mesh_b.faces, cell_size)
    grid_a = K.mesh_face_grid(mesh_a.vertices, mesh_a.faces, cell_size)
    d2_ab, face_ab = K.mesh_nearest_faces(sa[0], mesh_b.vertices, mesh_b.faces, grid_b, closest=False,
                                          finite_checked=True)
    d2_ba, face_ba = K.mesh_nearest_faces(sb[0], mesh_a.vertices, mesh_a.faces, grid_a, closest=False,
                                          finite_checked=True)
    cosines = None
    if normals:
        na, nb = sa[2].to(torch.float64), sb[2].to(torch.float64)
        cosines = ((na * _unit_face_normals(mesh_b)[face_ab.to(torch.int64)]).sum(1),
                   (nb * _unit_face_normals(mesh_a)[face_ba.to(torch.int64)]).sum(1))
    return _report(d2_ab, d2_ba, taus, cosines)
