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

CONTAINMENT (csrc/mesh_inside.hip) is the third: points_in_mesh counts the faces the vertical ray from
a query crosses, with an exact in-projection test, and from it come signed_distance_to_mesh (the sign for
nearest_on_mesh's magnitude) and volume_iou (Monte Carlo over kernels.box_points).  All three mean something for a
closed mesh only, unless rule="generalized".

THE GENERALISED WINDING NUMBER (csrc/mesh_winding.hip) answers for open and broken meshes too:
winding_number sums the signed solid angles of the faces seen from a query, exactly or with a dipole per far brick of
faces; rule="generalized" makes "inside" w > 0.5 in all three.
"""
from __future__ import annotations

import math

import torch

from . import kernels as K

__all__ = ["nearest_points", "nearest_on_mesh", "ray_cast_mesh", "point_set_metrics", "mesh_distance",
           "points_in_mesh", "signed_distance_to_mesh", "volume_iou", "winding_number"]

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


def _rule_arg(rule):
    if rule not in ("parity", "winding", "generalized"):
        raise ValueError(f"rule must be 'parity', 'winding' or 'generalized', got {rule!r}")
    return rule


def winding_number(query, mesh, beta=3.0, exact=False, bricks=None):
    """(n,) float64: the generalised winding number of every row of ``query`` (n,3) float32 with respect to ``mesh`` (a
    Mesh on the device): the sum of the signed solid angles of its faces over 4 pi (kernels.mesh_winding_number,
    DESIGN §3.11.10).  1 inside and 0 outside a closed mesh whose normals point outwards; on an open or broken mesh a
    real number that falls smoothly across the holes, "inside" being w > 0.5.  ``exact``: every face by its solid
    angle; otherwise the bricks of faces farther than ``beta`` brick radii contribute a dipole each (the error falls
    as beta grows).  ``bricks``: a kernels.mesh_winding_bricks of this mesh built before; default: built here.  ON the
    surface the value is deterministic and not meaningful.  A mesh without faces gives zeros.  ValueError before any
    launch as kernels.mesh_winding_bricks and kernels.mesh_winding_number state."""
    K._beta_arg(beta)
    if bricks is not None:
        return K.mesh_winding_number(query, mesh.vertices, mesh.faces, bricks, beta=beta, exact=exact)
    K._finite_points(query, "query")
    bricks = K.mesh_winding_bricks(mesh.vertices, mesh.faces)  # it checks the mesh
    return K.mesh_winding_number(query, mesh.vertices, mesh.faces, bricks, beta=beta, exact=exact, finite_checked=True)


def _generalized_args(rule, beta, exact, bricks):
    """beta, exact and bricks go with rule="generalized" alone: ValueError when one is set under another rule"""
    _rule_arg(rule)
    K._beta_arg(beta)
    if rule != "generalized" and (beta != 3.0 or exact or bricks is not None):
        raise ValueError("beta, exact and bricks go with rule='generalized' only")


def _inside(crossings, winding, rule):
    return (crossings & 1).to(torch.bool) if rule == "parity" else winding != 0


def points_in_mesh(query, mesh, rule="parity", cell_size=None, grid=None, beta=3.0, exact=False, bricks=None):
    """(n,) bool: whether every row of ``query`` (n,3) float32 lies inside ``mesh`` (a Mesh on the device), from the
    faces the vertical ray from the query crosses (kernels.mesh_point_crossings).  ``rule``: "parity",
    an odd number of crossings, or "winding", a non-zero sum of the crossed faces' orientations (it tells a doubly
    covered region from an empty one; for a closed mesh without self-intersections both agree).  The answer means
    something for a CLOSED mesh only, unless rule="generalized"; an extracted surface is open where it meets its box.
    rule="generalized": winding_number(query, mesh, beta, exact, bricks) > 0.5, which also answers for an open or
    broken mesh; it uses no face grid, so a ``grid`` given with it is a ValueError, and ``beta``, ``exact`` and
    ``bricks`` go with this rule alone.  Exact except within rounding of the surface itself.  ``grid``: a
    kernels.mesh_face_grid of this mesh built before (``cell_size`` is then
    ignored); default: built here with ``cell_size``.  A mesh without faces contains nothing.  ValueError before any
    launch on a bad rule and as kernels.mesh_face_grid and kernels.mesh_point_crossings state."""
    _generalized_args(rule, beta, exact, bricks)
    if rule == "generalized":
        if grid is not None:
            raise ValueError("rule='generalized' does not use a face grid: pass bricks, not grid")
        return winding_number(query, mesh, beta=beta, exact=exact, bricks=bricks) > 0.5
    if grid is not None:
        return _inside(*K.mesh_point_crossings(query, mesh.vertices, mesh.faces, grid), rule)
    K._finite_points(query, "query")
    grid = K.mesh_face_grid(mesh.vertices, mesh.faces, cell_size)  # it checks the mesh
    return _inside(*K.mesh_point_crossings(query, mesh.vertices, mesh.faces, grid, finite_checked=True), rule)


def signed_distance_to_mesh(query, mesh, rule="parity", cell_size=None, grid=None, beta=3.0, exact=False,
                            bricks=None):
    """(sd (n,) float64, face (n,) int32, closest (n,3) float32): nearest_on_mesh's face and closest point, and the
    distance sqrt(d2) with the sign of points_in_mesh: negative inside, positive outside, +0.0 where d2 == 0.  One face
    grid serves both queries (``grid``: one built before; ``cell_size`` is then ignored).  The sign is that of a
    CLOSED mesh (see points_in_mesh), unless rule="generalized": the distance still comes through the face grid, the
    sign from winding_number(query, mesh, beta, exact, bricks) > 0.5.  No pseudo-normals are involved.  A mesh without
    faces gives +inf, -1 and the query itself.  ValueError before any launch as points_in_mesh."""
    _generalized_args(rule, beta, exact, bricks)
    checked = grid is None
    if checked:
        K._finite_points(query, "query")
        grid = K.mesh_face_grid(mesh.vertices, mesh.faces, cell_size)  # it checks the mesh
    if rule == "generalized" and bricks is not None:  # before the first query launch
        K._winding_bricks_arg(bricks, int(mesh.faces.shape[0]))
    d2, face, closest = K.mesh_nearest_faces(query, mesh.vertices, mesh.faces, grid, finite_checked=checked)
    if rule == "generalized":
        if bricks is None:
            bricks = K.mesh_winding_bricks(mesh.vertices, mesh.faces)
        inside = K.mesh_winding_number(query, mesh.vertices, mesh.faces, bricks, beta=beta, exact=exact,
                                       finite_checked=True) > 0.5
    else:
        inside = _inside(*K.mesh_point_crossings(query, mesh.vertices, mesh.faces, grid, finite_checked=True), rule)
    d = torch.sqrt(d2)
    return torch.where(inside & (d2 > 0), -d, d), face, closest


def volume_iou(mesh_a, mesh_b, n_samples=2 ** 20, seed=0, rule="parity", cell_size=None, beta=3.0, exact=False,
               bricks=None):
    """The volumetric intersection over union of two CLOSED meshes (unless rule="generalized") by Monte Carlo:
    ``n_samples`` kernels.box_points of
    the common box of both meshes' vertices, each tested with points_in_mesh against either mesh.  Returns a dict:
    iou = intersection / union (0.0 when the union is empty); volume_a, volume_b, intersection, union = the count
    times box volume / n_samples; count_a, count_b, count_intersection, count_union the four raw counts; n_samples; box
    = (lo, hi), the fp32 corners as lists.  The standard error of a volume is box volume sqrt(p (1 - p) / n_samples)
    for its share p.  Equal arguments give equal dicts (the points and the counts are bitwise reproducible).  Host
    reads: the checks of both meshes, the two grids', the box, and one for the four counts.  rule="generalized": a
    point is inside a mesh where its winding_number is above 0.5, which also answers for open meshes such as a TSDF
    surface; ``beta`` and ``exact`` as there, ``bricks`` a pair (bricks of a, bricks of b) built before, and no face
    grid is built.  ValueError before any launch on n_samples < 1, a bad
    seed or rule, a mesh without faces, and as kernels.mesh_face_grid states."""
    K._count_arg(n_samples, "n_samples")
    if n_samples < 1:
        raise ValueError(f"n_samples must be >= 1, got {n_samples!r}")
    K._seed_arg(seed)
    _generalized_args(rule, beta, exact, bricks)
    if cell_size is not None:
        K._cell_size_arg(cell_size)
    if bricks is not None and (not isinstance(bricks, (tuple, list)) or len(bricks) != 2):
        raise ValueError("bricks must be a pair: the mesh_winding_bricks of mesh_a and of mesh_b")
    for m in (mesh_a, mesh_b):  # both meshes before the first grid's launches
        K._faces_arg(m.faces, K._finite_vertices(m.vertices))
        if m.faces.shape[0] == 0:
            raise ValueError("volume_iou needs meshes with faces")
    if rule == "generalized":
        if bricks is None:
            bricks = (K.mesh_winding_bricks(mesh_a.vertices, mesh_a.faces),
                      K.mesh_winding_bricks(mesh_b.vertices, mesh_b.faces))
        for m, b in zip((mesh_a, mesh_b), bricks):
            K._winding_bricks_arg(b, int(m.faces.shape[0]))
    else:
        grid_a = K.mesh_face_grid(mesh_a.vertices, mesh_a.faces, cell_size)
        grid_b = K.mesh_face_grid(mesh_b.vertices, mesh_b.faces, cell_size)
    both = torch.cat([mesh_a.vertices, mesh_b.vertices])
    box = torch.cat([both.amin(0), both.amax(0)]).tolist()
    lo, hi = box[:3], box[3:]
    points = K.box_points(n_samples, lo, hi, seed=seed, device=mesh_a.vertices.device)
    if rule == "generalized":
        ia, ib = (K.mesh_winding_number(points, m.vertices, m.faces, b, beta=beta, exact=exact,
                                        finite_checked=True) > 0.5 for m, b in zip((mesh_a, mesh_b), bricks))
    else:
        ia = _inside(*K.mesh_point_crossings(points, mesh_a.vertices, mesh_a.faces, grid_a, finite_checked=True), rule)
        ib = _inside(*K.mesh_point_crossings(points, mesh_b.vertices, mesh_b.faces, grid_b, finite_checked=True), rule)
    counts = torch.stack([ia.sum(), ib.sum(), (ia & ib).sum(), (ia | ib).sum()]).tolist()  # one host read
    scale = ((hi[0] - lo[0]) * (hi[1] - lo[1])) * (hi[2] - lo[2]) / n_samples
    out = dict(zip(("volume_a", "volume_b", "intersection", "union"), (c * scale for c in counts)))
    out.update(zip(("count_a", "count_b", "count_intersection", "count_union"), counts))
    out["iou"] = counts[2] / counts[3] if counts[3] else 0.0
    out["n_samples"], out["box"] = n_samples, (lo, hi)
    return out


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
