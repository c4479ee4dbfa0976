"""Reference for nearest-hit ray casting against a mesh (a helper, not a test file): the contract of DESIGN §3.11.6
restated in numpy float64 with every operation in its order, plus the inputs the tests share.

The rules.  A ray is a row [o, d, near, far] of fp32 values converted to float64, its points o + t d; d is not
normalised.  Corners a, b, c are fp32 values converted to float64.  dot(x, y) = (x0 y0 + x1 y1) + x2 y2, cross(x, y) =
(x1 y2 - x2 y1, x2 y0 - x0 y2, x0 y1 - x1 y0), every product and difference rounded once.

  e1 = b - a, e2 = c - a, p = cross(d, e2), det = dot(e1, p), s = o - a,
  u = dot(s, p) / det, q = cross(s, e1), v = dot(d, q) / det, t = dot(e2, q) / det.

Never hit: a face with a repeated index, with mesh_metrics_reference.face_cross exactly (0, 0, 0), with det == 0 and,
with cull, det <= 0 (det > 0: the ray runs against the winding normal).  Hit: u >= 0, u <= 1, v >= 0, u + v <= 1,
near <= t, t <= far and, per axis k, P_k = o_k + t d_k in [min_k - m, max_k + m] of the face's corners,
m = 2^-30 max |coordinate| over ALL vertices.  A NaN fails every comparison.  Per ray: the smallest t, the smaller face
on equal t; t = +inf, face = -1, bary = (0, 0) on a miss; bary = (u, v) rounded to fp32.

grid_ray_cast restates the walk of csrc/mesh_raycast_core.hpp operation by operation (Python floats are IEEE doubles):
the clip to the box widened by S = 2^-6 of a cell, the layers along the major axis, the cells of the two other axes
over a layer's interval, the stop before a layer entered after the best t.  It selects WHICH faces a ray tests; the
test of a face is face_hits, the same for both.
"""
import functools
import math

import numpy as np

import mesh_distance_reference as D
import mesh_metrics_reference as MR

F32, F64 = np.float32, np.float64
SLACK = 0.015625
FAR_ORIGIN = 4294967296.0
dot = D.dot


def cross(x, y):
    return np.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1], x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2],
                     x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], -1)


def c_max(vertices):
    v = np.asarray(vertices, F32)
    return float(np.abs(v).max()) if v.size else 0.0


def margin(vertices):
    return 2.0 ** -30 * c_max(vertices)


def dead_faces(vertices, faces):
    """(F,) bool: a repeated index or a cross product of exactly (0, 0, 0)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2]) | \
        (MR.face_cross(vertices, faces) == 0).all(1)


def _face_hits(vertices, faces, rays, cull, box_clause):
    p = np.ascontiguousarray(vertices, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    r = np.ascontiguousarray(rays, F32).reshape(-1, 8).astype(F64)
    o, d, near, far = r[:, None, 0:3], r[:, None, 3:6], r[:, None, 6], r[:, None, 7]
    corners = p[f]  # (F, 3 corners, 3 axes) fp32
    a, b, c = (corners[None, :, k].astype(F64) for k in range(3))
    e1, e2 = b - a, c - a
    pv = cross(d, e2)
    det = dot(e1, pv)
    s = o - a
    with np.errstate(all="ignore"):
        u = dot(s, pv) / det
        q = cross(s, e1)
        v = dot(d, q) / det
        t = dot(e2, q) / det
        ok = ~dead_faces(vertices, faces)[None] & ~(det == 0)
        if cull:
            ok &= ~(det <= 0)
        ok &= (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (near <= t) & (t <= far)
        if box_clause:
            m = margin(vertices)
            P = o + t[..., None] * d
            mn, mx = corners.min(1).astype(F64)[None] - m, corners.max(1).astype(F64)[None] + m
            ok &= ((P >= mn) & (P <= mx)).all(-1)
    return np.where(ok, t, np.inf), u, v


def face_hits(vertices, faces, rays, cull=False, box_clause=True, chunk=None):
    """(t, u, v), each (n, F) float64: every ray against every face; t = +inf where the face is not hit."""
    rays = np.ascontiguousarray(rays, F32).reshape(-1, 8)
    n, F = len(rays), len(np.asarray(faces).reshape(-1, 3))
    out = [np.empty((n, F), F64) for _ in range(3)]
    chunk = chunk or max(1, 2 ** 18 // max(F, 1))  # a few dozen (chunk, F, 3) float64 temporaries live at once
    for s in range(0, n, chunk):
        for dst, src in zip(out, _face_hits(vertices, faces, rays[s:s + chunk], cull, box_clause)):
            dst[s:s + chunk] = src
    return tuple(out)


def _pick(t, u, v):
    """the per-ray result from the (n, F) arrays: argmin returns the first of equal values"""
    n, F = t.shape
    if F == 0:
        return np.full(n, np.inf, F64), np.full(n, -1, np.int32), np.zeros((n, 2), F32)
    j = np.argmin(t, 1)
    rows = np.arange(n)
    best = t[rows, j]
    hit = best < np.inf
    bary = np.where(hit[:, None], np.stack([u[rows, j], v[rows, j]], 1), 0.0).astype(F32)
    return best, np.where(hit, j, -1).astype(np.int32), bary


def ray_cast(vertices, faces, rays, cull=False, box_clause=True):
    """Brute force: (t (n,) float64, face (n,) int32, bary (n,2) fp32)."""
    return _pick(*face_hits(vertices, faces, rays, cull, box_clause))


# ------------------------------------------------------------------ the walk


def _floor_cell(x, dim):
    if x != x:
        return 0  # a NaN counts as 0
    return int(min(max(math.floor(x) if abs(x) < 2.0 ** 62 else x, 0), dim - 1))


def _minor_cells(rel, d, dim, a, b, inv):
    sa, sb = a * d, b * d
    ca, cb = (rel + sa) * inv, (rel + sb) * inv
    pl, ph = min(ca, cb) - SLACK, max(ca, cb) + SLACK
    return _floor_cell(pl, dim), _floor_cell(ph, dim), ph >= 0.0 and pl <= float(dim)


def grid_ray_cast(vertices, faces, rays, grid, cull=False, counts=False, keys=None):
    """The walk of the kernel: (t, face, bary) as ray_cast; with ``counts`` also (layers walked, faces tested) per ray,
    (n, 2) int64.  ``keys``: the sorted keys of the grid when the caller has them (then a face is tested when the walk
    meets it, not every face up front: for meshes too large for the (n, F) arrays of face_hits)."""
    rays = np.ascontiguousarray(rays, F32).reshape(-1, 8)
    faces = np.asarray(faces).reshape(-1, 3)
    n, F = len(rays), len(faces)
    if keys is None:
        T, U, V = face_hits(vertices, faces, rays, cull)
        keys = D.face_keys(vertices, faces, grid)

        def tested(i, cand):
            return T[i, cand], U[i, cand], V[i, cand]
    else:
        def tested(i, cand):
            return tuple(x[0] for x in _face_hits(vertices, faces[cand], rays[i:i + 1], cull, True))
    cells, members = keys >> 32, (keys & 0xffffffff).astype(np.int64)
    first = np.flatnonzero(np.r_[True, cells[1:] != cells[:-1]]) if len(keys) else np.zeros(0, np.int64)
    runs = {int(c): (int(s), int(e)) for c, s, e in zip(cells[first], first, np.r_[first[1:], len(keys)])}
    nx, ny, nz = dims = [int(x) for x in grid["dims"]]
    cell = float(grid["cell"])
    inv = 1.0 / cell
    lo = [float(x) for x in grid["lo"]]
    out_t, out_f, out_uv = np.full(n, np.inf, F64), np.full(n, -1, np.int64), np.zeros((n, 2), F64)
    count = np.zeros((n, 2), np.int64)
    r64 = rays.astype(F64)
    for i in range(n if len(keys) else 0):
        o, d, t0, t1 = r64[i, 0:3].tolist(), r64[i, 3:6].tolist(), float(r64[i, 6]), float(r64[i, 7])
        best_t, best_f = math.inf, -1

        def consider(cand):
            nonlocal best_t, best_f
            if len(cand):
                tc, uc, vc = tested(i, cand)
                j = int(np.lexsort((cand, tc))[0])  # the smallest t, then the smallest face
                if tc[j] < best_t or (tc[j] == best_t and tc[j] < math.inf and cand[j] < best_f):
                    best_t, best_f, out_uv[i] = float(tc[j]), int(cand[j]), (uc[j], vc[j])
            count[i, 1] += len(cand)

        rel = [o[k] - lo[k] for k in range(3)]
        if not all(abs(rel[k]) <= FAR_ORIGIN * cell for k in range(3)):
            consider(np.arange(F))
            out_t[i], out_f[i] = best_t, best_f
            continue
        miss = False
        for k in range(3):
            a, b = -SLACK * cell, (float(dims[k]) + SLACK) * cell
            if d[k] == 0.0:
                miss = miss or not (a <= rel[k] <= b)
                continue
            ta, tb = (a - rel[k]) / d[k], (b - rel[k]) / d[k]
            t0, t1 = max(t0, min(ta, tb)), min(t1, max(ta, tb))
        if miss or not t0 <= t1:
            continue
        M = 0
        if abs(d[1]) > abs(d[M]):
            M = 1
        if abs(d[2]) > abs(d[M]):
            M = 2
        dm = d[M]
        if dm == 0.0:
            continue
        sg, nM = (1 if dm > 0 else -1), dims[M]
        s0 = t0 * dm
        layer = _floor_cell((rel[M] + s0) * inv - float(sg), nM)
        for _ in range(nM):
            if not 0 <= layer < nM:
                break
            A, B = (float(layer) - SLACK) * cell, (float(layer + 1) + SLACK) * cell
            ta, tb = (A - rel[M]) / dm, (B - rel[M]) / dm
            tin, tout = (ta, tb) if sg > 0 else (tb, ta)
            if tin > best_t or tin > t1:
                break
            a, b = max(tin, t0), min(tout, t1)
            this, layer = layer, layer + sg
            if not a <= b:
                continue
            count[i, 0] += 1
            box, inside = [], True
            for k in range(3):
                if k == M:
                    box.append((this, this))
                else:
                    c0, c1, ok = _minor_cells(rel[k], d[k], dims[k], a, b, inv)
                    box.append((c0, c1))
                    inside = inside and ok
            if not inside:
                continue
            for ix in range(box[0][0], box[0][1] + 1):
                for iy in range(box[1][0], box[1][1] + 1):
                    spans = [runs[c] for c in range((ix * ny + iy) * nz + box[2][0], (ix * ny + iy) * nz + box[2][1] + 1)
                             if c in runs]
                    if spans:
                        consider(np.concatenate([members[s:e] for s, e in spans]))
        out_t[i], out_f[i] = best_t, best_f
    result = (out_t, out_f.astype(np.int32), out_uv.astype(F32))
    return result + (count,) if counts else result


# ------------------------------------------------------------------ shared inputs

TRIANGLE = D.TRIANGLE
INF = float("inf")

# (o, d, near, far), cull -> (t, u, v) or None for a miss, on TRIANGLE (normal +z): the table of the issue
TABLE = (
    (((.25, .5, 1), (0, 0, -1), 0, INF), False, (1.0, .25, .5)),      # interior, from above: a front hit
    (((.25, .5, 1), (0, 0, -1), 0, INF), True, (1.0, .25, .5)),
    (((.25, .5, 2), (0, 0, -4), 0, INF), False, (.5, .25, .5)),       # d is not normalised: t is the ray's own
    (((.25, .5, -1), (0, 0, 1), 0, INF), False, (1.0, .25, .5)),      # from below: a back hit
    (((.25, .5, -1), (0, 0, 1), 0, INF), True, None),                 # ... culled
    (((.5, 0, 1), (0, 0, -1), 0, INF), False, (1.0, .5, 0.0)),        # the midpoint of ab: v = 0
    (((0, .5, 1), (0, 0, -1), 0, INF), False, (1.0, 0.0, .5)),        # the midpoint of ac: u = 0
    (((.5, .5, 1), (0, 0, -1), 0, INF), False, (1.0, .5, .5)),        # the midpoint of bc: 1 - u - v = 0
    (((0, 0, 1), (0, 0, -1), 0, INF), False, (1.0, 0.0, 0.0)),        # corner a
    (((1, 0, 1), (0, 0, -1), 0, INF), False, (1.0, 1.0, 0.0)),        # corner b
    (((.5, -2.0 ** -20, 1), (0, 0, -1), 0, INF), False, None),        # just outside ab
    (((.5 + 2.0 ** -20, .5, 1), (0, 0, -1), 0, INF), False, None),    # just outside bc
    (((-1, .25, 1), (1, 0, 0), 0, INF), False, None),                 # parallel to the plane
    (((-1, .25, 0), (1, 0, 0), 0, INF), False, None),                 # in the plane
    (((.25, .5, 1), (0, 0, 1), 0, INF), False, None),                 # pointing away
    (((.25, .5, 1), (0, 0, -1), 1.5, INF), False, None),              # near beyond the hit
    (((.25, .5, 1), (0, 0, -1), 0, .5), False, None),                 # far before the hit
    (((.25, .5, 1), (0, 0, -1), 2, .5), False, None),                 # far < near
    (((.25, .5, 1), (0, 0, -1), 1, 1), False, (1.0, .25, .5)),        # near == t == far
    (((.25, .5, 1), (0, 0, -1), -INF, INF), False, (1.0, .25, .5)),
)


def pack(o, d, near=0.0, far=INF):
    o, d = np.asarray(o, F64).reshape(-1, 3), np.asarray(d, F64).reshape(-1, 3)
    n = len(o)
    out = np.empty((n, 8), F32)
    out[:, 0:3], out[:, 3:6], out[:, 6], out[:, 7] = o, d, near, far
    return out


def table_rays():
    return np.array([[*o, *d, near, far] for ((o, d, near, far), _, _) in TABLE], F32)


def octahedron():
    """closed, convex, wound outwards: |x| / 1 + |y| / 1.5 + |z| / 2 = 1"""
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1.5, 0], [0, -1.5, 0], [0, 0, 2], [0, 0, -2]], F32)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return v, f


MESHES = {"soup60": D.soup60, "tiny_face": D.tiny_face_mesh, "spheres": D.spheres, "octahedron": octahedron}


def mesh(name):
    return MESHES[name]()


def _points_on_live_faces(v, f, n, rng):
    live = np.flatnonzero(~dead_faces(v, f))
    w = rng.dirichlet((1, 1, 1), n)
    return np.einsum("nk,nkc->nc", w, v[f[live[rng.integers(0, len(live), n)]]].astype(F64))


def _lengths(d, rng):
    return d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (len(d), 1))


@functools.lru_cache(maxsize=None)
def rays(name, n=1000, seed=5):
    """The ray set of a mesh: origins uniform in the box widened by half its longest extent; the first half aimed at
    random points of live faces, the second half with normal-distributed directions; |d| in [0.5, 2]; near = 0,
    far = +inf."""
    v, f = mesh(name)
    rng = np.random.default_rng(seed)
    lo, hi = v.min(0).astype(F64), v.max(0).astype(F64)
    pad = 0.5 * (hi - lo).max()
    o = rng.uniform(lo - pad, hi + pad, (n, 3))
    d = rng.normal(size=(n, 3))
    d[:n // 2] = _points_on_live_faces(v, f, n // 2, rng) - o[:n // 2]
    return pack(o, _lengths(d, rng))


@functools.lru_cache(maxsize=None)
def axis_rays(name, n=300, seed=6):
    """Axis-parallel rays, both signs: a point of a live face displaced along an axis, aimed back at it.  Both faces
    of tiny_face lie in planes z = const, where a ray along x or y runs inside the plane and is a miss by the rule:
    that mesh takes the z axis only."""
    v, f = mesh(name)
    rng = np.random.default_rng(seed)
    ext = float((v.max(0) - v.min(0)).max())
    o = _points_on_live_faces(v, f, n, rng).astype(F32).astype(F64)
    axis, sign = rng.choice((2,) if name == "tiny_face" else (0, 1, 2), n), rng.choice([-1.0, 1.0], n)
    d = np.zeros((n, 3))
    d[np.arange(n), axis] = sign * rng.uniform(0.5, 2.0, n)
    o[np.arange(n), axis] -= sign * rng.uniform(0.1, 1.5, n) * ext
    return pack(o, d)


def plane_rays(name, grid, n=200, seed=7):
    """Rays whose origin lies exactly on a cell plane lo + k cell (computed in fp32, as the grid's own arithmetic is)
    and that run along it: d has an exact zero on that axis."""
    v, _ = mesh(name)
    rng = np.random.default_rng(seed)
    lo, hi = v.min(0).astype(F64), v.max(0).astype(F64)
    pad = 0.25 * (hi - lo).max()
    o = rng.uniform(lo - pad, hi + pad, (n, 3)).astype(F32)
    d = rng.normal(size=(n, 3))
    axis = rng.integers(0, 3, n)
    for i in range(n):
        k = int(axis[i])
        plane = rng.integers(0, int(grid["dims"][k]) + 1)
        o[i, k] = F32(grid["lo"][k]) + F32(plane) * F32(grid["cell"])
        d[i, k] = 0.0
    return pack(o, _lengths(d, rng))


@functools.lru_cache(maxsize=None)
def inside_rays(name, n=300, seed=8):
    """origins inside the box of the vertices"""
    v, _ = mesh(name)
    rng = np.random.default_rng(seed)
    o = rng.uniform(v.min(0).astype(F64), v.max(0).astype(F64), (n, 3))
    return pack(o, _lengths(rng.normal(size=(n, 3)), rng))


@functools.lru_cache(maxsize=None)
def outside_rays(name, n=200, seed=9):
    """rays that stay on one side of the box: the origin beyond a face of it, the direction pointing farther away"""
    v, _ = mesh(name)
    rng = np.random.default_rng(seed)
    lo, hi = v.min(0).astype(F64), v.max(0).astype(F64)
    ext = (hi - lo).max()
    o = rng.uniform(lo - ext, hi + ext, (n, 3))
    d = rng.normal(size=(n, 3))
    axis, side = rng.integers(0, 3, n), rng.integers(0, 2, n)
    rows = np.arange(n)
    o[rows, axis] = np.where(side == 1, hi[axis] + rng.uniform(0.05, 2, n) * ext, lo[axis] - rng.uniform(0.05, 2, n) * ext)
    d[rows, axis] = np.where(side == 1, 1.0, -1.0) * np.abs(d[rows, axis])
    return pack(o, _lengths(d, rng))


@functools.lru_cache(maxsize=None)
def far_rays(name, n=100, seed=10):
    """origins 5 to 50 extents from the box's centre, aimed at points of live faces"""
    v, f = mesh(name)
    rng = np.random.default_rng(seed)
    lo, hi = v.min(0).astype(F64), v.max(0).astype(F64)
    direction = rng.normal(size=(n, 3))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    o = (lo + hi) / 2 + direction * rng.uniform(5, 50, (n, 1)) * (hi - lo).max()
    return pack(o, _lengths(_points_on_live_faces(v, f, n, rng) - o, rng))


@functools.lru_cache(maxsize=None)
def brute(name, which="rays", cull=False):
    v, f = mesh(name)
    r = {"rays": rays, "axis": axis_rays, "inside": inside_rays, "outside": outside_rays, "far": far_rays}[which](name)
    return ray_cast(v, f, r, cull)


def second_hit_rays(name):
    """the ray set with near just past its first hit (the next double after the reference's t, rounded UP to fp32):
    the first face is no longer a hit at that t, the next one along the ray is returned"""
    r = rays(name).copy()
    t = brute(name)[0]
    near = t.astype(F32)
    near = np.where(near.astype(F64) <= t, np.nextafter(near, F32(np.inf)), near)
    r[:, 6] = np.where(np.isfinite(t), near, 0.0)
    return r


def grid_cell(name, which):
    """the cell_size of the three grids of the tests: one cell, the default, the cap (1024 cells on an axis for
    tiny_face; 32 for the others, whose faces would have 10^9 keys at 1024)"""
    v, _ = mesh(name)
    if which == "cap":
        return D.cap_cell(v) if name == "tiny_face" else D.cap_cell(v, 32)
    return {"default": None, "one_cell": D.one_cell(v)}[which]


def sliver(scale=1.0):
    """(vertices, faces, rays (1,8)): a face whose cross product is tiny but not zero, and a ray that passes 98 units
    from it and that the test WITHOUT the box clause reports as a hit.  Unscaled: a = 0, b = (1, 0, 0),
    c = (2, 0, 2^-100), cross = (0, -2^-100, 0); o = (100, 1, 1), d = (0, -1, -1), so the ray meets the face's line, the
    x axis, at (100, 0, 0), t = 1.  det = d_y e2_z = -2^-100 is not zero, but the numerator of u is
    (100 d_y 2^-100 + -2) + 2, where the first term is absorbed, and that of v is d_y o_z - d_z o_y: both come out as
    exactly 0, so u = v = 0 and t = (-o_y 2^-100) / det = 1 pass every barycentric test although the hit point they
    name, corner a, is 100 units from o + t d.  ``scale`` (a power of two) scales everything and changes nothing."""
    s = float(scale)
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 2.0 ** -100]], F64) * s
    return v.astype(F32), np.array([[0, 1, 2]], np.int32), pack([[100 * s, s, s]], [[0, -s, -s]])


def camera(name):
    """(H, W, fx, fy, cx, cy, c2w (3,4) fp32) of a 16 x 12 view of the mesh from outside, looking at its centre along
    the camera's -z axis"""
    v, _ = mesh(name)
    lo, hi = v.min(0).astype(F64), v.max(0).astype(F64)
    centre, ext = (lo + hi) / 2, float((hi - lo).max())
    eye = centre + np.array([0.45, 0.3, 0.8]) * ext
    back = (eye - centre) / np.linalg.norm(eye - centre)
    right = np.cross([0.0, 1.0, 0.0], back)
    right /= np.linalg.norm(right)
    up = np.cross(back, right)
    c2w = np.concatenate([np.stack([right, up, back], 1), eye[:, None]], 1).astype(F32)
    return 12, 16, 14.0, 14.0, 8.0, 6.0, c2w
