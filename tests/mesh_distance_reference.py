"""Reference for the exact point-to-surface distance (a helper, not a test file): the contract of DESIGN §3.11.5
restated in numpy float64 with every operation in its order, plus the inputs the tests share.

The rules.  Corners a, b, c and the query q are fp32 values converted to float64.  dot(u, v) = (x x' + y y') + z z'.
With ab = b - a, ac = c - a, ap = q - a, bp = q - b, cp = q - c and d1 = ab.ap, d2 = ac.ap, d3 = ab.bp, d4 = ac.bp,
d5 = ab.cp, d6 = ac.cp, vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4, the regions are tested in this order:

  vertex a   d1 <= 0 and d2 <= 0                              a
  vertex b   d3 >= 0 and d4 <= d3                             b
  edge ab    vc <= 0 and d1 >= 0 and d3 <= 0                  a + clamp01(d1 / (d1 - d3)) ab
  vertex c   d6 >= 0 and d5 <= d6                             c
  edge ac    vb <= 0 and d2 >= 0 and d6 <= 0                  a + clamp01(d2 / (d2 - d6)) ac
  edge bc    va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0        b + clamp01((d4 - d3) / ((d4 - d3) + (d5 - d6))) (c - b)
  interior   s = (va + vb) + vc > 0                           (a + v ab) + w ac, v = clamp01(vb / s), w = clamp01(vc / s),
                                                              w = 1 - v when v + w > 1

clamp01(t) = t >= 0 ? (t <= 1 ? t : 1) : 0 (a NaN counts as 0).  d2 = dot(q - point, q - point) with the float64 point;
the point is then rounded to fp32.  A face with a repeated index, with a cross product (mesh_metrics_reference.face_cross)
of exactly (0, 0, 0), or that reaches the interior with s <= 0 is its three edges ab, ac, bc as segments:
t = clamp01(((q - p0) . e) / (e . e)), t = 0 when e . e == 0, point = p0 + t e, the smallest d2 and on a tie the earlier
edge.  Nearest face: brute force over all faces, the first index of the smallest d2.

Registration: face f lies in every cell of [cell_index(min corner), cell_index(max corner)] per axis, with the fp32
cell index t = (x - lo) * inv, i = clamp(floor(t), 0, dim - 1); key = (cell_id << 32) | f, cell_id = (ix ny + iy) nz + iz.
"""
import functools
import math

import numpy as np

import mesh_metrics_reference as MR

F32, F64 = np.float32, np.float64
MAX_DIM = 1024


def dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def clamp01(t):
    with np.errstate(invalid="ignore"):
        return np.where(t >= 0, np.where(t <= 1, t, 1.0), 0.0)


def _segment(p0, p1, q):
    e, w = p1 - p0, q - p0
    ee = dot(e, e)
    with np.errstate(all="ignore"):
        t = np.where(ee == 0, 0.0, clamp01(dot(w, e) / ee))
    r = p0 + t[..., None] * e
    d = q - r
    return dot(d, d), r


def closest_points(vertices, faces, query):
    """(d2 (n,F) float64, point (n,F,3) float32): every query against every face."""
    p = np.ascontiguousarray(vertices, F32).reshape(-1, 3).astype(F64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    q = np.ascontiguousarray(query, F32).reshape(-1, 1, 3).astype(F64)
    a, b, c = p[f[:, 0]][None], p[f[:, 1]][None], p[f[:, 2]][None]
    ab, ac, bc = b - a, c - a, c - b
    ap, bp, cp = q - a, q - b, q - c
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    u1, u2 = d4 - d3, d5 - d6
    s = (va + vb) + vc
    with np.errstate(all="ignore"):
        t_ab = clamp01(d1 / (d1 - d3))
        t_ac = clamp01(d2 / (d2 - d6))
        t_bc = clamp01(u1 / (u1 + u2))
        v, w = clamp01(vb / s), clamp01(vc / s)
    w = np.where(v + w > 1, 1.0 - v, w)
    r_in = (a + v[..., None] * ab) + w[..., None] * ac
    regions = [((d1 <= 0) & (d2 <= 0), a + 0 * q),
               ((d3 >= 0) & (d4 <= d3), b + 0 * q),
               ((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + t_ab[..., None] * ab),
               ((d6 >= 0) & (d5 <= d6), c + 0 * q),
               ((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + t_ac[..., None] * ac),
               ((va <= 0) & (u1 >= 0) & (u2 >= 0), b + t_bc[..., None] * bc)]
    r, hit = r_in, np.zeros(s.shape, bool)
    for cond, point in reversed(regions):  # the first region that holds wins
        r = np.where(cond[..., None], point, r)
        hit |= cond
    dq = q - r
    d2_walk = dot(dq, dq)
    cross = MR.face_cross(vertices, faces)
    flat = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2]) | (cross == 0).all(1)
    flat = flat[None] | (~hit & ~(s > 0))
    sd2, sr = _segment(a, b, q)
    for p0, p1 in ((a, c), (b, c)):
        e2, er = _segment(p0, p1, q)
        take = e2 < sd2
        sd2, sr = np.where(take, e2, sd2), np.where(take[..., None], er, sr)
    return np.where(flat, sd2, d2_walk), np.where(flat[..., None], sr, r).astype(F32)


def nearest_faces(vertices, faces, query, chunk=256):
    """Brute force: (d2 (n,) float64, face (n,) int32, closest (n,3) fp32); argmin returns the first of equal values.
    F == 0: +inf, -1, the query."""
    q = np.ascontiguousarray(query, F32).reshape(-1, 3)
    n, F = len(q), len(np.asarray(faces).reshape(-1, 3))
    if F == 0:
        return np.full(n, np.inf, F64), np.full(n, -1, np.int32), q.copy()
    d2, face, closest = np.empty(n, F64), np.empty(n, np.int32), np.empty((n, 3), F32)
    chunk = max(1, min(chunk, 2 ** 19 // F))  # a few dozen (chunk, F, 3) float64 temporaries live at once
    for s in range(0, n, chunk):
        d, r = closest_points(vertices, faces, q[s:s + chunk])
        j = np.argmin(d, 1)
        rows = np.arange(len(j))
        face[s:s + chunk], d2[s:s + chunk], closest[s:s + chunk] = j, d[rows, j], r[rows, j]
    return d2, face, closest


# ------------------------------------------------------------------ the grid


def face_grid(vertices, faces, cell_size=None):
    """{lo (3,) fp32, cell, inv (fp32), dims (3 ints)} by the rule of kernels.mesh_face_grid: the box of ALL vertices,
    default cell = longest extent / clamp(ceil(sqrt(F) / 2), 1, 1024)."""
    v = np.ascontiguousarray(vertices, F32).reshape(-1, 3)
    F = len(np.asarray(faces).reshape(-1, 3))
    lo = v.min(0)
    ext = v.max(0) - lo
    with np.errstate(all="ignore"):
        if cell_size is None:
            k = min(max(math.ceil(math.sqrt(F) / 2.0), 1), MAX_DIM)
            cell = ext.max() / F32(k) if ext.max() > 0 else F32(1.0)
            inv = F32(1.0) / cell
            if not (np.isfinite(cell) and cell > 0 and np.isfinite(inv) and inv > 0):
                cell, inv = F32(1.0), F32(1.0)
        else:
            cell = F32(cell_size)
            inv = F32(1.0) / cell
        cells = np.floor(ext * inv)
    if cell_size is None:
        cells = np.minimum(cells, MAX_DIM - 1)
    assert cells.max() + 1 <= MAX_DIM
    return {"lo": lo, "cell": F32(cell), "inv": F32(inv), "dims": [int(c) + 1 for c in cells]}


def cell_index(grid, axis, x):
    t = (np.asarray(x, F32) - grid["lo"][axis]) * grid["inv"]
    assert t.dtype == F32
    return np.clip(np.floor(t), 0, grid["dims"][axis] - 1).astype(np.int64)


def face_boxes(vertices, faces, grid):
    """(lo (F,3), hi (F,3)) int64: the index box of every face"""
    v = np.ascontiguousarray(vertices, F32).reshape(-1, 3)
    corners = v[np.asarray(faces, np.int64).reshape(-1, 3)]  # (F, 3 corners, 3 axes)
    lo = np.stack([cell_index(grid, c, corners[:, :, c].min(1)) for c in range(3)], 1)
    hi = np.stack([cell_index(grid, c, corners[:, :, c].max(1)) for c in range(3)], 1)
    return lo, hi


def face_cell_counts(vertices, faces, grid):
    lo, hi = face_boxes(vertices, faces, grid)
    return np.prod(hi - lo + 1, 1).astype(np.int64) if len(lo) else np.zeros(0, np.int64)


def face_keys(vertices, faces, grid):
    """The sorted keys (cell_id << 32) | face of every (cell, face) pair, int64."""
    lo, hi = face_boxes(vertices, faces, grid)
    _, ny, nz = grid["dims"]
    keys = []
    for f in range(len(lo)):
        ix, iy, iz = np.meshgrid(*(np.arange(lo[f, c], hi[f, c] + 1) for c in range(3)), indexing="ij")
        keys.append(((((ix * ny + iy) * nz + iz) << 32) | f).reshape(-1))
    return np.sort(np.concatenate(keys)) if keys else np.zeros(0, np.int64)


def grid_nearest_faces(vertices, faces, query, grid):
    """The search of the kernel, shell by shell, with its stopping rule: (d2, face, closest) as nearest_faces."""
    q = np.ascontiguousarray(query, F32).reshape(-1, 3)
    keys = face_keys(vertices, faces, grid)
    cells, members = keys >> 32, (keys & 0xffffffff).astype(np.int64)
    nx, ny, nz = grid["dims"]
    cell = float(grid["cell"])
    d2, face, closest = np.full(len(q), np.inf, F64), np.full(len(q), -1, np.int32), q.copy()
    if len(keys) == 0:
        return d2, face, closest
    for i in range(len(q)):
        c = [int(cell_index(grid, k, q[i, k])) for k in range(3)]
        for r in range(max(nx, ny, nz)):
            if r >= 2:
                up = F32(d2[i])
                if float(up) < d2[i]:
                    up = np.nextafter(up, F32(np.inf))
                bound = (float(r - 1) - 0.00390625) * cell
                if float(up) <= (bound * bound) * (1.0 - 0.0009765625):
                    break
            box = [(max(c[k] - r, 0), min(c[k] + r, n - 1)) for k, n in enumerate((nx, ny, nz))]
            ids = [(ix * ny + iy) * nz + iz
                   for ix in range(box[0][0], box[0][1] + 1) for iy in range(box[1][0], box[1][1] + 1)
                   for iz in range(box[2][0], box[2][1] + 1)
                   if max(abs(ix - c[0]), abs(iy - c[1]), abs(iz - c[2])) == r]
            cand = np.unique(members[np.isin(cells, ids)])
            if len(cand) == 0:
                continue
            d, p = closest_points(vertices, np.asarray(faces).reshape(-1, 3)[cand], q[i:i + 1])
            j = int(np.argmin(d[0]))  # cand ascends: the first is the smallest face
            if d[0, j] < d2[i] or (d[0, j] == d2[i] and (face[i] < 0 or cand[j] < face[i])):
                d2[i], face[i], closest[i] = d[0, j], cand[j], p[0, j]
    return d2, face, closest


# ------------------------------------------------------------------ shared inputs

TRIANGLE = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F32), np.array([[0, 1, 2]], np.int32))

# query, d2, closest point (None: not stated) on TRIANGLE; one row per region of the walk, then on and above the face
TABLE = (((.25, .25, 1), 1.0, (.25, .25, 0)),
         ((-1, -1, 0), 2.0, (0, 0, 0)),
         ((2, 0, 0), 1.0, (1, 0, 0)),
         ((0, 3, 0), 4.0, (0, 1, 0)),
         ((1, 1, 0), 0.5, (.5, .5, 0)),
         ((.5, -2, 0), 4.0, (.5, 0, 0)),
         ((-2, .5, 0), 4.0, (0, .5, 0)),
         ((.25, .25, 0), 0.0, None),
         ((1, 1, 1), 1.5, None))


def soup60():
    return MR.soup60()


def tiny_face_mesh():
    return MR.tiny_face_mesh()


@functools.lru_cache(maxsize=None)
def spheres():
    v, f, _ = MR.sample_meshes()["spheres"]
    return v, f


def _extent(v):
    return float((v.max(0) - v.min(0)).max())


def one_cell(v):
    """a cell that holds the whole box"""
    return 2.0 * _extent(v)


def cap_cell(v, dims=MAX_DIM):
    """the smallest cell with ``dims`` cells along the longest axis: floor(extent / cell) = dims - 1"""
    return _extent(v) / (dims - 0.5)


@functools.lru_cache(maxsize=None)
def queries(name, n=1000, far=100, seed=3):
    """n queries for the mesh ``name``: n - far in the box widened by a tenth, ``far`` of them 5 to 50 extents away."""
    v, _ = {"soup60": soup60, "tiny_face": tiny_face_mesh}[name]()
    rng = np.random.default_rng(seed)
    lo, hi = v.min(0), v.max(0)
    pad = 0.1 * (hi - lo).max()
    near = rng.uniform(lo - pad, hi + pad, (n - far, 3))
    direction = rng.normal(size=(far, 3))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    away = (lo + hi) / 2 + direction * rng.uniform(5, 50, (far, 1)) * (hi - lo).max()
    return np.concatenate([near, away]).astype(F32)


@functools.lru_cache(maxsize=None)
def cap_queries(n=1000, outside=100, seed=4, cells=24):
    """Queries for tiny_face_mesh on the grid of cap_cell (1024 cells per axis).  A query r cells from the surface
    walks r shells and about 4/3 r^3 columns, so these stay within ``cells`` cells of a face: n - outside around
    points of the two faces, ``outside`` below the box (z < its lower face, under the large face)."""
    v, f = tiny_face_mesh()
    rng = np.random.default_rng(seed)
    cell = cap_cell(v)
    w = rng.dirichlet((1, 1, 1), n)
    on = np.einsum("nk,nkc->nc", w, v[f[rng.integers(0, len(f), n)]].astype(F64))
    q = on + rng.uniform(-cells * cell, cells * cell, (n, 3))
    q[:outside, 2] = -rng.uniform(1, cells, outside) * cell
    q[:outside, :2] = np.einsum("nk,nkc->nc", w[:outside], np.broadcast_to(v[f[1]], (outside, 3, 3)).astype(F64))[:, :2]
    return q.astype(F32)


@functools.lru_cache(maxsize=None)
def brute(name, which="queries"):
    v, f = {"soup60": soup60, "tiny_face": tiny_face_mesh}[name]()
    return nearest_faces(v, f, queries(name) if which == "queries" else cap_queries())


def mirror_pair(rng):
    """(vertices (6,3), faces (2,3)): a random triangle with x > 0 and its mirror image in x = 0, the image first"""
    t = rng.uniform(-1, 1, (3, 3)).astype(F32)
    t[:, 0] = np.abs(t[:, 0]) + F32(0.01)
    m = t.copy()
    m[:, 0] = -m[:, 0]
    return np.concatenate([m, t]), np.array([[0, 1, 2], [3, 4, 5]], np.int32)


def margin(*arrays):
    """m = 2 sqrt(3) 2^-24 max|coordinate|: a surface point rounded once to fp32 moves by at most sqrt(3) 2^-24 times
    the largest coordinate; the factor 2 covers the float64 arithmetic."""
    return 2.0 * math.sqrt(3.0) * 2.0 ** -24 * max(float(np.abs(a).max()) for a in arrays)


# ------------------------------------------------------------------ the exact metric dict


def unit_face_normals(vertices, faces):
    c = MR.face_cross(vertices, faces)
    d = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
    return np.where(d[:, None] > 0, c / np.where(d > 0, d, 1.0)[:, None], 0.0)


def mesh_distance_exact(mesh_a, mesh_b, n_samples, seed=0, thresholds=(), normals=False):
    """mesh_metrics.mesh_distance(..., exact=True): the samples of a against the surface of b and the other way."""
    kind = "face" if normals else None
    sa = MR.sample_surface(*mesh_a, n_samples, seed, kind)
    sb = MR.sample_surface(*mesh_b, n_samples, seed, kind)
    d2_ab, face_ab, _ = nearest_faces(*mesh_b, sa[0])
    d2_ba, face_ba, _ = nearest_faces(*mesh_a, sb[0])
    out, sides = {}, {}
    for name, d2 in (("a_to_b", d2_ab), ("b_to_a", d2_ba)):
        d = np.sqrt(d2)
        sides[name] = (d, float(d2.mean()))
        out[f"{name}_mean"], out[f"{name}_rms"], out[f"{name}_max"] = float(d.mean()), float(np.sqrt(d2.mean())), float(d.max())
    out["chamfer"] = (out["a_to_b_mean"] + out["b_to_a_mean"]) / 2
    out["chamfer_sq"] = sides["a_to_b"][1] + sides["b_to_a"][1]
    out["hausdorff"] = max(out["a_to_b_max"], out["b_to_a_max"])
    for tau in thresholds:
        tau = float(tau)
        p = float((sides["a_to_b"][0] <= tau).sum()) / n_samples
        r = float((sides["b_to_a"][0] <= tau).sum()) / n_samples
        out[f"precision@{tau}"], out[f"recall@{tau}"] = p, r
        out[f"fscore@{tau}"] = 2 * p * r / (p + r) if p + r > 0 else 0.0
    if normals:
        na, nb = sa[2].astype(F64), sb[2].astype(F64)
        c_ab = np.abs((na * unit_face_normals(*mesh_b)[face_ab]).sum(1)).mean()
        c_ba = np.abs((nb * unit_face_normals(*mesh_a)[face_ba]).sum(1)).mean()
        out["normal_consistency"] = float((c_ab + c_ba) / 2)
    return out
