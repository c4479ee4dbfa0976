"""Reference for point-in-mesh by exact crossing counts (a helper, not a test file): the contract of DESIGN §3.11.7
restated with fractions.Fraction for the exact part and Python floats (IEEE doubles) for the rounded part, plus the
inputs the tests share.

The rule.  The query q and the corners a, b, c are fp32 values.  The ray is q + t e_z, t > 0: open, straight up.
orient(P, Q, R) is the exact sign of (Qx - Px)(Ry - Py) - (Qy - Py)(Rx - Px).  Face f is crossed iff

  1. in fp32 compares: max(az, bz, cz) > qz, qx in [min, max] of the corners' x, qy in [min, max] of the corners' y;
  2. s = orient(a, b, c) != 0;
  3. for the directed edges U -> V of the projection taken counter-clockwise (a b, b c, c a, with b and c swapped when
     s < 0): e = orient(U, V, q) > 0, or e == 0 and (Vy < Uy, or Vy == Uy and Vx > Ux);
  4. in rounded double, e1 = b - a, e2 = c - a (not swapped), w = q - a, n = e1 x e2 (six products, three differences),
     g = (nx wx + ny wy) + nz wz: g < 0 and s > 0, or g > 0 and s < 0.

crossings = the number of crossed faces, winding = the sum of s over them.  brute tests every face; column_walk
restates which faces csrc/mesh_inside_core.hpp tests (the column of q's cell from q's own cell upwards, a face at
the key whose iz == max(cell_index(min corner z), cz)); the test of a face is the same for both.  orient_float
restates the device's filter and expansion operation by operation; orient_fraction knows nothing of them.
"""
import functools
from fractions import Fraction

import numpy as np

import mesh_distance_reference as D
import mesh_metrics_reference as MR
import mesh_smooth_reference as MS

F32, F64 = np.float32, np.float64
BOX_STREAM = 0x626f78
FILTER = 2.0 ** -48


# ------------------------------------------------------------------ orient


def orient_fraction(P, Q, R):
    """the exact sign, by rational arithmetic on the coordinates as given"""
    px, py, qx, qy, rx, ry = (Fraction(float(x)) for x in (P[0], P[1], Q[0], Q[1], R[0], R[1]))
    d = (qx - px) * (ry - py) - (qy - py) * (rx - px)
    return (d > 0) - (d < 0)


def two_sum(a, b):
    x = a + b
    bv = x - a
    av = x - bv
    return x, (a - av) + (b - bv)


def _sign(x):
    return (x > 0) - (x < 0)


def expansion_sign(terms):
    """the sign of the exact sum of the floats ``terms``: each is added into a non-overlapping expansion, smallest
    component first (grow-expansion); the sign is that of the last non-zero component"""
    h = []
    for t in terms:
        q = t
        for k in range(len(h)):
            q, h[k] = two_sum(q, h[k])
        h.append(q)
    for x in reversed(h):
        if x != 0.0:
            return _sign(x)
    return 0


def orient_float(P, Q, R):
    """(sign, took_exact_path): the device's computation in Python floats"""
    px, py, qx, qy, rx, ry = (float(x) for x in (P[0], P[1], Q[0], Q[1], R[0], R[1]))
    t = [qx * ry, -(qx * py), -(px * ry), -(qy * rx), qy * px, py * rx]
    total = ((t[0] + t[1]) + (t[2] + t[3])) + (t[4] + t[5])
    mag = ((abs(t[0]) + abs(t[1])) + (abs(t[2]) + abs(t[3]))) + (abs(t[4]) + abs(t[5]))
    if abs(total) > FILTER * mag:
        return (1 if total > 0 else -1), False
    return expansion_sign(t), True


# ------------------------------------------------------------------ the test of a face


def _edge_passes(U, V, q, orient):
    e = orient(U, V, q)
    return e > 0 or (e == 0 and (V[1] < U[1] or (V[1] == U[1] and V[0] > U[0])))


def box_rule(corners, q):
    """rule 1 for fp32 corners (..., 3 corners, 3 axes) and queries broadcastable to (..., 3), in fp32 compares"""
    assert corners.dtype == F32 and q.dtype == F32
    mn, mx = corners.min(-2), corners.max(-2)
    return (mx[..., 2] > q[..., 2]) & (q[..., 0] >= mn[..., 0]) & (q[..., 0] <= mx[..., 0]) & \
        (q[..., 1] >= mn[..., 1]) & (q[..., 1] <= mx[..., 1])


def crossed(a, b, c, q, orient=orient_fraction):
    """0 when the face (a, b, c) (fp32 triples) is not crossed by the ray from q, else s = +1 or -1"""
    tri = np.stack([a, b, c]).astype(F32)
    if not box_rule(tri, np.asarray(q, F32)):
        return 0
    s = orient(a, b, c)
    if s == 0:
        return 0
    B, C = (b, c) if s > 0 else (c, b)
    if not (_edge_passes(a, B, q, orient) and _edge_passes(B, C, q, orient) and _edge_passes(C, a, q, orient)):
        return 0
    a64, b64, c64, q64 = ([float(x) for x in p] for p in (a, b, c, q))
    e1 = [b64[k] - a64[k] for k in range(3)]
    e2 = [c64[k] - a64[k] for k in range(3)]
    w = [q64[k] - a64[k] for k in range(3)]
    n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
    g = (n[0] * w[0] + n[1] * w[1]) + n[2] * w[2]
    return s if (g < 0 and s > 0) or (g > 0 and s < 0) else 0


def _mesh(vertices, faces):
    return np.ascontiguousarray(vertices, F32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)


def brute(vertices, faces, query, orient=orient_fraction, chunk=512):
    """(crossings (n,) int32, winding (n,) int32): every face against every query.  Rule 1 is a vectorised fp32
    compare; the faces that pass it go through ``crossed`` one by one."""
    v, f = _mesh(vertices, faces)
    q = np.ascontiguousarray(query, F32).reshape(-1, 3)
    crossings, winding = np.zeros(len(q), np.int32), np.zeros(len(q), np.int32)
    if len(f) == 0:
        return crossings, winding
    corners = v[f]
    for s0 in range(0, len(q), chunk):
        rows, cols = np.nonzero(box_rule(corners[None], q[s0:s0 + chunk, None]))
        for i, j in zip(rows + s0, cols):
            s = crossed(*corners[j], q[i], orient)
            crossings[i] += s != 0
            winding[i] += s
    return crossings, winding


def column_walk(vertices, faces, query, grid, counts=False, keys=None, orient=orient_fraction):
    """The walk of the kernel: (crossings, winding) as brute; with ``counts`` also (keys scanned, faces tested)
    per query, (n, 2) int64.  ``keys``: the sorted keys of the grid when the caller has them (for meshes too large
    for face_keys' loop over the faces)."""
    v, f = _mesh(vertices, faces)
    q = np.ascontiguousarray(query, F32).reshape(-1, 3)
    if keys is None:
        keys = D.face_keys(v, f, grid)
    _, ny, nz = grid["dims"]
    crossings, winding = np.zeros(len(q), np.int32), np.zeros(len(q), np.int32)
    count = np.zeros((len(q), 2), np.int64)
    if len(keys):
        lz = D.cell_index(grid, 2, v[f][:, :, 2].min(1))
        cells = [D.cell_index(grid, k, q[:, k]) for k in range(3)]
        for i in range(len(q)):
            cx, cy, cz = (int(c[i]) for c in cells)
            base = (cx * ny + cy) * nz
            j = int(np.searchsorted(keys, (base + cz) << 32))
            while j < len(keys) and keys[j] < (base + nz) << 32:
                face, iz = int(keys[j] & 0xffffffff), int(keys[j] >> 32) - base
                j += 1
                count[i, 0] += 1
                if iz != max(int(lz[face]), cz):
                    continue
                count[i, 1] += 1
                s = crossed(*v[f[face]], q[i], orient)
                crossings[i] += s != 0
                winding[i] += s
    return (crossings, winding, count) if counts else (crossings, winding)


# ------------------------------------------------------------------ the layers above


def box_points(n, seed, lo, hi):
    """(n,3) fp32: coordinate c of point i = lo_c + u (hi_c - lo_c) in fp32, u = (rand64(seed, BOX_STREAM + c, i) >> 40)
    2^-24"""
    lo, hi = np.asarray(lo, F32), np.asarray(hi, F32)
    out = np.empty((n, 3), F32)
    i = np.arange(n, dtype=np.uint64)
    for c in range(3):
        u = (MR.rand64(seed, BOX_STREAM + c, i) >> np.uint64(40)).astype(F32) * F32(2.0 ** -24)
        out[:, c] = lo[c] + u * (hi[c] - lo[c])
    assert out.dtype == F32
    return out


def inside(vertices, faces, query, rule="parity"):
    crossings, winding = brute(vertices, faces, query)
    return (crossings & 1).astype(bool) if rule == "parity" else winding != 0


def common_box(mesh_a, mesh_b):
    """(lo, hi) fp32: the box of the vertices of both meshes"""
    both = np.concatenate([np.asarray(mesh_a[0], F32).reshape(-1, 3), np.asarray(mesh_b[0], F32).reshape(-1, 3)])
    return both.min(0), both.max(0)


def box_volume(lo, hi):
    e = [float(hi[k]) - float(lo[k]) for k in range(3)]
    return (e[0] * e[1]) * e[2]


def volume_iou(mesh_a, mesh_b, n_samples, seed=0, rule="parity"):
    """mesh_metrics.volume_iou: the dict from the reference's containment of the reference's points"""
    lo, hi = common_box(mesh_a, mesh_b)
    p = box_points(n_samples, seed, lo, hi)
    ia, ib = inside(*mesh_a, p, rule), inside(*mesh_b, p, rule)
    counts = [int(ia.sum()), int(ib.sum()), int((ia & ib).sum()), int((ia | ib).sum())]
    scale = box_volume(lo, hi) / n_samples
    out = dict(zip(("volume_a", "volume_b", "intersection", "union"), (c * scale for c in counts)))
    out.update(zip(("count_a", "count_b", "count_intersection", "count_union"), counts))
    out["iou"] = counts[2] / counts[3] if counts[3] else 0.0
    out["n_samples"], out["box"] = n_samples, (lo.tolist(), hi.tolist())
    return out


def volume(vertices, faces):
    """sum of a . (b x c) / 6 in float64"""
    v, f = _mesh(vertices, faces)
    a, b, c = (v[f[:, k]].astype(F64) for k in range(3))
    return float((a * np.cross(b, c)).sum() / 6.0)


# ------------------------------------------------------------------ shared inputs

TRIANGLE = D.TRIANGLE
# (x, y) at z = -1 -> crossings on TRIANGLE: interior, the three edge midpoints, the three corners
TABLE = (((.25, .25), 1), ((.5, 0), 1), ((0, .5), 1), ((.5, .5), 0), ((0, 0), 1), ((1, 0), 0), ((0, 1), 0))
# query -> (crossings, winding) on mesh_raycast_reference.octahedron()
OCTAHEDRON = (((0, 0, 0), (1, 1)), ((0, 0, 2), (0, 0)), ((.5, 0, -2), (2, 0)), ((1, 0, -2), (0, 0)),
              ((0, 1, -2), (2, 0)), ((.5, .5, 0), (1, 1)))

SPHERE_N = 12
SPHERE_H = 2.0 / (SPHERE_N - 1)


@functools.lru_cache(maxsize=None)
def sphere():
    v, f, _ = MS.sphere_mesh(SPHERE_N)
    return v, f


def shifted_sphere():
    v, f = sphere()
    return (v + np.array([0.25, 0.125, 0.0], F32)).astype(F32), f


MESHES = {"sphere12": sphere, "spheres": D.spheres, "soup60": D.soup60, "tiny_face": D.tiny_face_mesh}


def mesh(name):
    return MESHES[name]()


@functools.lru_cache(maxsize=None)
def sphere_queries(seed=12):
    """2528 queries for sphere12: the 1728 lattice nodes (the extractor's own fp32 positions, so that they lie on the
    projections of edges and vertices), 400 vertex columns (the x and y of a vertex, half of them from z = -1, half
    from a random z) and 400 random points of [-1, 1]^3."""
    v, _ = sphere()
    rng = np.random.default_rng(seed)
    h = F32(2.0) / F32(SPHERE_N - 1)
    ax = F32(-1.0) + np.arange(SPHERE_N, dtype=F32) * h
    nodes = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    cols = v[rng.integers(0, len(v), 400)].copy()
    cols[:200, 2] = -1.0
    cols[200:, 2] = rng.uniform(-1, 1, 200)
    q = np.concatenate([nodes, cols, rng.uniform(-1, 1, (400, 3))]).astype(F32)
    assert q.shape == (2528, 3)
    return q


@functools.lru_cache(maxsize=None)
def queries(name, seed=13):
    """The query set of a mesh.  sphere12: sphere_queries.  tiny_face: the queries of the distance tests' cap grid (100
    of them under the large face, below the box) and a lattice under the tiny face, edges and corners included.
    The others: 600 of the distance tests' queries, 200 vertex columns and 200 columns through the fp32 midpoint of an
    edge, from below the box and from a random height."""
    if name == "sphere12":
        return sphere_queries()
    v, f = mesh(name)
    rng = np.random.default_rng(seed)
    if name == "tiny_face":
        k = np.arange(-1, 10, dtype=F64) * 2.0 ** -20
        under = np.stack(np.meshgrid(2 + k, 2 + k, [1.5, 2 - 2.0 ** -18, 2.0], indexing="ij"), -1).reshape(-1, 3)
        return np.concatenate([D.cap_queries(), under]).astype(F32)
    lo, hi = v.min(0), v.max(0)
    cols = v[f[rng.integers(0, len(f), 200), rng.integers(0, 3, 200)]].copy()
    e = f[rng.integers(0, len(f), 200)]
    mids = ((v[e[:, 0]] + v[e[:, 1]]) * F32(0.5)).astype(F32)
    both = np.concatenate([cols, mids])
    both[::2, 2] = lo[2] - F32(0.5)
    both[1::2, 2] = rng.uniform(lo[2], hi[2], len(both[1::2]))
    return np.concatenate([D.queries(name)[:600] if name == "soup60" else _box_queries(v, rng, 600), both]).astype(F32)


def _box_queries(v, rng, n):
    lo, hi = v.min(0), v.max(0)
    pad = 0.1 * (hi - lo).max()
    return rng.uniform(lo - pad, hi + pad, (n, 3))


@functools.lru_cache(maxsize=None)
def brute_of(name):
    return brute(*mesh(name), queries(name))


def grid_cell(name, which):
    """the cell_size of the three grids of the distance tests: one cell, the default, the cap (1024 cells per axis
    for tiny_face, 32 for the others)"""
    v, _ = mesh(name)
    if which == "cap":
        return D.cap_cell(v) if name == "tiny_face" else D.cap_cell(v, 32)
    return {"default": None, "one_cell": D.one_cell(v)}[which]


IOU_N, IOU_SEED = 4096, 0


@functools.lru_cache(maxsize=None)
def iou_reference(which):
    """volume_iou of sphere12 against itself ("self") or against its shifted copy ("shifted"), IOU_N samples"""
    return volume_iou(sphere(), sphere() if which == "self" else shifted_sphere(), IOU_N, IOU_SEED)
