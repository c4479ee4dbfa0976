"""Reference for the mesh smoothing (a helper, not a test file): the contract of DESIGN §3.11.3 restated in numpy with
its exact float64 operations in their order, plus the triangle lists the tests share.

The rules.  Neighbour adjacency: row v of the CSR pair (row_off (V+1), col (E)), both int32, lists ascending and once
each the vertices u != v that share a face with v; an unused vertex has an empty row.  Boundary vertices: every face
emits the six directed pairs (a,b), (b,a) of its three edges, pairs with a == b are dropped, and boundary[a] = 1 iff
some pair (a,b) occurs exactly once among all emitted pairs.  Vertex-to-face adjacency: row v lists ascending and once
each the faces that contain v.  One pass with the fp32 factor s: for v with neighbours u_0 < ... < u_{d-1}, d > 0, v
not fixed, per axis acc = double(p[u_0]); acc = acc + double(p[u_k]) in that order; m = acc / double(d);
q = double(p[v]); out = float(q + double(s) * (m - q)); with d == 0, v fixed or s == 0, out = p[v] bit for bit.
Normals: g = 0; for the faces f of row v ascending, (i0,i1,i2) = faces[f], a = double(p[i1]) - double(p[i0]),
b = double(p[i2]) - double(p[i0]), g = g + (a x b) with every product and difference rounded on its own;
out = float(g / max(sqrt((gx gx + gy gy) + gz gz), 1e-12)).
"""
import functools

import numpy as np

import mesh_reference as R
import mesh_simplify_reference as S

F32, F64 = np.float32, np.float64
SENTINEL = np.iinfo(np.int64).max


def _faces(faces):
    return np.asarray(faces, np.int64).reshape(-1, 3)


def pair_keys(faces):
    """The 6 F int64 keys (a << 32) | b of the directed pairs, the sentinel where a == b (in no particular order)."""
    f = _faces(faces)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2], f[:, 1], f[:, 2], f[:, 0]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0], f[:, 0], f[:, 1], f[:, 2]])
    return np.where(a == b, SENTINEL, (a << 32) | b)


def vertex_face_keys(faces):
    f = _faces(faces)
    return ((f << 32) | np.arange(len(f), dtype=np.int64)[:, None]).reshape(-1)


def _csr(keys, n_rows):
    """(row_off, col, counts of every distinct key) of the distinct keys that are no sentinel."""
    keys, counts = np.unique(keys[keys != SENTINEL], return_counts=True)
    rows = np.arange(n_rows + 1, dtype=np.int64) << 32
    return (np.searchsorted(keys, rows, side="left").astype(np.int32), (keys & 0xffffffff).astype(np.int32), keys,
            counts)


def adjacency(faces, n_vertices):
    """(row_off (V+1,) int32, col (E,) int32) of the neighbour adjacency."""
    row_off, col, _, _ = _csr(pair_keys(faces), n_vertices)
    return row_off, col


def boundary_vertices(faces, n_vertices):
    """(V,) uint8: 1 iff one of the vertex's directed pairs occurs exactly once."""
    _, _, keys, counts = _csr(pair_keys(faces), n_vertices)
    out = np.zeros(n_vertices, np.uint8)
    out[keys[counts == 1] >> 32] = 1
    return out


def vertex_faces(faces, n_vertices):
    """(row_off (V+1,) int32, col (E,) int32) of the vertex-to-face adjacency."""
    row_off, col, _, _ = _csr(vertex_face_keys(faces), n_vertices)
    return row_off, col


def adjacency_sets(faces, n_vertices):
    """The neighbour sets, from first principles: a list of V Python sets."""
    nb = [set() for _ in range(n_vertices)]
    for a, b, c in _faces(faces).tolist():
        for x, y in ((a, b), (b, c), (c, a)):
            if x != y:
                nb[x].add(y)
                nb[y].add(x)
    return nb


def smooth_pass(vertices, row_off, col, s, fixed=None):
    """One Jacobi pass: (V,3) fp32.  The k-th neighbour of every row is added in the k-th step, so every row is
    summed in its own order, one rounded float64 addition at a time."""
    p = np.ascontiguousarray(vertices, F32).reshape(-1, 3)
    s = F32(s)
    out = p.copy()
    if s == 0 or len(p) == 0:
        return out
    row_off = np.asarray(row_off, np.int64)
    d = row_off[1:] - row_off[:-1]
    move = d > 0
    if fixed is not None:
        move &= ~np.asarray(fixed).astype(bool)
    rows = np.nonzero(move)[0]
    if len(rows) == 0:
        return out
    start, deg = row_off[rows], d[rows]
    p64 = p.astype(F64)
    acc = p64[col[start]]
    for k in range(1, int(deg.max())):
        more = deg > k
        acc[more] = acc[more] + p64[col[start[more] + k]]
    m = acc / deg.astype(F64)[:, None]
    q = p64[rows]
    diff = m - q
    step = F64(s) * diff
    out[rows] = (q + step).astype(F32)
    return out


def vertex_normals(vertices, faces, row_off, col):
    """(V,3) fp32 unit normals from the faces of every vertex, summed in the row's order."""
    p64 = np.ascontiguousarray(vertices, F32).reshape(-1, 3).astype(F64)
    f = _faces(faces)
    V = len(p64)
    a = p64[f[:, 1]] - p64[f[:, 0]]
    b = p64[f[:, 2]] - p64[f[:, 0]]
    cross = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                      a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                      a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1) if len(f) else np.zeros((0, 3))
    row_off = np.asarray(row_off, np.int64)
    d = row_off[1:] - row_off[:-1]
    g = np.zeros((V, 3), F64)
    for k in range(int(d.max()) if V else 0):
        more = np.nonzero(d > k)[0]
        g[more] = g[more] + cross[col[row_off[more] + k]]
    length = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
    return (g / np.maximum(length, 1e-12)[:, None]).astype(F32)


def compute_normals(vertices, faces):
    return vertex_normals(vertices, faces, *vertex_faces(faces, len(vertices)))


def smooth(vertices, faces, iterations=10, lam=0.5, mu=-0.53, fix_boundary=True, fixed=None, normals=False):
    """Mesh.smooth: the smoothed vertices (V,3) fp32, and with ``normals`` also compute_normals of them."""
    p = np.ascontiguousarray(vertices, F32).reshape(-1, 3)
    V = len(p)
    if iterations and V and len(faces):
        row_off, col = adjacency(faces, V)
        fix = None if fixed is None else np.asarray(fixed).astype(bool)
        if fix_boundary:
            b = boundary_vertices(faces, V).astype(bool)
            fix = b if fix is None else fix | b
        for _ in range(iterations):
            for s in (lam,) if mu is None else (lam, mu):
                p = smooth_pass(p, row_off, col, s, fix)
    return (p, compute_normals(p, faces)) if normals else p


# ------------------------------------------------------------------ triangle lists


def fan(n_rim, closed=True, radius=1.0):
    """(vertices, faces): vertex 0 at the origin and n_rim vertices on a circle in the plane z = 0, regularly spaced;
    the triangles (0, i, i+1), counter-clockwise seen from +z; ``closed`` adds (0, n_rim, 1)."""
    t = 2.0 * np.pi * np.arange(n_rim) / n_rim
    v = np.concatenate([np.zeros((1, 3)), np.stack([radius * np.cos(t), radius * np.sin(t), 0 * t], 1)]).astype(F32)
    i = np.arange(1, n_rim + (1 if closed else 0))
    f = np.stack([np.zeros_like(i), i, i % n_rim + 1], 1).astype(np.int32)
    return v, f


def soup(V, seed=0):
    """(vertices, faces): V random vertices and about 4 V random faces, degenerate and duplicated ones among them."""
    rng = np.random.default_rng(3000 * seed + V)
    f = rng.integers(0, V, (max(1, 4 * V), 3)).astype(np.int32)
    return rng.uniform(-1, 1, (V, 3)).astype(F32), f


SOUP_V = (1, 63, 64, 65, 255, 256, 257, 2049)  # across the wave (64), the workgroup (256) and the scan tile (2048)

TETRA = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)  # outward for the vertices below
TETRA_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F32)


def _random_vertices(V, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (V, 3)).astype(F32)


@functools.lru_cache(maxsize=None)
def lists():
    """name -> (vertices (V,3) fp32, faces (F,3) int32): the lists of the adjacency, pass and normal tests."""
    out = {}
    out["triangle"] = (_random_vertices(3, 1), np.array([[0, 1, 2]], np.int32))
    out["two_triangles"] = (_random_vertices(4, 2), np.array([[0, 1, 2], [2, 1, 3]], np.int32))
    out["tetrahedron"] = (TETRA_V.copy(), TETRA.copy())
    out["fan300"] = fan(300)  # the centre's row is longer than a workgroup
    out["fan_open"] = fan(7, closed=False)
    out["unused"] = (_random_vertices(9, 3), np.array([[1, 4, 7], [4, 1, 5], [7, 4, 8]], np.int32))  # 0 2 3 6 unused
    base = np.array([[0, 1, 2], [2, 1, 3], [3, 1, 4]], np.int32)
    out["duplicated_mirrored"] = (_random_vertices(5, 4), np.concatenate([base, base[:2], base[:, [0, 2, 1]]]))
    out["degenerate"] = (_random_vertices(6, 5),
                         np.array([[0, 0, 1], [2, 2, 2], [1, 2, 3], [3, 4, 3], [5, 4, 4], [3, 2, 4]], np.int32))
    out["only_degenerate"] = (_random_vertices(4, 6), np.array([[0, 0, 0], [2, 2, 2], [3, 3, 3], [2, 2, 2]], np.int32))  # E = 0
    for V in SOUP_V:
        out[f"soup{V}"] = soup(V)
    for name in ("spheres", "noise"):
        v, f, _ = S.extracted(name)
        out[name] = (np.ascontiguousarray(v, F32), np.ascontiguousarray(f, np.int32))
    return out


CLEAN_LISTS = ("triangle", "two_triangles", "tetrahedron", "fan300", "fan_open", "unused", "spheres", "noise")
"""the lists without duplicated or degenerate faces and without an edge of more than two faces: there the boundary
vertices are the end points of mesh_reference.boundary_edges"""

PASS_FACTORS = (0.0, 0.5, 1.0, -0.53)


def fixed_mask(V, seed=7):
    return (np.random.default_rng(seed + V).uniform(size=V) < 0.3).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def structure(name):
    """(row_off, col, boundary, face_row_off, face_col) of a list (cached)."""
    v, f = lists()[name]
    return adjacency(f, len(v)) + (boundary_vertices(f, len(v)),) + vertex_faces(f, len(v))


@functools.lru_cache(maxsize=None)
def passed(name, s, with_fixed):
    v, f = lists()[name]
    row_off, col = structure(name)[:2]
    return smooth_pass(v, row_off, col, s, fixed_mask(len(v)) if with_fixed else None)


@functools.lru_cache(maxsize=None)
def normals_of(name):
    v, f = lists()[name]
    return vertex_normals(v, f, *structure(name)[3:])


# ------------------------------------------------------------------ the quality case


QUALITY_N, QUALITY_R0 = 24, 0.6
QUALITY_LO, QUALITY_HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)


@functools.lru_cache(maxsize=None)
def sphere_mesh(n=QUALITY_N):
    """(vertices, faces, grid normals) of the marching-tetrahedra sphere of radius 0.6 on an n^3 lattice over
    [-1,1]^3: closed."""
    shape = (n, n, n)
    return R.marching_tets(R.sphere_field(shape, QUALITY_LO, QUALITY_HI, QUALITY_R0), 0.0, QUALITY_LO, QUALITY_HI,
                           normals=True)


@functools.lru_cache(maxsize=None)
def noisy_sphere(n=QUALITY_N, amplitude=0.3, seed=0):
    """The sphere with every vertex moved along its radius by a normal deviate of ``amplitude`` lattice spacings."""
    v, f, _ = sphere_mesh(n)
    h = 2.0 / (n - 1)
    v64 = np.asarray(v, F64)
    r = np.linalg.norm(v64, axis=1, keepdims=True)
    dr = np.random.default_rng(seed).normal(0.0, amplitude * h, (len(v64), 1))
    return (v64 * (r + dr) / r).astype(F32), f


def radial_rms(vertices):
    """The RMS deviation of |v| from its mean."""
    r = np.linalg.norm(np.asarray(vertices, F64), axis=1)
    return float(np.sqrt(np.mean((r - r.mean()) ** 2)))
