"""Reference for the mesh metrics (a helper, not a test file): the contract of DESIGN §3.11.4 restated in numpy with
its exact integer, float64 and float32 operations in their order, plus the inputs the tests share.

The rules.  rand64(seed, a, b) = mix64(seed 0x9e3779b97f4a7c15 + mix64(a 0xd1b54a32d192ed03 + b)) in uint64, mix64 the
splitmix64 finaliser.  Area: 0.5 sqrt((x x + y y) + z z) of (p1 - p0) x (p2 - p0) in double, every operation rounded on
its own.  CDF: e = 32 - frexp(max area).exponent, w = rint(area 2^e) as int64, cdf = cumsum(w), total = cdf[-1].
Sample i: z_k = rand64(seed, 0x6d657368 + k, i); face = the first f with cdf[f] > umulhi64(z_0, total);
k1 = z_1 >> 40, k2 = z_2 >> 40, both 2^24 - k when k1 + k2 > 2^24; u = k 2^-24;
point = float((p0 + u1 (p1 - p0)) + u2 (p2 - p0)) per axis in double.  Face normal: the cross product divided by its
length in double, rounded once.  Vertex normal: g = ((1 - u1 - u2) n0 + u1 n1) + u2 n2, g / max(|g|, 1e-12).
Nearest neighbour: brute force, d2 = (dx dx + dy dy) + dz dz in fp32, the first index of the smallest d2.
"""
import functools

import numpy as np

import mesh_smooth_reference as MS

F32, F64, U64 = np.float32, np.float64, np.uint64
STREAM = 0x6d657368
MASK32 = U64(0xffffffff)


def mix64(z):
    z = np.asarray(z, U64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U64(30))) * U64(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> U64(27))) * U64(0x94d049bb133111eb)
    return z ^ (z >> U64(31))


def rand64(seed, a, b):
    with np.errstate(over="ignore"):
        return mix64(U64(seed) * U64(0x9e3779b97f4a7c15) + mix64(U64(a) * U64(0xd1b54a32d192ed03) + np.asarray(b, U64)))


def umulhi64(a, b):
    """The high 64 bits of a * b for uint64 arrays, through 32-bit halves (no step overflows)."""
    a, b = np.asarray(a, U64), np.asarray(b, U64)
    al, ah, bl, bh = a & MASK32, a >> U64(32), b & MASK32, b >> U64(32)
    p0, p1, p2, p3 = al * bl, al * bh, ah * bl, ah * bh
    mid = (p0 >> U64(32)) + (p1 & MASK32) + (p2 & MASK32)
    return p3 + (p1 >> U64(32)) + (p2 >> U64(32)) + (mid >> U64(32))


def _mesh(vertices, faces):
    return (np.ascontiguousarray(vertices, F32).reshape(-1, 3).astype(F64), np.asarray(faces, np.int64).reshape(-1, 3))


def face_cross(vertices, faces):
    p, f = _mesh(vertices, faces)
    a, b = p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]]
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _norm(c):
    return np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])


def face_areas(vertices, faces):
    """(F,) float64"""
    return 0.5 * _norm(face_cross(vertices, faces))


def area_cdf(area):
    """(weights (F,) int64, cdf (F,) int64, total int)"""
    area = np.asarray(area, F64)
    if len(area) == 0 or not area.max() > 0:
        return np.zeros(len(area), np.int64), np.zeros(len(area), np.int64), 0
    e = 32 - int(np.frexp(area.max())[1])
    w = np.rint(np.ldexp(area, e)).astype(np.int64)
    cdf = np.cumsum(w)
    return w, cdf, int(cdf[-1])


def sample_surface(vertices, faces, n, seed=0, normals=None, vertex_normals=None):
    """(points (n,3) fp32, face_idx (n,) int32, normals (n,3) fp32 or None, (u1, u2) float64)"""
    p, f = _mesh(vertices, faces)
    _, cdf, total = area_cdf(face_areas(vertices, faces))
    if n and total <= 0:
        raise ValueError("no face has area")
    i = np.arange(n, dtype=U64)
    z0, z1, z2 = (rand64(seed, STREAM + k, i) for k in range(3))
    target = umulhi64(z0, U64(total)).astype(np.int64)
    face = np.searchsorted(cdf, target, side="right")
    k1, k2 = (z1 >> U64(40)).astype(np.int64), (z2 >> U64(40)).astype(np.int64)
    fold = k1 + k2 > 2 ** 24
    k1, k2 = np.where(fold, 2 ** 24 - k1, k1), np.where(fold, 2 ** 24 - k2, k2)
    u1, u2 = k1.astype(F64) * 2.0 ** -24, k2.astype(F64) * 2.0 ** -24
    i0, i1, i2 = (f[face, c] for c in range(3)) if n else (np.zeros(0, np.int64),) * 3
    o = p[i0]
    e1, e2 = p[i1] - o, p[i2] - o
    t1, t2 = u1[:, None] * e1, u2[:, None] * e2
    s = o + t1
    points = (s + t2).astype(F32)
    nrm = None
    if normals == "face":
        g = face_cross(vertices, faces)[face]
        d = _norm(g)
        nrm = (g / np.where(d > 0, d, 1.0)[:, None]).astype(F32)
    elif normals == "vertex":
        vn = np.ascontiguousarray(vertex_normals, F32).reshape(-1, 3).astype(F64)
        w0 = (1.0 - u1) - u2
        g = (w0[:, None] * vn[i0] + u1[:, None] * vn[i1]) + u2[:, None] * vn[i2]
        nrm = (g / np.maximum(_norm(g), 1e-12)[:, None]).astype(F32)
    return points, face.astype(np.int32), nrm, (u1, u2)


def nearest(query, ref, chunk=512):
    """Brute force: (d2 (n,) fp32, idx (n,) int32); argmin returns the first of equal values.  m == 0: +inf, -1."""
    q = np.ascontiguousarray(query, F32).reshape(-1, 3)
    r = np.ascontiguousarray(ref, F32).reshape(-1, 3)
    n, m = len(q), len(r)
    if m == 0:
        return np.full(n, np.inf, F32), np.full(n, -1, np.int32)
    d2, idx = np.empty(n, F32), np.empty(n, np.int32)
    for s in range(0, n, chunk):
        c = q[s:s + chunk]
        dx, dy, dz = (c[:, None, k] - r[None, :, k] for k in range(3))
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == F32
        j = np.argmin(d, 1)
        idx[s:s + chunk] = j
        d2[s:s + chunk] = d[np.arange(len(c)), j]
    return d2, idx


def point_set_metrics(a, b, thresholds=(), normals_a=None, normals_b=None):
    """(the dict of floats, (d2_ab, idx_ab, d2_ba, idx_ba))"""
    d2_ab, idx_ab = nearest(a, b)
    d2_ba, idx_ba = nearest(b, a)
    out = {}
    sides = {}
    for name, d2 in (("a_to_b", d2_ab), ("b_to_a", d2_ba)):
        d2 = d2.astype(F64)
        d = np.sqrt(d2)
        sides[name] = (d, float(d2.mean()))
        out[f"{name}_mean"], out[f"{name}_rms"], out[f"{name}_max"] = float(d.mean()), float(np.sqrt(d2.mean())), float(d.max())
    out["chamfer"] = (out["a_to_b_mean"] + out["b_to_a_mean"]) / 2
    out["chamfer_sq"] = sides["a_to_b"][1] + sides["b_to_a"][1]
    out["hausdorff"] = max(out["a_to_b_max"], out["b_to_a_max"])
    for tau in thresholds:
        tau = float(tau)
        p = float((sides["a_to_b"][0] <= tau).sum()) / len(d2_ab)
        r = float((sides["b_to_a"][0] <= tau).sum()) / len(d2_ba)
        out[f"precision@{tau}"], out[f"recall@{tau}"] = p, r
        out[f"fscore@{tau}"] = 2 * p * r / (p + r) if p + r > 0 else 0.0
    if normals_a is not None:
        na, nb = np.asarray(normals_a, F32).astype(F64), np.asarray(normals_b, F32).astype(F64)
        c_ab = np.abs((na * nb[idx_ab]).sum(1)).mean()
        c_ba = np.abs((nb * na[idx_ba]).sum(1)).mean()
        out["normal_consistency"] = float((c_ab + c_ba) / 2)
    return out, (d2_ab, idx_ab, d2_ba, idx_ba)


def mesh_distance(mesh_a, mesh_b, n_samples, seed=0, thresholds=(), normals=False):
    """mesh_a, mesh_b: (vertices, faces).  The dict of point_set_metrics over the two sample sets."""
    kind = "face" if normals else None
    sa = sample_surface(*mesh_a, n_samples, seed, kind)
    sb = sample_surface(*mesh_b, n_samples, seed, kind)
    return point_set_metrics(sa[0], sb[0], thresholds, sa[2], sb[2])[0]


# ------------------------------------------------------------------ shared inputs


@functools.lru_cache(maxsize=None)
def soup60(seed=11):
    """(vertices (40,3), faces (60,3)): a random soup whose areas span a few orders of magnitude, with 6 faces that
    can never be sampled: 3 with a repeated index, 3 of exactly zero area (collinear corners on a lattice line)."""
    rng = np.random.default_rng(seed)
    v = (rng.uniform(-1, 1, (40, 3)) * rng.choice([0.05, 0.3, 1.0], (40, 1))).astype(F32)
    v[37], v[38], v[39] = (0.25, 0.5, -0.5), (0.5, 0.5, -0.5), (1.0, 0.5, -0.5)  # collinear, exactly
    f = np.stack([rng.permutation(37)[:3] for _ in range(60)]).astype(np.int32)
    f[5], f[17], f[41] = (3, 3, 9), (12, 7, 12), (20, 20, 20)
    f[0], f[30], f[59] = (37, 38, 39), (39, 37, 38), (38, 39, 37)
    return v, f


SOUP_DEAD = (0, 5, 17, 30, 41, 59)


@functools.lru_cache(maxsize=None)
def tiny_face_mesh():
    """Two faces with an area ratio below 2^-33: the small one has weight 0."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 2, 2], [2 + 2.0 ** -17, 2, 2], [2, 2 + 2.0 ** -17, 2]], F32)
    return v, np.array([[3, 4, 5], [0, 1, 2]], np.int32)


@functools.lru_cache(maxsize=None)
def sample_meshes():
    """name -> (vertices, faces, vertex normals): the meshes of the sampling tests."""
    out = {}
    lists = MS.lists()
    for name, (v, f) in (("one_face", lists["triangle"]), ("tiny_face", tiny_face_mesh()), ("soup60", soup60()),
                         ("degenerate", lists["degenerate"]), ("spheres", lists["spheres"])):
        out[name] = (v, f, MS.compute_normals(v, f))
    return out


SAMPLE_N = (0, 1, 63, 64, 65, 257, 4099)
SAMPLE_SEEDS = (0, 0x9e3779b97f4a7c15)


@functools.lru_cache(maxsize=None)
def sampled(name, n, seed, kind):
    v, f, vn = sample_meshes()[name]
    return sample_surface(v, f, n, seed, kind, vn if kind == "vertex" else None)


def _lattice(k=6):
    g = np.arange(k, dtype=F32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def nn_cases():
    """name -> (query (n,3), ref (m,3), cell_size or None)"""
    rng = np.random.default_rng(5)
    out = {}
    out["random3000"] = (rng.uniform(-1, 1, (3000, 3)).astype(F32), rng.uniform(-1, 1, (3000, 3)).astype(F32), None)
    lat = _lattice()
    centres = (_lattice(5) + F32(0.5)).astype(F32)
    q = np.concatenate([centres, lat])
    out["lattice"] = (q, lat, 1.0)  # points on cell faces; 8-way ties at the centres, d2 = 0 on the points
    out["lattice_third"] = (q, lat, 1.0 / 3.0)  # points off the cell faces by rounding only
    a = rng.normal(0, 0.05, (300, 3))
    b = rng.normal(0, 0.05, (300, 3)) + np.array([3.0, 0, 0])
    between = np.stack([np.linspace(0.2, 2.8, 40), rng.uniform(-.2, .2, 40), rng.uniform(-.2, .2, 40)], 1)
    far = rng.uniform(-1, 1, (40, 3)) * 3 + np.array([1.5, 9.0, -7.0])
    out["clusters"] = (np.concatenate([between, far]).astype(F32), np.concatenate([a, b]).astype(F32), 0.1)
    five = rng.uniform(-1, 1, (5, 3)).astype(F32)
    out["duplicates"] = (rng.uniform(-1.5, 1.5, (300, 3)).astype(F32), np.tile(five, (40, 1)), None)
    flat = rng.uniform(-1, 1, (500, 3)).astype(F32)
    flat[:, 2] = F32(0.25)
    out["flat"] = (rng.uniform(-1, 1, (300, 3)).astype(F32), flat, None)
    out["one_cell"] = (rng.uniform(-2, 2, (200, 3)).astype(F32), rng.uniform(-1, 1, (50, 3)).astype(F32), 4.0)
    out["one_cell_equal"] = (rng.uniform(-2, 2, (70, 3)).astype(F32), np.tile(five[:1], (9, 1)), None)
    out["m1"] = (rng.uniform(-2, 2, (100, 3)).astype(F32), five[1:2].copy(), None)
    out["m0"] = (rng.uniform(-2, 2, (10, 3)).astype(F32), np.zeros((0, 3), F32), None)
    out["n0"] = (np.zeros((0, 3), F32), five, None)
    for n in (63, 64, 65, 257):
        out[f"n{n}"] = (rng.uniform(-1, 1, (n, 3)).astype(F32), rng.uniform(-1, 1, (777, 3)).astype(F32), None)
    return out


@functools.lru_cache(maxsize=None)
def nn_reference(name):
    q, r, _ = nn_cases()[name]
    return nearest(q, r)


THRESHOLDS = (0.0, 0.01, 0.05, 0.5)


@functools.lru_cache(maxsize=None)
def metric_sets():
    """(a, b, normals_a, normals_b): two sample sets of the two-sphere list, the second moved a little."""
    v, f, _ = sample_meshes()["spheres"]
    a = sample_surface(v, f, 1500, 1, "face")
    b = sample_surface(v + F32(0.02), f, 1300, 2, "face")
    return a[0], b[0], a[2], b[2]


@functools.lru_cache(maxsize=None)
def metric_reference():
    return point_set_metrics(*metric_sets()[:2], THRESHOLDS, *metric_sets()[2:])[0]


# ------------------------------------------------------------------ the end-to-end case

E2E_SAMPLES = 20000
E2E_CELLS = (0.1, 0.2, 0.4)


def sphere():
    """(vertices, faces) of the 24^3 marching-tetrahedra sphere of the smoothing tests"""
    v, f, _ = MS.sphere_mesh()
    return np.ascontiguousarray(v, F32), np.ascontiguousarray(f, np.int32)
