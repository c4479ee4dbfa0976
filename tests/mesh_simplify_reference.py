"""Reference for the mesh simplification by vertex clustering (a helper, not a test file): the contract of DESIGN
§3.11.2 restated in numpy with its exact fp32 / int64 / float64 operations, plus the synthetic inputs the tests share.

The rules.  A grid of cells lo + (ix,iy,iz) cell, dims = (nx,ny,nz); inv = fp32(1) / fp32(cell).  Per axis
t = (v - lo) * inv in fp32 (one subtract, one multiply), i = clamp(floor(t), 0, dim - 1) clamped as a float,
key = (ix ny + iy) nz + iz in int64.  labels[v] = the smallest vertex index with v's key; v is a representative iff
labels[v] == v.  The cluster's vertex, at the representative's row (zeros elsewhere): u = clamp(t - float(i), 0, 1),
q = uint32(u * 2^24), S = the uint64 sum of q over the members, n their number, and
float(double(lo) + (double(i) + double(S) / (double(n) * 2^24)) * double(cell)).  Normals: the int64 sum of
rint(clamp(n, -1, 1) * 2^20), g = double(S) / 2^20, float(g / max(sqrt((gx gx + gy gy) + gz gz), 1e-12)).  Colours:
the uint64 sum of rint(clamp(c, 0, 1) * 2^24), float(double(S) / (double(n) * 2^24)).  clamp(x, a, b) is
x >= a ? (x <= b ? x : b) : a, so a NaN counts as a.  Faces: g = labels[faces]; a face with two equal new indices is
dropped; among the faces with one canonical form (the rotation with the smallest index first) the smallest face index
is kept; a face and its mirror image are different forms.  compact (mesh_clean_reference) then drops what no kept
face uses.
"""
import functools

import numpy as np

import mesh_clean_reference as C

F32, F64 = np.float32, np.float64
Q_POS = F32(16777216.0)
Q_NRM = F32(1048576.0)


def clamp(x, a, b):
    x = np.asarray(x, F32)
    return np.where(x >= F32(a), np.where(x <= F32(b), x, F32(b)), F32(a)).astype(F32)


def grid(lo, cell, dims):
    """(lo (3,) fp32, cell fp32, inv fp32, dims (3,) int64)."""
    cell = F32(cell)
    return np.asarray(lo, F32).reshape(3), cell, F32(1.0) / cell, np.asarray(dims, np.int64).reshape(3)


def cell_indices(vertices, lo, cell, dims):
    """(i (V,3) int64, t (V,3) fp32)."""
    lo, cell, inv, dims = grid(lo, cell, dims)
    v = np.asarray(vertices, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        t = ((v - lo) * inv).astype(F32)
        i = np.stack([clamp(np.floor(t[:, c]), 0.0, F32(dims[c] - 1)) for c in range(3)], 1).astype(np.int64)
    return i, t


def cell_keys(vertices, lo, cell, dims):
    i, _ = cell_indices(vertices, lo, cell, dims)
    dims = np.asarray(dims, np.int64)
    return (i[:, 0] * dims[1] + i[:, 1]) * dims[2] + i[:, 2]


def cluster_labels(vertices, lo, cell, dims):
    """(V,) int32 by a dictionary: the first vertex that shows a key is its smallest index."""
    first = {}
    keys = cell_keys(vertices, lo, cell, dims).tolist()
    return np.array([first.setdefault(k, v) for v, k in enumerate(keys)], np.int32).reshape(-1)


def cluster_labels_sorted(vertices, lo, cell, dims):
    """The same labels, written differently: a stable sort of the keys, the head of every run."""
    keys = cell_keys(vertices, lo, cell, dims)
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    head = np.ones(len(ks), bool)
    head[1:] = ks[1:] != ks[:-1]
    run_first = order[np.maximum.accumulate(np.where(head, np.arange(len(ks)), 0))] if len(ks) else order
    out = np.empty(len(ks), np.int32)
    out[order] = run_first
    return out


def cluster_reduce(vertices, labels, lo, cell, dims, normals=None, colors=None):
    """(vertices, normals or None, colors or None), each (V,3) fp32: the cluster's row at its representative."""
    lo32, cell32, _, _ = grid(lo, cell, dims)
    labels = np.asarray(labels, np.int64)
    V = len(labels)
    i, t = cell_indices(vertices, lo, cell, dims)
    rep = labels == np.arange(V)
    with np.errstate(all="ignore"):
        u = clamp((t - i.astype(F32)).astype(F32), 0.0, 1.0)
    q = (u * Q_POS).astype(F32).astype(np.int64).astype(np.uint64)
    S = np.zeros((V, 3), np.uint64)
    np.add.at(S, labels, q)
    n = np.zeros(V, np.int64)
    np.add.at(n, labels, 1)
    nn = np.where(rep, n, 1).astype(F64)[:, None]
    frac = S.astype(F64) / (nn * 16777216.0)
    pos = (lo32.astype(F64) + (i.astype(F64) + frac) * F64(cell32)).astype(F32)
    out_v = np.where(rep[:, None], pos, F32(0)).astype(F32)
    out_n = out_c = None
    if normals is not None:
        qn = np.rint(clamp(normals, -1.0, 1.0) * Q_NRM).astype(np.int64)
        Sn = np.zeros((V, 3), np.int64)
        np.add.at(Sn, labels, qn)
        g = Sn.astype(F64) / 1048576.0
        length = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        unit = (g / np.maximum(length, 1e-12)[:, None]).astype(F32)
        out_n = np.where(rep[:, None], unit, F32(0)).astype(F32)
    if colors is not None:
        qc = np.rint(clamp(colors, 0.0, 1.0) * Q_POS).astype(np.int64).astype(np.uint64)
        Sc = np.zeros((V, 3), np.uint64)
        np.add.at(Sc, labels, qc)
        mean = (Sc.astype(F64) / (nn * 16777216.0)).astype(F32)
        out_c = np.where(rep[:, None], mean, F32(0)).astype(F32)
    return out_v, out_n, out_c


def canonical(faces):
    """Every face rotated so that its smallest index comes first (the first of equal ones); the cyclic order is kept."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b, c = f[:, 0], f[:, 1], f[:, 2]
    first = (a <= b) & (a <= c)
    second = ~first & (b <= a) & (b <= c)
    rot1, rot2 = f[:, [1, 2, 0]], f[:, [2, 0, 1]]
    return np.where(first[:, None], f, np.where(second[:, None], rot1, rot2))


def cluster_faces(faces, labels):
    """(faces' (F,3) int32 = labels[faces], keep (F,) uint8)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    g = np.asarray(labels, np.int64)[f].reshape(-1, 3)
    ok = (g[:, 0] != g[:, 1]) & (g[:, 1] != g[:, 2]) & (g[:, 0] != g[:, 2])
    keep = np.zeros(len(g), np.uint8)
    seen = set()
    for j, key in enumerate(map(tuple, canonical(g).tolist())):
        if ok[j] and key not in seen:
            seen.add(key)
            keep[j] = 1
    return np.ascontiguousarray(g, np.int32), keep


def simplify_grid(vertices, cell_size, origin=None):
    """(lo, dims) of Mesh.simplify: lo = origin or the vertex minimum, dims = floor((max - lo) * inv) + 1 in fp32
    (at least 1: an origin above the vertices leaves one border cell)."""
    v = np.asarray(vertices, F32).reshape(-1, 3)
    cell = F32(cell_size)
    inv = F32(1.0) / cell
    lo = v.min(0) if origin is None else np.asarray(origin, F32)
    cells = np.floor(((v.max(0) - lo).astype(F32) * inv).astype(F32))
    return lo, [max(1, int(c) + 1) for c in cells]


def simplify(vertices, faces, cell_size, origin=None, normals=None, colors=None):
    """(vertices, faces, normals or None, colors or None) of Mesh.simplify, plus the pieces in a dict."""
    lo, dims = simplify_grid(vertices, cell_size, origin)
    labels = cluster_labels(vertices, lo, cell_size, dims)
    cv, cn, cc = cluster_reduce(vertices, labels, lo, cell_size, dims, normals, colors)
    g, keep = cluster_faces(faces, labels)
    attrs = [a for a in (cn, cc) if a is not None]
    ov, of, out = C.compact(cv, g, keep, attrs)
    out = iter(out)
    info = dict(lo=lo, dims=dims, labels=labels, faces=g, keep=keep, cluster_vertices=cv)
    return ov, of, (None if cn is None else next(out)), (None if cc is None else next(out)), info


def face_stats(faces, labels):
    """(degenerate, duplicate, opposite-orientation pairs among the kept) of a remap, for the record."""
    g, keep = cluster_faces(faces, labels)
    ok = (g[:, 0] != g[:, 1]) & (g[:, 1] != g[:, 2]) & (g[:, 0] != g[:, 2])
    kept = set(map(tuple, canonical(g[keep.astype(bool)]).tolist()))
    pairs = sum(1 for a, b, c in kept if (a, c, b) in kept) // 2
    return int((~ok).sum()), int(ok.sum() - keep.sum()), pairs


# ------------------------------------------------------------------ extracted meshes


def lattice_spacing(name):
    """The smallest lattice spacing of the two extracted meshes of mesh_clean_reference: the unit of their cell sizes."""
    lo, hi, shape = ((C.SPHERES_LO, C.SPHERES_HI, C.SPHERES_SHAPE) if name == "spheres"
                     else (C.BOX_LO, C.BOX_HI, (17, 16, 9)))
    return min((h - l) / (n - 1) for l, h, n in zip(lo, hi, shape))


def extracted(name):
    return C.two_spheres_mesh() if name == "spheres" else C.noise_mesh()


def vertex_colors(n_vertices, seed=11):
    return np.random.default_rng(seed).uniform(0, 1, (n_vertices, 3)).astype(F32)


MESH_CASES = (("spheres", 1.0), ("spheres", 2.0), ("noise", 1.0), ("noise", 1.5), ("noise", 2.0))


@functools.lru_cache(maxsize=None)
def simplified(name, factor, attributes=True):
    """The reference result on an extracted mesh at cell = factor x its smallest lattice spacing (cached)."""
    v, f, n = extracted(name)
    c = vertex_colors(len(v)) if attributes else None
    return simplify(v, f, F32(factor * lattice_spacing(name)), normals=n if attributes else None, colors=c)


# ------------------------------------------------------------------ synthetic vertex sets


SIZES = (1, 63, 64, 65, 255, 256, 257, 2049)  # across the wave (64), the workgroup (256) and the scan tile (2048)
LO, CELL, DIMS = (-1.0, 0.5, 2.0), 0.25, (5, 4, 3)  # a power-of-two cell and exact corners: boundaries are exact


def _points(cells_f):
    """World points of fractional cell coordinates (V,3) on the LO / CELL grid, fp32."""
    return (np.asarray(LO, F64) + np.asarray(cells_f, F64) * CELL).astype(F32)


def vertex_case(kind, V, seed=0):
    """(vertices (V,3) fp32, lo, cell, dims) of a synthetic labelling input."""
    rng = np.random.default_rng(1000 * seed + V)
    if kind == "one_cell":  # every vertex in cell (2,1,1)
        return _points(np.array([2, 1, 1]) + rng.uniform(0.05, 0.95, (V, 3))), LO, CELL, DIMS
    if kind == "own_cell":  # vertex j alone in a cell, the cells taken in shuffled order
        dims = (-(-V // 12), 4, 3)
        cells = rng.permutation(dims[0] * 12)[:V]
        ijk = np.stack([cells // 12, cells // 3 % 4, cells % 3], 1)
        return _points(ijk + rng.uniform(0.1, 0.9, (V, 3))), LO, CELL, dims
    if kind == "random":  # uniform over the 5 x 4 x 3 grid, in no order
        return _points(rng.uniform(0, 1, (V, 3)) * np.array(DIMS)), LO, CELL, DIMS
    if kind == "boundaries":  # every coordinate exactly on a cell boundary, the upper face of the grid included
        return _points(np.stack([rng.integers(0, d + 1, V) for d in DIMS], 1)), LO, CELL, DIMS
    if kind == "outside":  # up to three cells outside the grid on both sides of every axis
        return _points(rng.uniform(-3, 1, (V, 3)) * np.array(DIMS) + rng.integers(0, 2, (V, 3)) * 3 * np.array(DIMS)), \
            LO, CELL, DIMS
    if kind == "flat_axis":  # one cell along y, whatever y is
        p = _points(rng.uniform(0, 1, (V, 3)) * np.array(DIMS))
        p[:, 1] = rng.uniform(-50, 50, V).astype(F32)
        return p, LO, CELL, (5, 1, 3)
    raise ValueError(kind)


VERTEX_KINDS = ("one_cell", "own_cell", "random", "boundaries", "outside", "flat_axis")


def attribute_case(V, seed=5):
    """(normals, colors) (V,3) fp32 for the random vertex set: unit normals and colours slightly outside [0,1], one
    NaN colour and one NaN normal component."""
    rng = np.random.default_rng(seed)
    n = rng.normal(size=(V, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F32)
    c = rng.uniform(-0.1, 1.1, (V, 3)).astype(F32)
    c[V // 2, 1] = np.nan
    n[V // 3, 2] = np.nan
    return n, c


def cancelling_normals():
    """(vertices, normals, lo, cell, dims): cell (0,0,0) holds two vertices with opposite normals (their sum is zero),
    cell (1,0,0) two with equal ones."""
    v = _points(np.array([[0.2, 0.3, 0.4], [0.7, 0.6, 0.5], [1.2, 0.3, 0.4], [1.7, 0.6, 0.5]]))
    n = np.array([[0.6, 0.0, 0.8], [-0.6, 0.0, -0.8], [0.0, 1.0, 0.0], [0.0, 1.0, 0.0]], F32)
    return v, n, LO, CELL, DIMS


# ------------------------------------------------------------------ synthetic face lists


def face_case(kind, F, seed=0):
    """(faces (F,3) int32, labels (V,) int32) of a synthetic remapping input."""
    rng = np.random.default_rng(2000 * seed + F)
    i = np.arange(F, dtype=np.int64)
    if kind == "strip_partial":  # a strip whose first half is clustered in pairs (it collapses), the rest untouched
        V = F + 2
        labels = np.arange(V)
        half = (V // 2) // 2 * 2
        labels[:half] = labels[:half] // 2 * 2
        return np.stack([i, i + 1, i + 2], 1).astype(np.int32), labels.astype(np.int32)
    if kind == "strip_distinct":  # F different faces: with the minimal table the load factor is F / 2^k
        return np.stack([i, i + 1, i + 2], 1).astype(np.int32), np.arange(F + 2, dtype=np.int32)
    if kind == "rotations":  # F copies of one triangle, in its three rotations
        tri = np.array([[3, 7, 5], [7, 5, 3], [5, 3, 7]])
        return tri[i % 3].astype(np.int32), np.arange(8, dtype=np.int32)
    if kind == "opposite":  # even faces: rotations of (0,1,2); odd faces: rotations of its mirror image (0,2,1)
        a = np.array([[0, 1, 2], [1, 2, 0], [2, 0, 1]])
        b = np.array([[0, 2, 1], [2, 1, 0], [1, 0, 2]])
        return np.where((i % 2 == 0)[:, None], a[i // 2 % 3], b[i // 2 % 3]).astype(np.int32), np.arange(3, dtype=np.int32)
    if kind == "degenerate":  # (a,a,b), (a,a,a) and faces that two clustered vertices collapse, between good faces
        V = 40
        labels = np.arange(V)
        labels[1::4] -= 1  # vertex 4k+1 joins vertex 4k
        f = np.stack([rng.integers(0, V, F), rng.integers(0, V, F), rng.integers(0, V, F)], 1)
        f[1::5, 1] = f[1::5, 0]
        f[3::7] = f[3::7, :1]
        a = f[2::6, 0] // 4 * 4  # (4k, x, 4k+1): three different indices before the remap, two equal after it
        f[2::6, 0], f[2::6, 2] = a, a + 1
        return f.astype(np.int32), labels.astype(np.int32)
    raise ValueError(kind)


FACE_KINDS = ("strip_partial", "strip_distinct", "rotations", "opposite", "degenerate")
