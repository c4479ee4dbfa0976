"""Reference for the quadric-error placement of the vertex clustering (a helper, not a test file): the contract of
DESIGN §3.11.2 ("Quadric placement") restated in numpy, plus the inputs the tests share.

Every float64 operation below is one elementwise numpy operation, so each rounds on its own, in the order in which
csrc/mesh_quadric_core.hpp performs it: no ``@``, ``dot`` or ``einsum``.  The arrays run over the clusters (one element
per representative), never over the terms of a sum: the faces of a row are added one after the other, in the row's
order.

The rules.  For every representative r (labels[r] == r): (ix,iy,iz) = the cell of vertices[r] (cell_indices of
mesh_simplify_reference), c = double(lo) + (double(i) + 0.5) * double(cell), local coordinates
y = (double(p) - c) / double(cell).  A = 0 (a00 a01 a02 a11 a12 a22), b = 0; for the faces of row r of the
vertex-to-face adjacency of labels[faces], ascending, with local corners a, b1, c1: u = b1 - a, w = c1 - a,
n = (u1 w2 - u2 w1, u2 w0 - u0 w2, u0 w1 - u1 w0), L = sqrt((nx nx + ny ny) + nz nz), skipped unless L > 0, m = n / L,
d = -((mx ax + my ay) + mz az), A_ij = A_ij + L * (m_i * m_j), b_i = b_i + (L * d) * m_i.  Eight cyclic Jacobi sweeps
over the pairs (0,1), (0,2), (1,2) (``rotate`` below), eigenvalues l_i = the diagonal, eigenvectors the columns e_i.
xbar = the local coordinates of mean[r]; lmax = max |l_i|; the mean is kept unless lmax > 0.
g_i = -b_i - ((A_i0 xbar_0 + A_i1 xbar_1) + A_i2 xbar_2); x = xbar; for i = 0, 1, 2, if l_i > tol * lmax:
k = ((e_0i g_0 + e_1i g_1) + e_2i g_2) / l_i, x_j = x_j + k * e_ji.  The mean is kept unless every x_j is in
[-0.5, 0.5] (a NaN is not).  position[r] = float(c + x * double(cell)) where x was accepted (placed[r] = 1), the bits
of mean[r] at the other representatives, zeros elsewhere.
"""
import functools

import numpy as np

import mesh_clean_reference as C
import mesh_simplify_reference as S
import mesh_smooth_reference as M

F32, F64 = np.float32, np.float64
SWEEPS = 8
TOL = 1e-3


def _f64(x):
    return np.asarray(x, F64)


def face_terms(a, b, c):
    """(ok (n,), dA (n,6), db (n,3)) of faces with local corners a, b, c (n,3) float64."""
    a, b, c = _f64(a), _f64(b), _f64(c)
    with np.errstate(all="ignore"):
        u0, u1, u2 = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1], b[:, 2] - a[:, 2]
        w0, w1, w2 = c[:, 0] - a[:, 0], c[:, 1] - a[:, 1], c[:, 2] - a[:, 2]
        x0, x1 = u1 * w2, u2 * w1
        y0, y1 = u2 * w0, u0 * w2
        z0, z1 = u0 * w1, u1 * w0
        nx, ny, nz = x0 - x1, y0 - y1, z0 - z1
        xx, yy, zz = nx * nx, ny * ny, nz * nz
        L = np.sqrt((xx + yy) + zz)
        ok = L > 0.0
        mx, my, mz = nx / L, ny / L, nz / L
        dx, dy, dz = mx * a[:, 0], my * a[:, 1], mz * a[:, 2]
        d = -((dx + dy) + dz)
        dA = np.stack([L * (mx * mx), L * (mx * my), L * (mx * mz), L * (my * my), L * (my * mz), L * (mz * mz)], 1)
        Ld = L * d
        db = np.stack([Ld * mx, Ld * my, Ld * mz], 1)
    return ok, dA, db


def rotate(app, aqq, apq, arp, arq, vp, vq):
    """One Jacobi rotation of the pair (p, q), r the third index; vp, vq the columns p and q of the eigenvectors as
    lists of three arrays.  Returns the new (app, aqq, apq, arp, arq, vp, vq); a pair with apq == 0 is left alone."""
    with np.errstate(all="ignore"):
        skip = apq == 0.0
        diff = aqq - app
        twice = 2.0 * apq
        theta = diff / twice
        th2 = theta * theta
        root = np.sqrt(th2 + 1.0)
        den = np.abs(theta) + root
        tp = 1.0 / den
        t = np.where(theta < 0.0, -tp, tp)
        t2 = t * t
        c = 1.0 / np.sqrt(t2 + 1.0)
        s = t * c
        h = t * apq
        n_app = app - h
        n_aqq = aqq + h
        n_arp = c * arp - s * arq
        n_arq = s * arp + c * arq
        n_vp = [c * vp[k] - s * vq[k] for k in range(3)]
        n_vq = [s * vp[k] + c * vq[k] for k in range(3)]
    keep = lambda old, new: np.where(skip, old, new)
    return (keep(app, n_app), keep(aqq, n_aqq), keep(apq, np.zeros_like(apq)), keep(arp, n_arp), keep(arq, n_arq),
            [keep(vp[k], n_vp[k]) for k in range(3)], [keep(vq[k], n_vq[k]) for k in range(3)])


def jacobi(A6):
    """Eigenpairs of the symmetric matrices A6 (n,6) = a00 a01 a02 a11 a12 a22: (lam (n,3), E (n,3,3)) with
    E[:, j, i] = component j of eigenvector i."""
    A6 = _f64(A6).reshape(-1, 6)
    a00, a01, a02, a11, a12, a22 = (A6[:, k].copy() for k in range(6))
    n = len(A6)
    one, zero = np.ones(n), np.zeros(n)
    v0, v1, v2 = [one, zero, zero], [zero, one, zero], [zero, zero, one]  # the columns
    for _ in range(SWEEPS):
        a00, a11, a01, a02, a12, v0, v1 = rotate(a00, a11, a01, a02, a12, v0, v1)
        a00, a22, a02, a01, a12, v0, v2 = rotate(a00, a22, a02, a01, a12, v0, v2)
        a11, a22, a12, a01, a02, v1, v2 = rotate(a11, a22, a12, a01, a02, v1, v2)
    lam = np.stack([a00, a11, a22], 1)
    E = np.stack([np.stack([v0[j], v1[j], v2[j]], 1) for j in range(3)], 1)
    return lam, E


def jacobi_matrix(A):
    """(lam (3,), E (3,3), columns the eigenvectors) of one symmetric 3x3 matrix."""
    A = _f64(A)
    lam, E = jacobi([[A[0, 0], A[0, 1], A[0, 2], A[1, 1], A[1, 2], A[2, 2]]])
    return lam[0], E[0]


def solve(A6, b3, xbar, tol=TOL):
    """(x (n,3), placed (n,) bool, rank (n,)) from the quadrics A6 (n,6), b3 (n,3) and the local means xbar (n,3)."""
    A6, b3, xbar = _f64(A6).reshape(-1, 6), _f64(b3).reshape(-1, 3), _f64(xbar).reshape(-1, 3)
    lam, E = jacobi(A6)
    with np.errstate(all="ignore"):
        m = np.abs(lam)
        lmax = m[:, 0]
        lmax = np.where(m[:, 1] > lmax, m[:, 1], lmax)
        lmax = np.where(m[:, 2] > lmax, m[:, 2], lmax)
        some = lmax > 0.0
        rows = ((0, 1, 2), (1, 3, 4), (2, 4, 5))
        g = []
        for i in range(3):
            r0, r1, r2 = (A6[:, rows[i][j]] * xbar[:, j] for j in range(3))
            g.append(-b3[:, i] - ((r0 + r1) + r2))
        cut = F64(tol) * lmax
        x = [xbar[:, j].copy() for j in range(3)]
        rank = np.zeros(len(A6), np.int64)
        for i in range(3):
            on = lam[:, i] > cut
            p0, p1, p2 = (E[:, j, i] * g[j] for j in range(3))
            k = ((p0 + p1) + p2) / lam[:, i]
            x = [np.where(on, x[j] + k * E[:, j, i], x[j]) for j in range(3)]
            rank += on
        x = np.stack(x, 1)
        inside = ((x >= -0.5) & (x <= 0.5)).all(1)
    return x, some & inside, np.where(some, rank, 0)


def cluster_quadric(vertices, faces, labels, row_off, col, mean, lo, cell, dims, tol=TOL, return_info=False):
    """(position (V,3) fp32, placed (V,) uint8) of kernels.mesh_cluster_quadric; with ``return_info`` also a dict with
    the representatives and, per representative, the rank used (0 where no eigenvalue is positive) and A, b."""
    lo32, cell32, _, _ = S.grid(lo, cell, dims)
    v = np.asarray(vertices, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    labels = np.asarray(labels, np.int64)
    row_off, col = np.asarray(row_off, np.int64), np.asarray(col, np.int64)
    mean = np.asarray(mean, F32).reshape(-1, 3)
    V = len(v)
    reps = np.flatnonzero(labels == np.arange(V))
    i, _ = S.cell_indices(v, lo, cell, dims)
    cd = F64(cell32)
    centre = lo32.astype(F64) + (i[reps].astype(F64) + 0.5) * cd
    xbar = (mean[reps].astype(F64) - centre) / cd
    start, length = row_off[reps], row_off[reps + 1] - row_off[reps]
    A, b = np.zeros((len(reps), 6)), np.zeros((len(reps), 3))
    for k in range(int(length.max()) if len(reps) else 0):  # the k-th face of every row that has one
        sel = np.flatnonzero(length > k)
        fk = f[col[start[sel] + k]]
        c = centre[sel]
        ok, dA, db = face_terms(*[(v[fk[:, j]].astype(F64) - c) / cd for j in range(3)])
        A[sel] = np.where(ok[:, None], A[sel] + dA, A[sel])
        b[sel] = np.where(ok[:, None], b[sel] + db, b[sel])
    x, placed, rank = solve(A, b, xbar, tol)
    position = np.zeros((V, 3), F32)
    with np.errstate(all="ignore"):
        moved = (centre + x * cd).astype(F32)
    position[reps] = np.where(placed[:, None], moved, mean[reps])
    flag = np.zeros(V, np.uint8)
    flag[reps] = placed
    if return_info:
        return position, flag, dict(reps=reps, rank=rank, A=A, b=b, rows=length)
    return position, flag


def cluster_rows(faces, labels):
    """The CSR pair the placement reads: the vertex-to-face adjacency of labels[faces]."""
    g, _ = S.cluster_faces(faces, labels)
    return M.vertex_faces(g, len(labels))


def simplify(vertices, faces, cell_size, origin=None, normals=None, colors=None, placement="quadric", tol=TOL):
    """(vertices, faces, normals or None, colors or None, info) of Mesh.simplify(placement=...)."""
    if placement == "mean":
        return S.simplify(vertices, faces, cell_size, origin, normals, colors)
    lo, dims = S.simplify_grid(vertices, cell_size, origin)
    labels = S.cluster_labels(vertices, lo, cell_size, dims)
    cv, cn, cc = S.cluster_reduce(vertices, labels, lo, cell_size, dims, normals, colors)
    g, keep = S.cluster_faces(faces, labels)
    row_off, col = M.vertex_faces(g, len(labels))
    pos, placed, q = cluster_quadric(vertices, faces, labels, row_off, col, cv, lo, cell_size, dims, tol, True)
    attrs = [a for a in (cn, cc) if a is not None]
    ov, of, out = C.compact(pos, g, keep, attrs)
    out = iter(out)
    info = dict(lo=lo, dims=dims, labels=labels, faces=g, keep=keep, cluster_vertices=cv, position=pos, placed=placed,
                row_off=row_off, col=col, rank=q["rank"], reps=q["reps"])
    return ov, of, (None if cn is None else next(out)), (None if cc is None else next(out)), info


def used_fallbacks(info):
    """The clusters a kept face uses that kept the mean."""
    used = np.zeros(len(info["labels"]), bool)
    used[info["faces"][info["keep"].astype(bool)].reshape(-1)] = True
    return int((used & (info["placed"] == 0)).sum()), int(used.sum())


@functools.lru_cache(maxsize=None)
def simplified(name, factor, attributes=True):
    """The quadric result on an extracted mesh of mesh_simplify_reference (cached)."""
    v, f, n = S.extracted(name)
    c = S.vertex_colors(len(v)) if attributes else None
    return simplify(v, f, F32(factor * S.lattice_spacing(name)), normals=n if attributes else None, colors=c)


# ------------------------------------------------------------------ measures


def volume(vertices, faces):
    """The divergence volume in double: the sum of a . (b x c) / 6 over the faces."""
    p = np.asarray(vertices, F64)[np.asarray(faces, np.int64).reshape(-1, 3)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def cube_surface_distance(points):
    """The distance of every point to the surface of the unit cube [0,1]^3, in double."""
    q = np.abs(np.asarray(points, F64) - 0.5) - 0.5  # per axis: > 0 outside, < 0 inside
    outside = np.sqrt((np.maximum(q, 0.0) ** 2).sum(1))
    return np.where(outside > 0.0, outside, -q.max(1))


# ------------------------------------------------------------------ the shared inputs

CUBE_N = 12
CUBE_CELL = F32(2.5 / CUBE_N)


@functools.lru_cache(maxsize=None)
def cube_mesh(n=CUBE_N):
    """(vertices, faces) of the unit cube [0,1]^3 with n x n quads per side, two triangles each, wound outwards:
    V = (n+1)^3 - (n-1)^3, F = 12 n^2."""
    index = {}

    def at(i, j, k):
        return index.setdefault((i, j, k), len(index))

    faces = []
    for axis in range(3):
        for side in (0, n):
            for p in range(n):
                for q in range(n):
                    corner = []
                    for dp, dq in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        ijk = [0, 0, 0]
                        ijk[axis], ijk[(axis + 1) % 3], ijk[(axis + 2) % 3] = side, p + dp, q + dq
                        corner.append(at(*ijk))
                    a, b, c, d = corner if side else corner[::-1]  # (axis+1) x (axis+2) = +axis: outwards at side n
                    faces += [(a, b, c), (a, c, d)]
    v = (np.array(sorted(index, key=index.get), F64) / n).astype(F32)
    return v, np.array(faces, np.int32)


def cube_case():
    """(vertices, faces, cell, origin): the cube, cell 2.5 / 12, the grid's corner 0.4 cells below the cube's."""
    v, f = cube_mesh()
    return v, f, CUBE_CELL, np.full(3, F32(-0.4) * CUBE_CELL, F32)


CUBE_CORNERS = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], F64)


@functools.lru_cache(maxsize=None)
def sphere_mesh(segments=64, rings=32, radius=1.0):
    """(vertices, faces) of a latitude / longitude sphere, closed and wound outwards: V = 2 + (rings - 1) segments."""
    v = [(0.0, 0.0, radius)]
    for i in range(1, rings):
        th = np.pi * i / rings
        for j in range(segments):
            ph = 2.0 * np.pi * j / segments
            v.append((radius * np.sin(th) * np.cos(ph), radius * np.sin(th) * np.sin(ph), radius * np.cos(th)))
    v.append((0.0, 0.0, -radius))
    last = len(v) - 1
    at = lambda i, j: 1 + (i - 1) * segments + j % segments
    f = []
    for j in range(segments):
        f.append((0, at(1, j), at(1, j + 1)))
        f.append((last, at(rings - 1, j + 1), at(rings - 1, j)))
        for i in range(1, rings - 1):
            f.append((at(i, j), at(i + 1, j), at(i + 1, j + 1)))
            f.append((at(i, j), at(i + 1, j + 1), at(i, j + 1)))
    return np.array(v, F64).astype(F32), np.array(f, np.int32)


SPHERE_CELLS = (0.2, 0.3)
SPHERE_VOLUME = 4.0 * np.pi / 3.0


# the matrix families of the Jacobi checks: (name, symmetric 3x3 float64)
def matrix_cases(seed=0, n_random=40):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n_random):
        B = rng.normal(size=(3, 3)) * 10.0 ** rng.integers(-3, 4)
        out.append((f"random{k}", (B + B.T) / 2.0))
    for k in range(10):
        u, w = rng.normal(size=3), rng.normal(size=3)
        out.append((f"rank1_{k}", np.outer(u, u)))
        out.append((f"rank2_{k}", np.outer(u, u) + np.outer(w, w)))
    out.append(("diagonal", np.diag([3.0, -1.0, 0.5])))
    out.append(("identity", np.eye(3)))
    out.append(("zero", np.zeros((3, 3))))
    out.append(("axis_plane", np.diag([0.0, 0.0, 7.0])))
    out.append(("tiny_offdiagonal", np.array([[1.0, 1e-200, 0.0], [1e-200, 2.0, 0.0], [0.0, 0.0, 3.0]])))
    return out
