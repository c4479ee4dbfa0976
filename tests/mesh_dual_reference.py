"""Reference for dual contouring (a helper, not a test file): the rule of DESIGN §3.11.11 restated in numpy and plain
Python loops, operation by operation, plus the fields with exact Hermite data that the dual tests share.

The rule.  Lattice, box, inside iff field > iso and p = (ix ny + iy) nz + iz as in mesh_reference.  Point p owns the
axis edges p -> p + e_a, a = 0,1,2, that stay in the lattice; an owned edge whose ends differ crosses and carries
marching tetrahedra's vertex pa + t (pb - pa), t = (f[p] - iso) / (f[p] - f[q]) and its grid normal, all fp32, and the
key 3 p + a.  Edges are ordered by (p, a).  The cell with low corner p is active iff its 8 inside bits are mixed; cells
are ordered by p.  Its edges are taken in the order a = 0,1,2, (b,c) = ((a+1)%3, (a+2)%3), (ob,oc) = (0,0), (1,0),
(0,1), (1,1), the edge being owned by p + ob e_b + oc e_c.  Every crossing edge's point goes to
y_k = (double(x_k) - double(pa_k)) / double(h_k) - 0.5, pa_k = lo_k + float(i_k) h_k in fp32; xbar = their sum in that
order over their number.  "mean": x = xbar.  "qef": every crossing edge adds m_k = double(n_k) double(h_k),
L = sqrt((m0 m0 + m1 m1) + m2 m2), skipped unless L > 0, u = m / L, d = -((u0 y0 + u1 y1) + u2 y2),
A_ij = A_ij + u_i u_j, b_i = b_i + d u_i; x = mesh_quadric_reference.solve(A, b, xbar, tol), and xbar (fallback = 1)
where that is rejected.  vertex = pa_k + float(x_k + 0.5) h_k in fp32.  The vertex normal is the double sum s of the
edge normals in order, float(s / max(|s|, 1e-12)).  A crossing edge (p, a) is interior iff 1 <= j_b <= n_b - 2 and
1 <= j_c <= n_c - 2; it gives the quad over the cells k0 = p - e_b - e_c, k1 = p - e_c, k2 = p, k3 = p - e_b, kept when
p is inside and reversed to k0 k3 k2 k1 otherwise, split into (v0,v1,v2), (v0,v2,v3).  Faces are ordered by (p, a).

Python floats are IEEE doubles and every expression below is one operation per rounding, so the doubles agree with
csrc/mesh_dual_core.hpp (built with -ffp-contract=off) bit for bit; the solve and its Jacobi are the ones of
mesh_quadric_reference.

``variant`` breaks the rule on purpose, for the tests that show the checks have teeth: "reversed" swaps the quad
order, "no_boundary" drops the interior test (the missing cells of a border edge are clamped to the existing ones) and
"no_h" leaves the spacing out of the local normal.
"""
import functools
import math

import numpy as np

import mesh_quadric_reference as Q
import mesh_reference as M

F32, F64 = np.float32, np.float64
TOL = 1e-3
ORDER = tuple((a, ob, oc) for a in range(3) for ob, oc in ((0, 0), (1, 0), (0, 1), (1, 1)))


def _unit(a):
    return tuple(1 if k == a else 0 for k in range(3))


def _add(i, d, s=1):
    return (i[0] + s * d[0], i[1] + s * d[1], i[2] + s * d[2])


def hermite(field, iso, lo, hi):
    """The crossing edges of the lattice: dict with keys (E,) int32, points (E,3) and normals (E,3) fp32 and
    index {(i, a): e}."""
    f = np.ascontiguousarray(field, F32)
    n = f.shape
    iso = F32(iso)
    lo = np.asarray(lo, F32)
    h = M.spacing(n, lo, hi)
    inside = f > iso
    grad = M.grid_gradient(f, h)
    index, keys, points, normals = {}, [], [], []
    for ix in range(n[0]):
        for iy in range(n[1]):
            for iz in range(n[2]):
                i = (ix, iy, iz)
                for a in range(3):
                    j = _add(i, _unit(a))
                    if j[a] >= n[a] or inside[i] == inside[j]:
                        continue
                    t = (f[i] - iso) / (f[i] - f[j])
                    v = np.zeros(3, F32)
                    for k in range(3):
                        pa = lo[k] + F32(i[k]) * h[k]
                        pb = lo[k] + F32(j[k]) * h[k]
                        v[k] = pa + t * (pb - pa)
                    g = grad[i] + t * (grad[j] - grad[i])
                    ln = F32(np.sqrt(np.sum(g * g, dtype=F32)))
                    index[(i, a)] = len(keys)
                    keys.append(3 * ((ix * n[1] + iy) * n[2] + iz) + a)
                    points.append(v)
                    normals.append(-g / max(ln, F32(1e-12)))
    return dict(keys=np.array(keys, np.int32), points=np.array(points, F32).reshape(-1, 3),
                normals=np.array(normals, F32).reshape(-1, 3), index=index)


def dual_contour(field, iso, lo, hi, placement="qef", tol=TOL, points=None, normals=None, variant=None):
    """The whole rule.  points / normals (E,3) replace the grid's Hermite data.  Returns a dict: E, V, F, keys, points,
    normals, verts (V,3) fp32, faces (F,3) int32, vertex_normals (V,3) fp32, fallback (V,) uint8, cells (V,3) int (the
    low corner of every vertex's cell) and interior (the number of interior crossing edges, counted on its own)."""
    assert placement in ("qef", "mean") and variant in (None, "reversed", "no_boundary", "no_h")
    f = np.ascontiguousarray(field, F32)
    n = f.shape
    lo32 = np.asarray(lo, F32)
    h = M.spacing(n, lo32, hi)
    inside = f > F32(iso)
    H = hermite(f, iso, lo, hi)
    index, E = H["index"], len(H["keys"])
    pts = H["points"] if points is None else np.asarray(points, F32).reshape(E, 3)
    nrm = H["normals"] if normals is None else np.asarray(normals, F32).reshape(E, 3)
    hd = [float(h[k]) for k in range(3)]

    cell_index, cells, xbars, A6, b3, vnorm = {}, [], [], [], [], []
    for ix in range(n[0] - 1):
        for iy in range(n[1] - 1):
            for iz in range(n[2] - 1):
                i = (ix, iy, iz)
                bits = [bool(inside[ix + (c & 1), iy + ((c >> 1) & 1), iz + ((c >> 2) & 1)]) for c in range(8)]
                if all(bits) or not any(bits):
                    continue
                pa = [lo32[k] + F32(i[k]) * h[k] for k in range(3)]
                count, ysum, s = 0, [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
                A, b = [0.0] * 6, [0.0] * 3
                for a, ob, oc in ORDER:
                    owner = _add(_add(i, _unit((a + 1) % 3), ob), _unit((a + 2) % 3), oc)
                    e = index.get((owner, a))
                    if e is None:
                        continue
                    y = [(float(pts[e, k]) - float(pa[k])) / hd[k] - 0.5 for k in range(3)]
                    count += 1
                    ysum = [ysum[k] + y[k] for k in range(3)]
                    nk = [float(nrm[e, k]) for k in range(3)]
                    s = [s[k] + nk[k] for k in range(3)]
                    m = nk if variant == "no_h" else [nk[k] * hd[k] for k in range(3)]
                    L = math.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
                    if not L > 0.0:
                        continue
                    u = [m[k] / L for k in range(3)]
                    d = -((u[0] * y[0] + u[1] * y[1]) + u[2] * y[2])
                    for slot, (p, q) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
                        A[slot] = A[slot] + u[p] * u[q]
                    b = [b[k] + d * u[k] for k in range(3)]
                cell_index[i] = len(cells)
                cells.append(i)
                xbars.append([ysum[k] / float(count) for k in range(3)])
                A6.append(A)
                b3.append(b)
                ln = math.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
                den = ln if ln > 1e-12 else 1e-12
                vnorm.append([s[k] / den for k in range(3)])
    V = len(cells)
    xbar = np.array(xbars, F64).reshape(V, 3)
    x, fallback = xbar, np.zeros(V, np.uint8)
    if placement == "qef" and V:
        xs, placed, _ = Q.solve(np.array(A6, F64), np.array(b3, F64), xbar, tol)
        x = np.where(placed[:, None], xs, xbar)
        fallback = (~placed).astype(np.uint8)
    verts = np.zeros((V, 3), F32)
    for v, i in enumerate(cells):
        for k in range(3):
            verts[v, k] = (lo32[k] + F32(i[k]) * h[k]) + F32(x[v, k] + 0.5) * h[k]

    faces, interior = [], 0
    for ix in range(n[0]):
        for iy in range(n[1]):
            for iz in range(n[2]):
                i = (ix, iy, iz)
                for a in range(3):
                    if (i, a) not in index:
                        continue
                    b_, c_ = (a + 1) % 3, (a + 2) % 3
                    inner = 1 <= i[b_] <= n[b_] - 2 and 1 <= i[c_] <= n[c_] - 2
                    interior += inner
                    if not inner and variant != "no_boundary":
                        continue
                    eb, ec = _unit(b_), _unit(c_)
                    ks = [_add(_add(i, eb, -1), ec, -1), _add(i, ec, -1), i, _add(i, eb, -1)]
                    ks = [tuple(min(max(k[d], 0), n[d] - 2) for d in range(3)) for k in ks]  # no_boundary only
                    v0, v1, v2, v3 = (cell_index[k] for k in ks)
                    if bool(inside[i]) == (variant == "reversed"):
                        v1, v3 = v3, v1
                    faces += [(v0, v1, v2), (v0, v2, v3)]
    return dict(E=E, V=V, F=len(faces), keys=H["keys"], points=pts, normals=nrm, verts=verts,
                faces=np.array(faces, np.int32).reshape(-1, 3), vertex_normals=np.array(vnorm, F64).astype(F32).reshape(V, 3),
                fallback=fallback, cells=np.array(cells, np.int64).reshape(V, 3), interior=int(interior))


def tets_axis_vertices(field, iso, lo, hi):
    """The marching_tets vertices on the axis edges, in the order (p, a): (E,3) fp32."""
    f = np.ascontiguousarray(field, F32)
    n = f.shape
    inside = f > F32(iso)
    verts = M.marching_tets(f, iso, lo, hi)[0]
    pick, count = [], 0
    for ix in range(n[0]):
        for iy in range(n[1]):
            for iz in range(n[2]):
                for d in range(1, 8):
                    j = (ix + (d & 1), iy + ((d >> 1) & 1), iz + ((d >> 2) & 1))
                    if j[0] >= n[0] or j[1] >= n[1] or j[2] >= n[2] or inside[ix, iy, iz] == inside[j]:
                        continue
                    if d in (1, 2, 4):
                        pick.append(count)
                    count += 1
    assert count == len(verts)
    return verts[np.array(pick, np.int64)].reshape(-1, 3)


def count_interior_crossings(field, iso):
    """Interior crossing axis edges, counted with array slices (independent of the loops above)."""
    ins = np.asarray(field, F32) > F32(iso)
    total = 0
    for a in range(3):
        m = np.moveaxis(ins, (a, (a + 1) % 3, (a + 2) % 3), (0, 1, 2))
        total += int((m[1:, 1:-1, 1:-1] != m[:-1, 1:-1, 1:-1]).sum())
    return total


def edge_ends(keys, shape, lo, hi):
    """(i (E,3) lattice index of the owner, a (E,), pa (E,3), pb (E,3) fp32 world ends) of the edges ``keys``."""
    keys = np.asarray(keys, np.int64)
    p, a = keys // 3, keys % 3
    i = np.stack([p // (shape[1] * shape[2]), (p // shape[2]) % shape[1], p % shape[2]], 1)
    lo32 = np.asarray(lo, F32)
    h = M.spacing(shape, lo32, hi)
    j = i.copy()
    j[np.arange(len(keys)), a] += 1
    return i, a, lo32 + i.astype(F32) * h, lo32 + j.astype(F32) * h


def refine(density_fn, keys, field, iso, shape, lo, hi, steps):
    """``steps`` bisection steps of every crossing point along its own edge: the bracket starts at the edge's ends, the
    midpoint replaces the end whose ``> iso`` bit it shares, the result is the last bracket's midpoint.  fp32."""
    i, a, pa, pb = edge_ends(keys, shape, lo, hi)
    rows = np.arange(len(a))
    inside_a = np.asarray(field, F32)[i[:, 0], i[:, 1], i[:, 2]] > F32(iso)
    A, B = pa[rows, a].copy(), pb[rows, a].copy()
    pts = pa.copy()
    for _ in range(steps):
        pts[rows, a] = F32(0.5) * (A + B)
        same = (np.asarray(density_fn(pts), F32).reshape(-1) > F32(iso)) == inside_a
        A, B = np.where(same, pts[rows, a], A), np.where(same, B, pts[rows, a])
    pts[rows, a] = F32(0.5) * (A + B)
    return pts


# ------------------------------------------------------------------ fields with exact Hermite data

BOX_LO, BOX_HI = (-1.0, -0.8, -0.6), (1.0, 0.9, 0.7)  # non-cubic: three different spacings on most lattices


def planes_field(shape, lo, hi, planes):
    """min_i (d_i - n_i . x) over the lattice, in double, as fp32: the inside of a convex region."""
    x = M.lattice_points(shape, lo, hi)
    return np.min([d - x @ np.asarray(nv, F64) for nv, d in planes], axis=0).astype(F32)


def planes_value(planes, x):
    x = np.asarray(x, F64)
    return np.min([d - x @ np.asarray(nv, F64) for nv, d in planes], axis=0)


def planes_hermite(planes, keys, shape, lo, hi):
    """Exact Hermite data of planes_field on the edges ``keys``: where the edge meets the region's boundary (of the
    planes' roots on the edge's line, the one at which the field vanishes) and the outward normal n_i there, fp32."""
    _, a, pa, pb = edge_ends(keys, shape, lo, hi)
    pa, pb = pa.astype(F64), pb.astype(F64)
    best, pts, nrm = np.full(len(a), np.inf), np.zeros((len(a), 3)), np.zeros((len(a), 3))
    for nv, d in planes:
        nv = np.asarray(nv, F64)
        la, lb = d - pa @ nv, d - pb @ nv
        with np.errstate(all="ignore"):
            t = la / (la - lb)
        ok = np.isfinite(t) & (t >= 0.0) & (t <= 1.0)
        x = pa + np.where(ok, t, 0.0)[:, None] * (pb - pa)
        miss = np.where(ok, np.abs(planes_value(planes, x)), np.inf)
        take = miss < best
        best = np.where(take, miss, best)
        pts[take], nrm[take] = x[take], nv
    assert np.isfinite(best).all() and best.max() < 1e-6, best.max()
    return pts.astype(F32), nrm.astype(F32)


CUBE_C, CUBE_R = (0.0371, -0.0213, 0.0129), 0.4417  # off the lattice on every axis


def cube_planes(c=CUBE_C, r=CUBE_R):
    """r - max|x - c| as six planes."""
    out = []
    for a in range(3):
        for s in (1.0, -1.0):
            out.append((tuple(s if k == a else 0.0 for k in range(3)), r + s * c[a]))
    return out


def cube_surface_distance(points, c=CUBE_C, r=CUBE_R):
    q = np.abs(np.asarray(points, F64) - np.asarray(c, F64)) - r
    outside = np.sqrt((np.maximum(q, 0.0) ** 2).sum(1))
    return np.where(outside > 0.0, outside, -q.max(1))


def cube_corner_distance(verts, c=CUBE_C, r=CUBE_R):
    """The distance from each of the 8 true corners to its nearest vertex."""
    corners = np.asarray(c, F64) + r * np.array([[i, j, k] for i in (-1, 1) for j in (-1, 1) for k in (-1, 1)], F64)
    d = np.linalg.norm(corners[:, None, :] - np.asarray(verts, F64)[None, :, :], axis=-1)
    return d.min(1)


# two oblique planes that meet in a crease through the box: the normals are neither axis-aligned nor equal, so the
# covariant factor h of the local normal matters on a lattice with unequal spacings
WEDGE = (((0.48, 0.6, 0.64), 0.21), ((-0.6, 0.64, -0.48), 0.17))

SHAPE = (14, 13, 12)


@functools.lru_cache(maxsize=None)
def case(name, placement="qef", variant=None):
    """The shared known-answer cases, cached: (field, result of dual_contour)."""
    lo, hi = BOX_LO, BOX_HI
    if name == "sphere":
        lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
        f = M.sphere_field(SHAPE, lo, hi)
        return f, dual_contour(f, 0.0, lo, hi, placement, variant=variant)
    if name == "plane":
        x = M.lattice_points(SHAPE, lo, hi)
        f = (x @ np.array(PLANE_N) - PLANE_D).astype(F32)
        return f, dual_contour(f, 0.0, lo, hi, placement, variant=variant)
    planes = cube_planes() if name == "cube" else WEDGE
    f = planes_field(SHAPE, lo, hi, planes)
    keys = hermite(f, 0.0, lo, hi)["keys"]
    pts, nrm = planes_hermite(planes, keys, SHAPE, lo, hi)
    return f, dual_contour(f, 0.0, lo, hi, placement, points=pts, normals=nrm, variant=variant)


PLANE_N, PLANE_D = (0.36, -0.48, 0.8), 0.0523

# 4 x what this reference itself gives on case("cube") / case("wedge") with "qef" (test_mesh_dual_reference.py lists the
# measured values): the cube's max surface distance and max corner-to-nearest-vertex distance, the wedge's max |field|
CUBE_SURFACE_BOUND = 4 * 1.32e-8
CUBE_CORNER_BOUND = 4 * 1.56e-8
WEDGE_BOUND = 4 * 3.10e-8
