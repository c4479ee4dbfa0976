"""Reference for the mesh extractor (a helper, not a test file): marching tetrahedra over the Kuhn split of a lattice,
restated in numpy with plain loops, plus the topology helpers the mesh tests share.

The rule.  field (nx,ny,nz) fp32, linear index p = (ix ny + iy) nz + iz; a point is inside iff
field > iso.  Point p owns the edges p -> p + d, d = 1..7 (bit 0 = +x, bit 1 = +y, bit 2 = +z) that stay in the
lattice; an owned edge whose ends differ carries one vertex pa + t (pb - pa), t = (f[p] - iso) / (f[p] - f[q]), all in
fp32.  Vertices are ordered by (p, d).  The cell with low corner p is cut into the six tetrahedra of the axis
permutations (x,y,z), (x,z,y), (y,x,z), (y,z,x), (z,x,y), (z,y,x): c0 = p, c1 = c0 + e_a, c2 = c1 + e_b,
c3 = p + (1,1,1).  One or three corners inside: the triangle of the three edges at the lone corner A, towards the
others in corner order.  Two inside (A < B inside, C < D outside): the quad [E(A,C), E(A,D), E(B,D), E(B,C)] as
(q0,q1,q2), (q0,q2,q3).  Faces are ordered by (cell, tetrahedron, triangle).

Orientation is decided here geometrically, never from a table: on the unit cube with every vertex at its edge's
midpoint, a triangle whose normal (v1-v0) x (v2-v0) points from the outside corners' centroid towards the inside
corners' has its second and third index swapped (both triangles of a quad alike).  The swap is invariant under the
positive axis scalings and the vertex positions of a real lattice, because the triangle always separates the
tetrahedron's inside corners from its outside corners.
"""
import numpy as np

F32 = np.float32
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))


def tet_corners(t):
    """The four corner masks (bit a = +e_a) of tetrahedron t of a cell."""
    a, b, _ = PERMS[t]
    return (0, 1 << a, (1 << a) | (1 << b), 7)


def _unit(mask):
    return np.array([(mask >> a) & 1 for a in range(3)], dtype=np.float64)


def case_triangles(inside):
    """inside: 4 bools (corner order) -> list of triangles, each three (i, j) corner pairs, as the rule writes them."""
    ins = [i for i in range(4) if inside[i]]
    out = [i for i in range(4) if not inside[i]]
    if len(ins) in (0, 4):
        return []
    if len(ins) in (1, 3):
        A = ins[0] if len(ins) == 1 else out[0]
        B, C, D = [i for i in range(4) if i != A]
        return [((A, B), (A, C), (A, D))]
    A, B = ins
    C, D = out
    q = ((A, C), (A, D), (B, D), (B, C))
    return [(q[0], q[1], q[2]), (q[0], q[2], q[3])]


def swap_needed(t, inside):
    """Geometric orientation test on the unit cube with midpoint vertices: True iff the rule's triangles of
    (tetrahedron t, inside pattern) point towards the inside corners and must have indices 1 and 2 swapped."""
    cm = tet_corners(t)
    tris = case_triangles(inside)
    if not tris:
        return False
    pos = [_unit(m) for m in cm]
    cin = np.mean([pos[i] for i in range(4) if inside[i]], axis=0)
    cout = np.mean([pos[i] for i in range(4) if not inside[i]], axis=0)
    flips = []
    for tri in tris:
        v = [(pos[i] + pos[j]) / 2 for i, j in tri]
        n = np.cross(v[1] - v[0], v[2] - v[0])
        s = float(np.dot(n, cout - cin))
        assert abs(s) > 1e-9, (t, inside)
        flips.append(s < 0)
    assert all(f == flips[0] for f in flips), (t, inside)
    return flips[0]


def spacing(shape, lo, hi):
    lo, hi = np.asarray(lo, F32), np.asarray(hi, F32)
    return np.array([(hi[a] - lo[a]) / F32(shape[a] - 1) for a in range(3)], F32)


def grid_gradient(field, h):
    """Central differences (one-sided on the border) over the world spacing, fp32: (nx,ny,nz,3)."""
    f = np.asarray(field, F32)
    g = np.zeros(f.shape + (3,), F32)
    for a in range(3):
        fa = np.moveaxis(f, a, 0)
        ga = np.zeros_like(fa)
        ga[1:-1] = (fa[2:] - fa[:-2]) / (F32(2) * h[a])
        ga[0] = (fa[1] - fa[0]) / h[a]
        ga[-1] = (fa[-1] - fa[-2]) / h[a]
        g[..., a] = np.moveaxis(ga, 0, a)
    return g


def marching_tets(field, iso, lo, hi, normals=False):
    """-> verts (V,3) f32, faces (F,3) i32 [, normals (V,3) f32] by the rule above."""
    f = np.ascontiguousarray(field, F32)
    nx, ny, nz = f.shape
    n = (nx, ny, nz)
    iso = F32(iso)
    lo = np.asarray(lo, F32)
    h = spacing(n, lo, hi)
    inside = f > iso
    grad = grid_gradient(f, h) if normals else None
    vid = {}
    verts, norms = [], []
    for ix in range(nx):
        for iy in range(ny):
            for iz in range(nz):
                i = (ix, iy, iz)
                for d in range(1, 8):
                    j = (ix + (d & 1), iy + ((d >> 1) & 1), iz + ((d >> 2) & 1))
                    if j[0] >= nx or j[1] >= ny or j[2] >= nz or inside[i] == inside[j]:
                        continue
                    t = (f[i] - iso) / (f[i] - f[j])
                    v = np.zeros(3, F32)
                    for a in range(3):
                        pa = lo[a] + F32(i[a]) * h[a]
                        pb = lo[a] + F32(j[a]) * h[a]
                        v[a] = pa + t * (pb - pa)
                    vid[(i, d)] = len(verts)
                    verts.append(v)
                    if normals:
                        g = grad[i] + t * (grad[j] - grad[i])
                        ln = F32(np.sqrt(np.sum(g * g, dtype=F32)))
                        norms.append(-g / max(ln, F32(1e-12)))
    faces = []
    for ix in range(nx - 1):
        for iy in range(ny - 1):
            for iz in range(nz - 1):
                for t in range(6):
                    cm = tet_corners(t)
                    cp = [(ix + (m & 1), iy + ((m >> 1) & 1), iz + ((m >> 2) & 1)) for m in cm]
                    ins = [bool(inside[c]) for c in cp]
                    tris = case_triangles(ins)
                    if not tris:
                        continue
                    sw = swap_needed(t, ins)
                    for tri in tris:
                        idx = [vid[(cp[min(a, b)], cm[max(a, b)] ^ cm[min(a, b)])] for a, b in tri]
                        faces.append([idx[0], idx[2], idx[1]] if sw else idx)
    V = np.array(verts, F32).reshape(-1, 3)
    Fc = np.array(faces, np.int32).reshape(-1, 3)
    if normals:
        return V, Fc, np.array(norms, F32).reshape(-1, 3)
    return V, Fc


# ------------------------------------------------------------------ fields


def lattice_points(shape, lo, hi):
    """World positions of the lattice, float64 (for building analytic fields): (nx,ny,nz,3)."""
    ax = [np.linspace(float(lo[a]), float(hi[a]), shape[a]) for a in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1)


def sphere_field(shape, lo, hi, r0=0.6, centre=(0.0, 0.0, 0.0)):
    x = lattice_points(shape, lo, hi) - np.asarray(centre, np.float64)
    return (r0 - np.linalg.norm(x, axis=-1)).astype(F32)


def torus_field(shape, lo, hi, R=0.55, r=0.25):
    x = lattice_points(shape, lo, hi)
    return (r - np.sqrt((np.sqrt(x[..., 0] ** 2 + x[..., 1] ** 2) - R) ** 2 + x[..., 2] ** 2)).astype(F32)


def noise_field(shape, seed, border_outside=False):
    f = np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(F32)
    if border_outside:
        f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = -1, -1, -1, -1, -1, -1
    return f


def sines_field(shape, lo, hi):
    x = lattice_points(shape, lo, hi)
    return (np.sin(2.3 * x[..., 0] + 0.4) + np.sin(3.1 * x[..., 1] - 0.7) * np.cos(1.7 * x[..., 2])
            + 0.5 * np.sin(4.0 * x[..., 0] * x[..., 2] + 1.1)).astype(F32)


def integer_field(shape, seed):
    """Integer values in -2..2, all-outside border: iso = 0 lies on lattice values."""
    f = np.random.default_rng(seed).integers(-2, 3, shape).astype(F32)
    f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = -1, -1, -1, -1, -1, -1
    return f


# ------------------------------------------------------------------ topology and measures


def directed_edge_counts(faces):
    c = {}
    for a, b, d in np.asarray(faces).tolist():
        for e in ((a, b), (b, d), (d, a)):
            c[e] = c.get(e, 0) + 1
    return c


def undirected_edge_counts(faces):
    c = {}
    for (a, b), k in directed_edge_counts(faces).items():
        e = (min(a, b), max(a, b))
        c[e] = c.get(e, 0) + k
    return c


def is_closed(faces):
    """Every undirected edge in exactly two faces and every directed edge exactly once (closed, consistently
    oriented)."""
    return (all(k == 1 for k in directed_edge_counts(faces).values())
            and all(k == 2 for k in undirected_edge_counts(faces).values()))


def boundary_edges(faces):
    return [e for e, k in undirected_edge_counts(faces).items() if k != 2]


def euler_characteristic(n_verts, faces):
    return int(n_verts) - len(undirected_edge_counts(faces)) + len(faces)


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.sum(np.einsum("ij,ij->i", a, np.cross(b, c))) / 6.0)


def face_normals(verts, faces):
    v = np.asarray(verts, np.float64)
    return np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])


def area(verts, faces):
    return float(0.5 * np.linalg.norm(face_normals(verts, faces), axis=-1).sum())
