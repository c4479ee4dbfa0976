"""Reference for the generalised winding number (a helper, not a test file): the contract of DESIGN §3.11.10 and of
csrc/mesh_winding_core.hpp restated in numpy, operation by operation, plus the inputs the tests share.

Every quantity but the centroid cell is float64 and every operation is rounded once: a dot product is
(x x' + y y') + z z', a cross product six products and three differences.

  the solid angle   a, b, c = corner - q (fp32 values widened); N = a . (b x c); la = sqrt(a . a), lb, lc;
                    D = (((la lb) lc + (a . b) lc) + (b . c) la) + (c . a) lb; omega = 2 atan2(N, D)
  the brick         g_k = ((a_k + b_k) + c_k) * fp32(1/3) in fp32; brick = cell_id of the cell indices of g in the
                    brick grid; key = (brick << 32) | face, sorted; occupied brick b owns a run of sorted positions
  the moments       over the run in sorted order: x = (b - a) x (c - a); n += 0.5 x; m = sqrt(x . x); s = (a + b) + c;
                    P += m s; M += m; S += s; p = P / (3 M) if M > 0 else S / (3 count); r2 = max (corner - p)^2
  the sum           bricks ascending, d = p - q, d2 = d . d; far iff not exact and d2 > (beta beta) r2 (strict):
                    acc += (d . n) / (d2 sqrt(d2)); else acc += omega of the run's faces in order; w = acc / FOUR_PI

Only atan2 is not the same IEEE operation here and on the device; w of a closed mesh wound outwards is +1 inside,
the crossing-count winding of mesh_inside_reference with the SAME sign.
"""
import functools
import math

import numpy as np

import mesh_distance_reference as D
import mesh_inside_reference as R

F32, F64 = np.float32, np.float64
THIRD = F32(1.0 / 3.0)
FOUR_PI = 12.566370614359172
MAX_DIM = 1024
assert float(THIRD) == float.fromhex("0x1.555556p-2") and FOUR_PI == 4.0 * math.pi


def dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def _mesh(vertices, faces):
    return np.ascontiguousarray(vertices, F32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)


# ------------------------------------------------------------------ the solid angle


def solid_angles(corners, query):
    """omega (n, F) float64 of the faces ``corners`` (F, 3 corners, 3) fp32 seen from ``query`` (n, 3) fp32"""
    assert corners.dtype == F32 and query.dtype == F32
    q = query.astype(F64)[:, None, :]
    a, b, c = (corners[None, :, k, :].astype(F64) - q for k in range(3))
    N = dot(a, cross(b, c))
    la, lb, lc = np.sqrt(dot(a, a)), np.sqrt(dot(b, b)), np.sqrt(dot(c, c))
    ab, bc, ca = dot(a, b), dot(b, c), dot(c, a)
    den = (((la * lb) * lc + ab * lc) + bc * la) + ca * lb
    return 2.0 * np.arctan2(N, den)


def plain(vertices, faces, query):
    """w by a plain loop over the faces in their own order (no bricks): (n,) float64"""
    v, f = _mesh(vertices, faces)
    om = solid_angles(v[f], np.ascontiguousarray(query, F32).reshape(-1, 3))
    acc = np.zeros(len(om), F64)
    for j in range(om.shape[1]):
        acc = acc + om[:, j]
    return acc / FOUR_PI


# ------------------------------------------------------------------ the bricks


def default_bricks_per_axis(F):
    return min(max(math.ceil(1.25 * F ** 0.25), 1), MAX_DIM)


def brick_grid(vertices, faces, bricks_per_axis=None):
    """{lo (3,) fp32, cell, inv (fp32), dims} by the rule of kernels.mesh_winding_bricks"""
    v, f = _mesh(vertices, faces)
    k = default_bricks_per_axis(len(f)) if bricks_per_axis is None else bricks_per_axis
    lo = v.min(0)
    ext = v.max(0) - lo
    with np.errstate(all="ignore"):
        cell = ext.max() / F32(k) if ext.max() > 0 else F32(1.0)
        inv = F32(1.0) / cell
        if not (np.isfinite(cell) and cell > 0 and np.isfinite(inv) and inv > 0):
            cell, inv = F32(1.0), F32(1.0)
        cells = np.minimum(np.floor(ext * inv), k - 1)
    return {"lo": lo, "cell": F32(cell), "inv": F32(inv), "dims": [int(c) + 1 for c in cells]}


def face_keys(vertices, faces, grid):
    """the sorted keys (brick << 32) | face, (F,) int64"""
    v, f = _mesh(vertices, faces)
    t = v[f]
    g = ((t[:, 0] + t[:, 1]) + t[:, 2]) * THIRD
    assert g.dtype == F32
    i = [D.cell_index(grid, k, g[:, k]) for k in range(3)]
    _, ny, nz = grid["dims"]
    return np.sort((((i[0] * ny + i[1]) * nz + i[2]) << 32) | np.arange(len(f), dtype=np.int64))


def bricks(vertices, faces, bricks_per_axis=None):
    """The dict of kernels.mesh_winding_bricks in numpy: keys, runs (B,2) int32, moments (B,7) float64, soup (F,9) fp32,
    lo, cell, inv, dims, B, F.  The moments are summed face by face in sorted order."""
    v, f = _mesh(vertices, faces)
    grid = brick_grid(v, f, bricks_per_axis)
    keys = face_keys(v, f, grid)
    soup = v[f[keys & 0xffffffff]].reshape(-1, 9) if len(f) else np.zeros((0, 9), F32)
    cells = keys >> 32
    starts = np.nonzero(np.concatenate([[True], cells[1:] != cells[:-1]]))[0] if len(f) else np.zeros(0, np.int64)
    ends = np.concatenate([starts[1:], [len(f)]]) if len(f) else starts
    moments = np.zeros((len(starts), 7), F64)
    for b, (s, e) in enumerate(zip(starts, ends)):
        n, P, S, M = np.zeros(3, F64), np.zeros(3, F64), np.zeros(3, F64), F64(0.0)
        for j in range(s, e):
            a, bb, c = (soup[j, 3 * k:3 * k + 3].astype(F64) for k in range(3))
            x = cross(bb - a, c - a)
            m = np.sqrt(dot(x, x))
            sk = (a + bb) + c
            n, P, S, M = n + 0.5 * x, P + m * sk, S + sk, M + m
        p = P / (3.0 * M) if M > 0 else S / (3.0 * F64(e - s))
        d = soup[s:e].reshape(-1, 3).astype(F64) - p
        moments[b, :3], moments[b, 3:6], moments[b, 6] = p, n, max(0.0, dot(d, d).max())
    return {**grid, "keys": keys, "runs": np.stack([starts, ends], 1).astype(np.int32).reshape(-1, 2),
            "moments": moments, "soup": soup, "B": len(starts), "F": len(f)}


# ------------------------------------------------------------------ the sum of a query


def winding(query, br, beta=3.0, exact=False, counts=False, omega=None):
    """w (n,) float64 of ``query`` (n,3) fp32 against the dict ``br`` of bricks(); with ``counts`` also (far bricks,
    faces summed exactly) per query, (n,2) int64.  ``omega``: solid_angles of the mesh's faces in their OWN order,
    (n, F), when the caller has them (a face's solid angle does not depend on the bricks; the order of the sum does)."""
    q32 = np.ascontiguousarray(query, F32).reshape(-1, 3)
    q = q32.astype(F64)
    # (n, F) in sorted order
    om = solid_angles(br["soup"].reshape(-1, 3, 3), q32) if omega is None else omega[:, br["keys"] & 0xffffffff]
    acc = np.zeros(len(q), F64)
    count = np.zeros((len(q), 2), np.int64)
    beta2 = float(beta) * float(beta)
    for b in range(br["B"]):
        rec = br["moments"][b]
        d = rec[:3] - q
        d2 = dot(d, d)
        far = np.zeros(len(q), bool) if exact else d2 > beta2 * rec[6]
        with np.errstate(all="ignore"):
            term = dot(d, rec[3:6]) / (d2 * np.sqrt(d2))
        acc = np.where(far, acc + term, acc)
        s, e = br["runs"][b]
        for j in range(s, e):
            acc = np.where(far, acc, acc + om[:, j])
        count[:, 0] += far
        count[:, 1] += np.where(far, 0, e - s)
    w = acc / FOUR_PI
    return (w, count) if counts else w


# ------------------------------------------------------------------ shared inputs


def uv_sphere(rings, segments, radius=1.0, z_min=None, z_max=None):
    """A latitude / longitude sphere wound outwards (the generator of the host checks), fp32; only the faces whose
    three corners have z in [z_min, z_max] are kept, the vertices all stay.  The ring at the equator (even ``rings``)
    has z = 0 exactly."""
    v = [(0.0, 0.0, radius)]
    for i in range(1, rings):
        for j in range(segments):
            th, ph = math.pi * i / rings, 2 * math.pi * j / segments
            z = 0.0 if 2 * i == rings else radius * math.cos(th)
            v.append((radius * math.sin(th) * math.cos(ph), radius * math.sin(th) * math.sin(ph), z))
    v.append((0.0, 0.0, -radius))
    last = len(v) - 1

    def at(i, j):
        return 1 + (i - 1) * segments + j % segments

    f = []
    for j in range(segments):
        f.append((0, at(1, j), at(1, j + 1)))
        f.append((last, at(rings - 1, j + 1), at(rings - 1, j)))
        for i in range(1, rings - 1):
            f.append((at(i, j), at(i + 1, j), at(i + 1, j + 1)))
            f.append((at(i, j), at(i + 1, j + 1), at(i, j + 1)))
    v, f = np.asarray(v, F32), np.asarray(f, np.int32)
    z = v[f][:, :, 2]
    keep = np.ones(len(f), bool)
    if z_min is not None:
        keep &= (z >= z_min).all(1)
    if z_max is not None:
        keep &= (z <= z_max).all(1)
    return v, np.ascontiguousarray(f[keep])


@functools.lru_cache(maxsize=None)
def hemisphere():
    """the upper half of a 16 x 24 sphere of radius 1, open, its rim in the plane z = 0: 360 faces"""
    v, f = uv_sphere(16, 24, z_min=0.0)
    used = np.unique(f)
    assert len(f) == 360 and (v[used, 2] >= 0).all() and (v[used, 2] == 0).sum() == 24
    return v, f


@functools.lru_cache(maxsize=None)
def cut_sphere():
    """a 20 x 32 sphere of radius 1 without the faces that reach above z = 0.85 (a cap cut off at 15 % of the radius):
    open, 992 faces"""
    v, f = uv_sphere(20, 32, z_max=0.85)
    assert len(f) == 992
    return v, f


def one_face():
    return D.TRIANGLE


MESHES = {"one_face": one_face, "sphere12": R.sphere, "hemisphere": hemisphere, "cut_sphere": cut_sphere,
          "soup60": D.soup60, "tiny_face": D.tiny_face_mesh}
OPEN = ("hemisphere", "cut_sphere")


def mesh(name):
    return MESHES[name]()


@functools.lru_cache(maxsize=None)
def box_queries(n=400, half=1.3, seed=21):
    """n queries uniform in [-half, half]^3, fp32"""
    return np.random.default_rng(seed).uniform(-half, half, (n, 3)).astype(F32)


@functools.lru_cache(maxsize=None)
def queries(name):
    """The query set of a mesh: 2000 box queries of [-1.3, 1.3]^3 for the unit spheres and their parts, the sets of
    mesh_inside_reference for its meshes (lattice nodes and points under edges and corners included), 300 around
    the one face."""
    if name in ("hemisphere", "cut_sphere"):
        return box_queries(2000, 1.3, 22)
    if name == "one_face":
        return np.random.default_rng(23).uniform(-1.0, 2.0, (300, 3)).astype(F32)
    return R.queries(name)


def fine_bricks_per_axis(name):
    """a brick grid fine enough that most bricks hold one face"""
    return {"one_face": 4, "soup60": 64, "tiny_face": 1024}.get(name, 128)


@functools.lru_cache(maxsize=None)
def bricks_of(name, which):
    """bricks() of a mesh for ``which`` in ("one", "default", "fine")"""
    k = {"one": 1, "default": None, "fine": fine_bricks_per_axis(name)}[which]
    return bricks(*mesh(name), k)


@functools.lru_cache(maxsize=None)
def omega_of(name):
    v, f = _mesh(*mesh(name))
    return solid_angles(v[f], queries(name))


@functools.lru_cache(maxsize=None)
def winding_of(name, which, beta, exact):
    w = winding(queries(name), bricks_of(name, which), beta, exact, omega=omega_of(name))
    w.setflags(write=False)
    return w


def tolerance(br):
    """(F + B) 2^-50: about a dozen ulps of 2 pi per term for the device's atan2, every other operation being the
    same on both sides"""
    return (br["F"] + br["B"]) * 2.0 ** -50


# The error table of DESIGN §3.11.10: (max, mean) of |w_beta - w_exact| over box_queries() on the default bricks,
# as this reference gave them; tests/test_mesh_winding_reference.py bounds each entry by twice these.
ERROR_BETAS = (2.0, 3.0, 4.0)
ERROR_TABLE = {"hemisphere": ((1.2190e-02, 1.9858e-03), (4.2960e-03, 8.2250e-04), (8.4503e-04, 3.7922e-04)),
               "cut_sphere": ((1.3112e-02, 3.0527e-03), (8.2845e-03, 1.3661e-03), (3.1622e-03, 7.0476e-04))}


@functools.lru_cache(maxsize=None)
def error_table(name):
    """((max, mean) of |w_beta - w_exact| for beta in ERROR_BETAS, (far bricks, exact faces) per query likewise)"""
    q, br = box_queries(), bricks_of(name, "default")
    v, f = _mesh(*mesh(name))
    om = solid_angles(v[f], q)
    exact = winding(q, br, exact=True, omega=om)
    errors, work = [], []
    for beta in ERROR_BETAS:
        w, count = winding(q, br, beta, counts=True, omega=om)
        e = np.abs(w - exact)
        errors.append((float(e.max()), float(e.mean())))
        work.append((float(count[:, 0].mean()), float(count[:, 1].mean())))
    return tuple(errors), tuple(work)
