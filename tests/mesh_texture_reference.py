"""Numpy restatement of texture baking (csrc/mesh_texture_core.hpp): the per-face atlas, what every
texel stands for and the bilinear lookup, operation by operation.  numpy rounds every fp32 and fp64 operation on its
own, which is what the device does under -ffp-contract=off; the GPU tests compare bits.

The atlas of (F, S).  Faces 2c and 2c + 1 share the square cell c of S x S texels, S >= 5.  cells = max(1, (F+1)//2),
cols = the smallest integer with cols^2 >= cells, T = cols S, cell c starts at texel (S (c % cols), S (c // cols)).
Texel units, x to the right, y down, texel (i, j) covers [i, i+1] x [j, j+1].  In its cell the even face has the UV
corners (1,1), (S-3,1), (1,S-3) for its vertices 0, 1, 2, the odd face those turned by 180 degrees: (S-1,S-1),
(3,S-1), (S-1,3).  Texel (i, j) of a cell belongs to the even face where i + j < S, else to the odd one; a texel whose
face is >= F belongs to nobody (-1)."""
import math

import numpy as np

F32 = np.float32
MIN_TEXELS, MAX_SIDE = 5, 16384


def layout(F, S):
    """(cols, T), in integers."""
    if S < MIN_TEXELS:
        raise ValueError("S < 5")
    cells = max(1, (F + 1) // 2)
    cols = math.isqrt(cells - 1) + 1
    if cols * S > MAX_SIDE:
        raise ValueError("T > 16384")
    return cols, cols * S


def local_corners(S, odd):
    """(3,2) float32: the UV corners inside the cell."""
    even = np.array([[1, 1], [S - 3, 1], [1, S - 3]], F32)
    return (F32(S) - even) if odd else even


def atlas_uv(F, S):
    """(F,3,2) float32 corner coordinates in texel units of the whole atlas."""
    cols, _ = layout(F, S)
    out = np.zeros((F, 3, 2), F32)
    for f in range(F):
        c = f // 2
        out[f] = local_corners(S, f & 1) + np.array([S * (c % cols), S * (c // cols)], F32)
    return out


def owner(F, S):
    """(T,T) int32 indexed [y, x]: the face that owns every texel, -1 for nobody."""
    cols, T = layout(F, S)
    ja, ia = np.meshgrid(np.arange(T), np.arange(T), indexing="ij")
    i, j = ia % S, ja % S
    f = 2 * ((ja // S) * cols + ia // S) + (i + j >= S)
    return np.where(f < F, f, -1).astype(np.int32)


def texel_bary(S, i, j, odd):
    """(b0, b1, b2) float32 of the texels (i, j) (arrays, inside their cell) of a face of the given parity (array)."""
    xc, yc = i.astype(F32) + F32(0.5), j.astype(F32) + F32(0.5)
    x = np.where(odd, F32(S) - xc, xc).astype(F32)
    y = np.where(odd, F32(S) - yc, yc).astype(F32)
    L = F32(S - 4)
    b1 = np.maximum((x - F32(1)) / L, F32(0)).astype(F32)
    b2 = np.maximum((y - F32(1)) / L, F32(0)).astype(F32)
    s = (b1 + b2).astype(F32)
    over = s > F32(1)
    safe = np.where(over, s, F32(1)).astype(F32)
    b1 = np.where(over, b1 / safe, b1).astype(F32)
    b2 = np.where(over, b2 / safe, b2).astype(F32)
    b0 = np.maximum((F32(1) - b1) - b2, F32(0)).astype(F32)
    return b0, b1, b2


def atlas_texels(vertices, faces, S, vertex_normals=None, normals=True):
    """dict of "face" (T,T) int32, "bary" (T,T,2), "position" (T,T,3) and "normal" (T,T,3), float32, indexed [y, x]:
    position = (b0 v0 + b1 v1) + b2 v2 in fp32; normal in double, rounded to fp32 at the end: g / |g| with
    g = (b0 n0 + b1 n1) + b2 n2, or without vertex normals g = (v1 - v0) x (v2 - v0); zeros where |g| == 0.  An unowned
    texel holds zeros."""
    v = np.ascontiguousarray(vertices, F32).reshape(-1, 3)
    fa = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    F = fa.shape[0]
    cols, T = layout(F, S)
    face = owner(F, S)
    out = {"face": face, "bary": np.zeros((T, T, 2), F32), "position": np.zeros((T, T, 3), F32), "T": T, "cols": cols}
    if normals:
        out["normal"] = np.zeros((T, T, 3), F32)
    ys, xs = np.nonzero(face >= 0)
    if ys.size == 0:
        return out
    f = face[ys, xs].astype(np.int64)
    with np.errstate(all="ignore"):
        b0, b1, b2 = texel_bary(S, xs % S, ys % S, (f & 1) == 1)
        out["bary"][ys, xs] = np.stack([b1, b2], 1)
        p0, p1, p2 = v[fa[f, 0]], v[fa[f, 1]], v[fa[f, 2]]
        t0, t1, t2 = b0[:, None] * p0, b1[:, None] * p1, b2[:, None] * p2
        out["position"][ys, xs] = ((t0 + t1).astype(F32) + t2).astype(F32)
        if not normals:
            return out
        if vertex_normals is not None:
            n = np.ascontiguousarray(vertex_normals, F32).reshape(-1, 3).astype(np.float64)
            d0, d1, d2 = b0.astype(np.float64)[:, None], b1.astype(np.float64)[:, None], b2.astype(np.float64)[:, None]
            g = (d0 * n[fa[f, 0]] + d1 * n[fa[f, 1]]) + d2 * n[fa[f, 2]]
        else:
            o = p0.astype(np.float64)
            a, b = p1.astype(np.float64) - o, p2.astype(np.float64) - o
            g = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                          a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
        xx, yy, zz = g[:, 0] * g[:, 0], g[:, 1] * g[:, 1], g[:, 2] * g[:, 2]
        length = np.sqrt((xx + yy) + zz)
        zero = length == 0.0
        unit = g / np.where(zero, 1.0, length)[:, None]
        out["normal"][ys, xs] = np.where(zero[:, None], 0.0, unit).astype(F32)
    return out


def face_uv(S, face, bary):
    """(x, y) float32 inside the cell of every (face, (u, v)): (w0 P0 + u P1) + v P2 with w0 = (1 - u) - v."""
    face = np.asarray(face, np.int64)
    u, v = np.asarray(bary, F32)[:, 0], np.asarray(bary, F32)[:, 1]
    w0 = ((F32(1) - u).astype(F32) - v).astype(F32)
    odd = (face & 1) == 1
    P = np.where(odd[:, None, None], local_corners(S, True)[None], local_corners(S, False)[None]).astype(F32)
    xy = []
    for a in range(2):
        t0, t1, t2 = w0 * P[:, 0, a], u * P[:, 1, a], v * P[:, 2, a]
        xy.append(((t0 + t1).astype(F32) + t2).astype(F32))
    return xy[0], xy[1]


def _clamp_index(v, hi):
    """A float that holds an integer as an index in [0, hi], compared in float; NaN gives 0."""
    ok = v >= F32(0)
    inside = ok & (v <= F32(hi))
    return np.where(ok, np.where(inside, np.where(inside, v, 0).astype(np.int64), hi), 0)


def footprint(F, S, face, bary):
    """What the fetch reads: (ix0, ix1, iy0, iy1) int64 texel indices in the atlas and (fx, fy) float32."""
    cols, T = layout(F, S)
    face = np.asarray(face, np.int64)
    with np.errstate(all="ignore"):
        x, y = face_uv(S, np.maximum(face, 0), bary)
        ax, ay = (x - F32(0.5)).astype(F32), (y - F32(0.5)).astype(F32)
        flx, fly = np.floor(ax).astype(F32), np.floor(ay).astype(F32)
        fx, fy = (ax - flx).astype(F32), (ay - fly).astype(F32)
        cell = np.maximum(face, 0) >> 1
        ox, oy = ((cell % cols) * S).astype(F32), ((cell // cols) * S).astype(F32)
        ix0, ix1 = _clamp_index(flx + ox, T - 1), _clamp_index((flx + F32(1)).astype(F32) + ox, T - 1)
        iy0, iy1 = _clamp_index(fly + oy, T - 1), _clamp_index((fly + F32(1)).astype(F32) + oy, T - 1)
    return ix0, ix1, iy0, iy1, fx, fy


def texture_lookup(texture, S, F, face, bary):
    """(N,C) float32: top = c00 + fx (c10 - c00), bot = c01 + fx (c11 - c01), out = top + fy (bot - top) per channel;
    zeros where face < 0."""
    tex = np.ascontiguousarray(texture, F32)
    face = np.asarray(face, np.int64)
    N, C = face.shape[0], tex.shape[2]
    if N == 0:
        return np.zeros((0, C), F32)
    ix0, ix1, iy0, iy1, fx, fy = footprint(F, S, face, np.asarray(bary, F32).reshape(-1, 2))
    with np.errstate(all="ignore"):
        c00, c10, c01, c11 = tex[iy0, ix0], tex[iy0, ix1], tex[iy1, ix0], tex[iy1, ix1]
        top = (c00 + (fx[:, None] * (c10 - c00).astype(F32)).astype(F32)).astype(F32)
        bot = (c01 + (fx[:, None] * (c11 - c01).astype(F32)).astype(F32)).astype(F32)
        out = (top + (fy[:, None] * (bot - top).astype(F32)).astype(F32)).astype(F32)
    return np.where((face < 0)[:, None], F32(0), out).astype(F32)


def bake(vertices, faces, S, color_fn, vertex_normals=None):
    """The (T,T,3) float32 texture of color_fn(points, normals) at the owned texels, zeros elsewhere."""
    a = atlas_texels(vertices, faces, S, vertex_normals)
    T = a["T"]
    tex = np.zeros((T, T, 3), F32)
    own = a["face"] >= 0
    tex[own] = np.asarray(color_fn(a["position"][own], a["normal"][own]), F32)
    return tex


# ---------------------------------------------------------------- the quality check's shapes


def octasphere(levels=2):
    """An octahedron subdivided ``levels`` times with the vertices pushed onto the unit sphere: (V,3) float32,
    (F,3) int32 wound outwards; 8 * 4^levels faces (128 at two levels)."""
    v = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    v = [np.array(p, np.float64) for p in v]
    for _ in range(levels):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        f = nf
    return np.array(v, F32), np.array(f, np.int32)


def analytic_color(p, n=None):
    """0.5 + 0.5 sin(6 p + (0, 1, 2)), float32 in, float32 out (evaluated in double)."""
    p = np.asarray(p, np.float64)
    return (0.5 + 0.5 * np.sin(6.0 * p + np.array([0.0, 1.0, 2.0]))).astype(F32)


def surface_samples(faces_count, n, seed):
    """n seeded samples: (face (n,) int32, bary (n,2) float32 = (u, v)), uniform over each face by folding the unit
    square onto the triangle; the faces uniformly, which on the octasphere is nearly by area."""
    rng = np.random.default_rng(seed)
    face = rng.integers(0, faces_count, n).astype(np.int32)
    u, v = rng.random(n), rng.random(n)
    fold = u + v > 1.0
    u, v = np.where(fold, 1.0 - u, u), np.where(fold, 1.0 - v, v)
    return face, np.stack([u, v], 1).astype(F32)


def surface_points(vertices, faces, face, bary):
    """(n,3) float64: (1 - u - v) a + u b + v c."""
    v = np.asarray(vertices, np.float64)
    fa = np.asarray(faces, np.int64)[np.asarray(face, np.int64)]
    u, w = np.asarray(bary, np.float64)[:, :1], np.asarray(bary, np.float64)[:, 1:]
    return (1.0 - u - w) * v[fa[:, 0]] + u * v[fa[:, 1]] + w * v[fa[:, 2]]


def vertex_color_mix(colors, faces, face, bary):
    """(n,3) float64: the barycentric mix of per-vertex colours, what Mesh.render's "color" shows."""
    c = np.asarray(colors, np.float64)
    fa = np.asarray(faces, np.int64)[np.asarray(face, np.int64)]
    u, w = np.asarray(bary, np.float64)[:, :1], np.asarray(bary, np.float64)[:, 1:]
    return (1.0 - u - w) * c[fa[:, 0]] + u * c[fa[:, 1]] + w * c[fa[:, 2]]
