"""Reference for the TSDF fusion (a helper, not a test file): the rule of DESIGN §3.11.8 restated in numpy, vectorised
over the voxels with a Python loop over the views, every intermediate an np.float32 array (numpy rounds every fp32
operation once and its fp32 divide and sqrt are correctly rounded); the face filter as a loop over cells; and the
sphere case the CPU and the device tests share.

The rule.  Volume (nx,ny,nz), p = (ix ny + iy) nz + iz, x = lo + (ix,iy,iz) h with mesh_reference.spacing's h; a fresh
volume has tsdf = 1, weight = 0.  Per voxel and view M (12 floats, rows of the 3x4 camera-to-world matrix; pixel
centres, the camera looks along -z, y up), in ascending view order:
  q = x - (M[3], M[7], M[11]);  c_j = q0 M[j] + q1 M[4+j] + q2 M[8+j];  zc = -c_2, skip unless zc > 0
  u = fx (c_0 / zc) + cx,  v = fy ((-c_1) / zc) + cy;  skip unless 0 <= u < W and 0 <= v < H (float compare)
  d = depth[floor(v), floor(u)];  skip unless d finite and d > 0
  r = sqrt(q0 q0 + q1 q1 + q2 q2);  s = d - r;  skip if s < -trunc
  t = min(1, s / trunc);  tsdf = (tsdf w + t) / (w + 1);  w = w + 1
"""
import numpy as np

import mesh_reference as MR

F32 = np.float32


def fresh(shape):
    return np.ones(shape, F32), np.zeros(shape, F32)


def lattice(shape, lo, hi):
    """fp32 world positions (nx,ny,nz,3), lo + i h as the extractor rounds it"""
    lo = np.asarray(lo, F32)
    h = MR.spacing(shape, lo, hi)
    ax = [lo[a] + np.arange(shape[a]).astype(F32) * h[a] for a in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).astype(F32)


def rows12(c2w):
    """(n,12) fp32 from (n,3,4), (n,4,4), (3,4) or (4,4)"""
    c = np.asarray(c2w, F32)
    if c.ndim == 2:
        c = c[None]
    return np.ascontiguousarray(c[:, :3, :4]).reshape(-1, 12)


def integrate(tsdf, weight, lo, hi, depth, c2w, fx, fy, cx, cy, trunc):
    """-> (tsdf, weight), new arrays; the inputs are left as they are"""
    tsdf, weight = np.array(tsdf, F32), np.array(weight, F32)
    shape = tsdf.shape
    depth = np.asarray(depth, F32)
    if depth.ndim == 2:
        depth = depth[None]
    M_all = rows12(c2w)
    assert len(M_all) == len(depth)
    H, W = depth.shape[1:]
    fx, fy, cx, cy, trunc = F32(fx), F32(fy), F32(cx), F32(cy), F32(trunc)
    x = lattice(shape, lo, hi).reshape(-1, 3)
    T, Wt = tsdf.reshape(-1), weight.reshape(-1)
    one = F32(1)
    with np.errstate(all="ignore"):
        for M, img in zip(M_all, depth):
            q0, q1, q2 = x[:, 0] - M[3], x[:, 1] - M[7], x[:, 2] - M[11]
            c = [q0 * M[j] + q1 * M[4 + j] + q2 * M[8 + j] for j in range(3)]
            zc = -c[2]
            ok = zc > 0
            u = fx * (c[0] / zc) + cx
            v = fy * ((-c[1]) / zc) + cy
            ok &= (u >= 0) & (u < F32(W)) & (v >= 0) & (v < F32(H))
            col = np.where(ok, np.floor(u), 0).astype(np.int64)
            row = np.where(ok, np.floor(v), 0).astype(np.int64)
            d = img[row, col]
            ok &= np.isfinite(d) & (d > 0)
            r = np.sqrt(q0 * q0 + q1 * q1 + q2 * q2)
            s = d - r
            ok &= ~(s < -trunc)
            tq = s / trunc
            t = np.where(tq < one, tq, one).astype(F32)
            new = (T * Wt + t) / (Wt + one)
            assert new.dtype == F32 and r.dtype == F32 and u.dtype == F32
            T = np.where(ok, new, T)
            Wt = np.where(ok, Wt + one, Wt)
    return T.reshape(shape), Wt.reshape(shape)


def face_offsets(field, iso):
    """(P+1,) int32: the exclusive scan of the triangles per cell of marching_tets(field, iso, ...), by low corner p"""
    f = np.asarray(field, F32)
    nx, ny, nz = f.shape
    inside = f > F32(iso)
    cnt = np.zeros(nx * ny * nz + 1, np.int64)
    for ix in range(nx - 1):
        for iy in range(ny - 1):
            for iz in range(nz - 1):
                k = 0
                for t in range(6):
                    cm = MR.tet_corners(t)
                    ins = [bool(inside[ix + (m & 1), iy + ((m >> 1) & 1), iz + ((m >> 2) & 1)]) for m in cm]
                    k += len(MR.case_triangles(ins))
                cnt[(ix * ny + iy) * nz + iz + 1] = k
    return np.cumsum(cnt).astype(np.int32)


def cell_observed(weight, ix, iy, iz, min_weight):
    w = np.asarray(weight, F32)
    return bool((w[ix:ix + 2, iy:iy + 2, iz:iz + 2] >= F32(min_weight)).all())


def face_observed(face_off, weight, min_weight):
    """keep (F,) uint8: a loop over the cells and their ranges of face_off"""
    nx, ny, nz = weight.shape
    keep = np.zeros(int(face_off[-1]), np.uint8)
    for ix in range(nx - 1):
        for iy in range(ny - 1):
            for iz in range(nz - 1):
                p = (ix * ny + iy) * nz + iz
                if face_off[p + 1] > face_off[p]:
                    keep[face_off[p]:face_off[p + 1]] = cell_observed(weight, ix, iy, iz, min_weight)
    return keep


def compact(verts, faces, keep):
    """the faces with keep set and the vertices they use, both in their order, renumbered densely (mesh_compact)"""
    f = np.asarray(faces)[np.asarray(keep, bool)]
    used = np.zeros(len(verts), bool)
    used[f.reshape(-1)] = True
    new = np.cumsum(used) - 1
    return np.asarray(verts)[used], new[f].astype(np.int32)


def extract(tsdf, weight, lo, hi, min_weight=1):
    """The reference pipeline: marching tetrahedra of -tsdf at 0, the face filter, the compaction.
    -> (verts, faces) kept, (verts, faces) unfiltered, keep"""
    v, f = MR.marching_tets(-np.asarray(tsdf, F32), 0.0, lo, hi)
    keep = face_observed(face_offsets(-np.asarray(tsdf, F32), 0.0), weight, min_weight)
    return compact(v, f, keep), (v, f), keep


# ------------------------------------------------------------------ the sphere case

SPHERE_R = 0.6
SPHERE_SHAPE = (24, 24, 24)
SPHERE_LO, SPHERE_HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
SPHERE_HW = 48
SPHERE_FOCAL = 24.0 / np.tan(0.5 * 0.6911112)


def sphere_h():
    return float(MR.spacing(SPHERE_SHAPE, SPHERE_LO, SPHERE_HI).max())


def sphere_cameras():
    """(14,3,4) fp32: scene.look_at from distance 4 on the 6 axis and the 8 diagonal directions"""
    import torch
    from nerf_amd.scene import look_at
    dirs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    dirs += [(a, b, c) for a in (1, -1) for b in (1, -1) for c in (1, -1)]
    out = []
    for d in dirs:
        p = torch.tensor(d, dtype=torch.float64)
        out.append(look_at(p / p.norm() * 4.0).numpy())
    return np.stack(out).astype(F32)


def pixel_rays(c2w, H, W, fx, fy, cx, cy):
    """origins (3,) and unit directions (H,W,3), float64, of make_ray's pixel centres"""
    M = np.asarray(c2w, np.float64)[:3, :4]
    j, i = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    d = np.stack([(i - cx) / fx, -(j - cy) / fy, -np.ones_like(i)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return M[:, 3], d @ M[:, :3].T


def sphere_depth(c2w, H, W, fx, fy, cx, cy, radius=SPHERE_R):
    """(H,W) fp32: the analytic range to the sphere at the origin, +inf on a miss"""
    o, d = pixel_rays(c2w, H, W, fx, fy, cx, cy)
    b = d @ o
    disc = b * b - (o @ o - radius * radius)
    t = -b - np.sqrt(np.maximum(disc, 0.0))
    return np.where((disc > 0) & (t > 0), t, np.inf).astype(F32)


_SPHERE = {}


def sphere_case():
    """dict: c2w, depth, intrinsics, trunc, the fused (tsdf, weight) and the extraction; computed once per process"""
    if not _SPHERE:
        c2w = sphere_cameras()
        n = SPHERE_HW
        k = (SPHERE_FOCAL, SPHERE_FOCAL, n / 2.0, n / 2.0)
        depth = np.stack([sphere_depth(M, n, n, *k) for M in c2w])
        trunc = F32(3.0) * F32(sphere_h())
        tsdf, weight = integrate(*fresh(SPHERE_SHAPE), SPHERE_LO, SPHERE_HI, depth, c2w, *k, trunc)
        kept, full, keep = extract(tsdf, weight, SPHERE_LO, SPHERE_HI, 1)
        for a in (c2w, depth, tsdf, weight, *kept, *full, keep):
            a.setflags(write=False)
        _SPHERE.update(c2w=c2w, depth=depth, k=k, trunc=float(trunc), tsdf=tsdf, weight=weight, kept=kept, full=full,
                       keep=keep)
    return _SPHERE


def sphere_errors(verts, radius=SPHERE_R):
    return np.abs(np.linalg.norm(np.asarray(verts, np.float64), axis=-1) - radius)
