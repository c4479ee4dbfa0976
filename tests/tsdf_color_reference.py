"""Reference for the TSDF fusion with colour (a helper, not a test file): the two rules of DESIGN §3.11.9 restated in
numpy on top of tests/tsdf_reference.py, every intermediate an np.float32 array (one rounding per operation; numpy's
fp32 divide and sqrt are correctly rounded), and the coloured sphere case the CPU and the device tests share.

Fusion.  color (nx,ny,nz,4) = r, g, b and a colour weight cw per voxel, zeros in a fresh volume; rgb (n,H,W,3).  Per
voxel and view, in ascending view order, the steps of tsdf_reference up to  s = d - r, skip if s < -trunc, then
  tq = s / trunc;  t = min(1, tq);  tsdf = (tsdf w + t) / (w + 1);  w = w + 1
  if tq < 1 and the three channels of rgb[view, floor(v), floor(u)] are finite:
      c_j = (c_j cw + pixel_j) / (cw + 1) for j = r, g, b;  cw = cw + 1

Sampling at a point x.  Per axis a:  g = (x_a - lo_a) / h_a clamped to [0, n_a - 1];  i = min(int(floor(g)), n_a - 2);
f = g - float(i).  Over the corners c = 0..7 at (i_x + (c & 1), i_y + (c >> 1 & 1), i_z + (c >> 2 & 1)):
  w_a = f_a where the corner's bit of the axis is set, else 1 - f_a;  tw = (w_x w_y) w_z;  k = tw cw_corner
  cover = cover + k;  acc_j = acc_j + k c_j
rgb_j = acc_j / cover where cover > 0, else 0.  A point with a NaN coordinate has cover = 0.
"""
import numpy as np

import mesh_reference as MR
from tsdf_reference import lattice, rows12, sphere_case
import tsdf_reference as T

F32 = np.float32


def fresh_color(shape):
    return np.zeros(tuple(shape) + (4,), F32)


def integrate(tsdf, weight, color, lo, hi, depth, rgb, c2w, fx, fy, cx, cy, trunc):
    """-> (tsdf, weight, color), new arrays; the inputs are left as they are"""
    tsdf, weight, color = np.array(tsdf, F32), np.array(weight, F32), np.array(color, F32)
    shape = tsdf.shape
    assert color.shape == shape + (4,)
    depth, rgb = np.asarray(depth, F32), np.asarray(rgb, F32)
    if depth.ndim == 2:
        depth, rgb = depth[None], rgb[None]
    M_all = rows12(c2w)
    assert len(M_all) == len(depth) and rgb.shape == depth.shape + (3,)
    H, W = depth.shape[1:]
    fx, fy, cx, cy, trunc = F32(fx), F32(fy), F32(cx), F32(cy), F32(trunc)
    x = lattice(shape, lo, hi).reshape(-1, 3)
    T_, Wt, C = tsdf.reshape(-1), weight.reshape(-1), color.reshape(-1, 4)
    one = F32(1)
    with np.errstate(all="ignore"):
        for M, img, col_img in zip(M_all, depth, rgb):
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
            new = (T_ * Wt + t) / (Wt + one)
            assert new.dtype == F32 and tq.dtype == F32
            T_ = np.where(ok, new, T_)
            Wt = np.where(ok, Wt + one, Wt)
            pixel = col_img[row, col]  # (P,3)
            paint = ok & (tq < one) & np.isfinite(pixel).all(-1)
            cw = C[:, 3]
            cw1 = cw + one
            mixed = (C[:, :3] * cw[:, None] + pixel) / cw1[:, None]
            assert mixed.dtype == F32
            C = np.where(paint[:, None], np.concatenate([mixed, cw1[:, None]], 1), C).astype(F32)
    return T_.reshape(shape), Wt.reshape(shape), C.reshape(shape + (4,))


def sample(color, lo, hi, points):
    """-> rgb (N,3), cover (N,), fp32"""
    color = np.asarray(color, F32)
    shape = color.shape[:3]
    pts = np.asarray(points, F32).reshape(-1, 3)
    lo32 = np.asarray(lo, F32)
    h = MR.spacing(shape, lo, hi)
    nan = np.isnan(pts).any(-1)
    one = F32(1)
    idx, frac = [], []
    with np.errstate(all="ignore"):
        for a in range(3):
            g = (np.where(nan, F32(0), pts[:, a]) - lo32[a]) / h[a]
            g = np.minimum(np.maximum(g, F32(0)), F32(shape[a] - 1)).astype(F32)
            i = np.minimum(np.floor(g).astype(np.int64), shape[a] - 2)
            idx.append(i)
            frac.append((g - i.astype(F32)).astype(F32))
        cover = np.zeros(len(pts), F32)
        acc = np.zeros((len(pts), 3), F32)
        for c in range(8):
            b = [(c >> a) & 1 for a in range(3)]
            w = [frac[a] if b[a] else one - frac[a] for a in range(3)]
            corner = color[idx[0] + b[0], idx[1] + b[1], idx[2] + b[2]]  # (N,4)
            k = ((w[0] * w[1]) * w[2]) * corner[:, 3]
            assert k.dtype == F32
            cover = cover + k
            acc = acc + k[:, None] * corner[:, :3]
        cover = np.where(nan, F32(0), cover).astype(F32)
        seen = cover > 0
        rgb = np.where(seen[:, None], acc / np.where(seen, cover, one)[:, None], F32(0)).astype(F32)
    return rgb, cover


# ------------------------------------------------------------------ the coloured sphere case


def sphere_color_at(p):
    """the analytic colour 0.5 + 0.4 p / R of a point of the sphere (float64)"""
    return 0.5 + 0.4 * np.asarray(p, np.float64) / T.SPHERE_R


def sphere_rgb(c2w, depth, k):
    """(H,W,3) fp32: the colour of every pixel's hit point, 0 on a miss"""
    H, W = depth.shape
    o, d = T.pixel_rays(c2w, H, W, *k)
    hit = np.isfinite(depth)
    p = o + d * np.where(hit, depth, 0.0).astype(np.float64)[..., None]
    return np.where(hit[..., None], sphere_color_at(p), 0.0).astype(F32)


_SPHERE = {}


def sphere_color_case():
    """sphere_case() with rgb (14,48,48,3), the fused (tsdf, weight, color) and the colours and cover of the kept mesh's
    vertices; computed once per process"""
    if not _SPHERE:
        case = sphere_case()
        rgb = np.stack([sphere_rgb(M, d, case["k"]) for M, d in zip(case["c2w"], case["depth"])])
        tsdf, weight, color = integrate(*T.fresh(T.SPHERE_SHAPE), fresh_color(T.SPHERE_SHAPE), T.SPHERE_LO,
                                        T.SPHERE_HI, case["depth"], rgb, case["c2w"], *case["k"], case["trunc"])
        vert_rgb, vert_cover = sample(color, T.SPHERE_LO, T.SPHERE_HI, case["kept"][0])
        for a in (rgb, tsdf, weight, color, vert_rgb, vert_cover):
            a.setflags(write=False)
        _SPHERE.update(case, rgb=rgb, tsdf_c=tsdf, weight_c=weight, color=color, vert_rgb=vert_rgb,
                       vert_cover=vert_cover)
    return _SPHERE
