"""The numpy restatement of the TSDF rule (tests/tsdf_reference.py) against properties that do not
depend on it: closed-form values on a camera's axis, and the sphere case, where the fused field's zero level must be
the sphere to within a voxel once the filter has removed the sheet at -trunc behind it.  CPU only.

A CPU prototype of the sphere case (same rule; face-to-cell by centroid, another camera roll) gave, with h = 0.087, a
largest kept error of 0.038 = 0.43 h and a largest unfiltered error of 0.31 = 3.6 h; the bounds here are h and 2 h."""
import numpy as np
import torch

import mesh_reference as MR
import tsdf_reference as T

F32 = np.float32


def test_axis_camera_constant_depth():
    """camera at (0,0,4) looking at the origin, depth 3.4 everywhere: on the optical axis r = 4 - z"""
    from nerf_amd.scene import look_at
    shape, lo, hi = (9, 9, 17), (-1.0, -1.0, -1.5), (1.0, 1.0, 6.5)  # z reaches past the camera
    c2w = look_at(torch.tensor([0.0, 0.0, 4.0]), up=(0.0, 1.0, 0.0)).numpy()
    assert np.array_equal(c2w, np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 4]], F32))
    H = W = 8
    depth = np.full((H, W), 3.4, F32)
    trunc = F32(0.75)
    f = 4.0  # the image covers |x| < z_c: the lattice's x = +-1 columns leave it near the camera
    tsdf, weight = T.integrate(*T.fresh(shape), lo, hi, depth, c2w, f, f, W / 2.0, H / 2.0, trunc)
    x = T.lattice(shape, lo, hi)
    z = x[4, 4, :, 2]
    assert x[4, 4, 0, 0] == 0 and x[4, 4, 0, 1] == 0  # the axis column
    seen = 0
    for iz in range(shape[2]):
        r = F32(4.0) - z[iz]
        s = F32(3.4) - r
        if r > 0 and s / trunc >= -1:
            want = min(F32(1), s / trunc)
            assert tsdf[4, 4, iz] == want and weight[4, 4, iz] == 1, (iz, tsdf[4, 4, iz], want)
            seen += 1
        else:
            assert tsdf[4, 4, iz] == 1 and weight[4, 4, iz] == 0, iz
    assert seen >= 5 and (tsdf[4, 4] < 0).any() and (tsdf[4, 4] == 1).any()
    behind = x[..., 2] >= 4.0
    assert behind.any() and (weight[behind] == 0).all() and (tsdf[behind] == 1).all()
    # outside the image: |x| / (4 - z) >= 1 or |y| / (4 - z) >= 1 in front of the camera
    zc = 4.0 - x[..., 2].astype(np.float64)
    outside = (zc > 0) & ((np.abs(x[..., 0]) > 1.001 * zc) | (np.abs(x[..., 1]) > 1.001 * zc))
    assert outside.any() and (weight[outside] == 0).all() and (tsdf[outside] == 1).all()
    # a second view accumulates: the same view twice leaves tsdf (t + t) / 2 = t and weight 2 where it was seen
    t2, w2 = T.integrate(tsdf, weight, lo, hi, depth, c2w, f, f, W / 2.0, H / 2.0, trunc)
    assert np.array_equal(w2, 2 * weight) and np.array_equal(t2, tsdf)


def test_depth_values_that_see_nothing():
    from nerf_amd.scene import look_at
    shape, lo, hi = (3, 3, 5), (-0.1, -0.1, -1.0), (0.1, 0.1, 1.0)
    c2w = look_at(torch.tensor([0.0, 0.0, 4.0]), up=(0.0, 1.0, 0.0)).numpy()
    for bad in (np.inf, -np.inf, np.nan, 0.0, -3.0):
        tsdf, weight = T.integrate(*T.fresh(shape), lo, hi, np.full((1, 1), bad, F32), c2w, 1.0, 1.0, 0.5, 0.5, 0.5)
        assert (weight == 0).all() and (tsdf == 1).all(), bad
    tsdf, weight = T.integrate(*T.fresh(shape), lo, hi, np.full((1, 1), 5.0, F32), c2w, 1.0, 1.0, 0.5, 0.5, 0.5)
    assert (weight[1, 1] == 1).all()  # r = 4 - z is in [3, 5] on the axis: s >= 0


def test_batch_equals_sequence():
    case = T.sphere_case()
    c2w, depth, k, trunc = case["c2w"][:3], case["depth"][:3], case["k"], case["trunc"]
    shape, lo, hi = T.SPHERE_SHAPE, T.SPHERE_LO, T.SPHERE_HI
    a = T.integrate(*T.fresh(shape), lo, hi, depth, c2w, *k, trunc)
    b = T.fresh(shape)
    for i in range(3):
        b = T.integrate(*b, lo, hi, depth[i], c2w[i], *k, trunc)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])
    assert a[1].max() >= 2


def test_sphere_volume():
    case = T.sphere_case()
    assert case["c2w"].shape == (14, 3, 4) and case["depth"].shape == (14, 48, 48)
    hit = np.isfinite(case["depth"])
    assert 0.05 < hit.mean() < 0.5 and (case["depth"][hit] > 3.3).all() and (case["depth"][hit] < 4.0).all()
    tsdf, weight = case["tsdf"], case["weight"]
    assert tsdf.dtype == F32 and weight.dtype == F32 and tsdf.shape == T.SPHERE_SHAPE
    assert tsdf.max() == 1 and tsdf.min() >= -1 and weight.max() <= 14 and weight.min() == 0
    x = T.lattice(T.SPHERE_SHAPE, T.SPHERE_LO, T.SPHERE_HI).astype(np.float64)
    r = np.linalg.norm(x, axis=-1)
    h = T.sphere_h()
    # The looked-up pixel's ray passes within half a pixel diagonal of the voxel: 0.71 * 3.9 / 66.7 = 0.042 < h / 2.
    # So for a voxel more than h inside the sphere, the point of that ray at the voxel's range is inside too, the ray
    # has hit the sphere before it, and every view that updates the voxel does so with s < 0 ...
    inside = (r < T.SPHERE_R - h) & (weight > 0)
    assert inside.sum() > 200 and (tsdf[inside] < 0).all()
    # ... and one more than trunc + h inside lies more than trunc behind that hit: hidden from every camera
    assert (weight[r < T.SPHERE_R - case["trunc"] - h] == 0).all()
    # in front of the sphere towards a camera: free space, t = 1 from every view that sees it
    assert tsdf[23, 12, 12] == 1 and weight[23, 12, 12] >= 1


def test_sphere_extraction():
    case = T.sphere_case()
    h = T.sphere_h()
    (v, f), (v_all, f_all), keep = case["kept"], case["full"], case["keep"]
    assert 0 < len(f) < len(f_all) and keep.sum() == len(f)
    assert MR.is_closed(f)
    err, err_all = T.sphere_errors(v), T.sphere_errors(v_all)
    print(f"h = {h:.4f}: kept max error {err.max():.4f} = {err.max() / h:.2f} h, "
          f"unfiltered {err_all.max():.4f} = {err_all.max() / h:.2f} h, faces {len(f)} of {len(f_all)}")
    assert err.max() < h
    assert err_all.max() > 2 * h  # the sheet at -trunc behind the surface
    vol = MR.signed_volume(v, f)
    assert abs(vol - 4.0 / 3.0 * np.pi * T.SPHERE_R ** 3) < 0.15 * vol and vol > 0  # outward normals


def test_face_ranges_against_each_faces_own_cell():
    """the keep mask from face_off ranges equals one computed face by face from the cell that emitted the face"""
    shape = (5, 6, 7)
    field = MR.noise_field(shape, 3)
    lo, hi = (0.0, 0.0, 0.0), (4.0, 5.0, 6.0)  # unit spacing: a vertex's cell is the floor of its position
    v, f = MR.marching_tets(field, 0.0, lo, hi)
    off = T.face_offsets(field, 0.0)
    assert off[-1] == len(f) and (np.diff(off) <= 12).all() and (np.diff(off) >= 0).all()
    weight = np.random.default_rng(5).choice([0, 1, 2], size=shape, p=[0.1, 0.45, 0.45]).astype(F32)
    for mw in (0, 1, 2):
        keep = T.face_observed(off, weight, mw)
        brute = np.zeros(len(f), np.uint8)
        for i, tri in enumerate(f):
            # the face's cell: every vertex lies on an edge of it, so the low corner is the floor of the smallest
            # coordinates, clamped into the cells (a vertex exactly on a lattice point does not occur in noise)
            c = np.floor(v[tri].min(0)).astype(int)
            c = np.minimum(c, np.array(shape) - 2)
            brute[i] = T.cell_observed(weight, *c, mw)
        assert np.array_equal(keep, brute), mw
        print(f"min_weight {mw}: {int(keep.sum())} of {len(f)} faces kept")
        assert (keep == 1).all() if mw == 0 else keep.sum() < len(f)
        assert mw != 1 or keep.sum() > 0
