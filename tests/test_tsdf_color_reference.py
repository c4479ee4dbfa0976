"""The numpy restatement of the TSDF colour rules (tests/tsdf_color_reference.py) on the sphere case of
tests/tsdf_reference.py: 24^3 voxels, 14 views of 48x48, every view coloured 0.5 + 0.4 p / R at its hit point p and 0
on a miss.  CPU only.

The fused colour of a vertex is a mean of pixel colours whose hit points lie within about a cell of it, so it stays
within one cell diagonal of colour gradient of the analytic colour at the vertex's radial projection:
(0.4 / 0.6) sqrt(3) h = 0.100.  A numpy prototype of these rules gave 0 unseen vertices of 2858, a smallest cover of
3.5, a largest error of 0.033, colour updates on 23 % of the voxels and plain updates on 74 %."""
import numpy as np

import tsdf_color_reference as TC
import tsdf_reference as T

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_tsdf_and_weight_are_the_plain_rule():
    case = TC.sphere_color_case()
    assert np.array_equal(_bits(case["tsdf_c"]), _bits(case["tsdf"]))
    assert np.array_equal(_bits(case["weight_c"]), _bits(case["weight"]))
    # on a used volume and one view at a time too
    shape, lo, hi = T.SPHERE_SHAPE, T.SPHERE_LO, T.SPHERE_HI
    a = (case["tsdf"], case["weight"])
    b = (case["tsdf"], case["weight"], case["color"])
    for i in (0, 9):
        a = T.integrate(*a, lo, hi, case["depth"][i], case["c2w"][i], *case["k"], case["trunc"])
        b = TC.integrate(*b, lo, hi, case["depth"][i], case["rgb"][i], case["c2w"][i], *case["k"], case["trunc"])
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    assert (b[2][..., 3] >= case["color"][..., 3]).all() and (b[2][..., 3] > case["color"][..., 3]).any()


def test_colour_stays_in_the_band():
    case = TC.sphere_color_case()
    weight, color = case["weight"], case["color"]
    cw = color[..., 3]
    assert cw.dtype == F32 and (cw <= weight).all() and (cw == np.floor(cw)).all()
    assert (color[cw == 0] == 0).all()  # written only where a view coloured the voxel
    share_c, share_w = float((cw > 0).mean()), float((weight > 0).mean())
    print(f"colour updates on {share_c:.1%} of the voxels, plain updates on {share_w:.1%}")
    assert 0.1 < share_c < 0.4 < share_w
    # a coloured voxel lies within trunc (+ half a pixel's reach) of the sphere; its colour is a mean of surface colours
    r = np.linalg.norm(T.lattice(T.SPHERE_SHAPE, T.SPHERE_LO, T.SPHERE_HI).astype(np.float64), axis=-1)
    assert (np.abs(r[cw > 0] - T.SPHERE_R) < case["trunc"] + T.sphere_h()).all()
    seen = color[cw > 0][:, :3]
    assert seen.min() >= 0.1 - 1e-6 and seen.max() <= 0.9 + 1e-6  # no miss pixel's 0 was averaged in


def test_vertex_colours_on_the_sphere():
    case = TC.sphere_color_case()
    v = case["kept"][0].astype(np.float64)
    rgb, cover = case["vert_rgb"], case["vert_cover"]
    assert rgb.shape == (len(v), 3) and cover.shape == (len(v),) and rgb.dtype == F32 and cover.dtype == F32
    want = TC.sphere_color_at(v / np.linalg.norm(v, axis=-1, keepdims=True) * T.SPHERE_R)
    err = np.abs(rgb - want).max()
    bound = (0.4 / T.SPHERE_R) * np.sqrt(3.0) * T.sphere_h()
    print(f"{int((cover <= 0).sum())} unseen vertices of {len(v)}, min cover {cover.min():.2f}, "
          f"max colour error {err:.4f}, bound {bound:.4f}")
    assert (cover > 0).all()
    assert err < bound


def test_sampling_rule_by_hand():
    """one cell, colours and weights chosen so that the weighted mean is known in closed form"""
    color = np.zeros((2, 2, 2, 4), F32)
    color[0, 0, 0] = (1.0, 0.0, 0.5, 1.0)
    color[1, 0, 0] = (0.0, 1.0, 0.5, 3.0)
    color[0, 1, 1] = (9.0, 9.0, 9.0, 0.0)  # cw = 0: ignored whatever it holds
    lo, hi = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    pts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.25, 0.5, 0.5], [0.0, 1.0, 1.0],
                    [-3.0, -1.0, 0.0], [2.0, 0.0, -5.0], [np.nan, 0.0, 0.0], [1.0, 1.0, 1.0]], F32)
    rgb, cover = TC.sample(color, lo, hi, pts)
    assert np.array_equal(cover, np.array([1, 3, 2, 0.375, 0, 1, 3, 0, 0], F32))
    assert np.array_equal(rgb[0], color[0, 0, 0, :3]) and np.array_equal(rgb[1], color[1, 0, 0, :3])
    assert np.array_equal(rgb[2], np.array([0.25, 0.75, 0.5], F32))  # (0.5 * 1 * c0 + 0.5 * 3 * c1) / 2
    assert np.array_equal(rgb[3], np.array([0.5, 0.5, 0.5], F32))  # k = 0.1875 from each of the two
    assert np.array_equal(rgb[5], rgb[0]) and np.array_equal(rgb[6], rgb[1])  # clamped onto the box
    assert (rgb[[4, 7, 8]] == 0).all()


def test_fusion_rule_by_hand():
    """one voxel column under an axis camera: the colour is taken inside the band only, and only from finite pixels"""
    import torch
    from nerf_amd.scene import look_at
    shape, lo, hi = (3, 3, 9), (-0.1, -0.1, -1.0), (0.1, 0.1, 1.0)
    c2w = look_at(torch.tensor([0.0, 0.0, 4.0]), up=(0.0, 1.0, 0.0)).numpy()
    depth = np.full((1, 1), 4.0, F32)  # the surface at z = 0 on the axis
    trunc = F32(0.5)
    cam = (1.0, 1.0, 0.5, 0.5)
    vol = (*T.fresh(shape), TC.fresh_color(shape))
    red, blue = np.array([[[1.0, 0.0, 0.0]]], F32), np.array([[[0.0, 0.0, 1.0]]], F32)
    t, w, c = TC.integrate(*vol, lo, hi, depth, red, c2w, *cam, trunc)
    z = T.lattice(shape, lo, hi)[1, 1, :, 2]
    band = (z > -0.5 - 1e-6) & (z < 0.5 - 1e-6)  # s = z: -trunc <= s and s / trunc < 1
    assert band.sum() == 4 and np.array_equal(c[1, 1, :, 3], band.astype(F32))
    assert (w[1, 1][z >= -0.5] == 1).all() and (w[1, 1] >= c[1, 1, :, 3]).all() and (w[1, 1] > c[1, 1, :, 3]).any()
    assert (c[1, 1, band, :3] == red[0, 0]).all() and (c[1, 1, ~band] == 0).all()
    t2, w2, c2 = TC.integrate(t, w, c, lo, hi, depth, blue, c2w, *cam, trunc)
    assert (c2[1, 1, band] == np.array([0.5, 0.0, 0.5, 2.0], F32)).all() and (w2 == 2 * w).all()
    for bad in (np.nan, np.inf, -np.inf):
        px = blue.copy()
        px[0, 0, 1] = bad
        t3, w3, c3 = TC.integrate(t, w, c, lo, hi, depth, px, c2w, *cam, trunc)
        assert np.array_equal(c3, c) and np.array_equal(w3, w2) and np.array_equal(t3, t2)
