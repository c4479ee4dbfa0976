"""kernels.tsdf_integrate_color / tsdf_sample_color (csrc/tsdf.hip), TSDFVolume(color=True),
ray_rendering.fuse_depth_views(colors=True) and InstantNGP.extract_mesh_tsdf(colors="fused") on the device (-m gpu),
against the numpy restatement of the two rules in tests/tsdf_color_reference.py.

Everything is compared bitwise, as in test_gpu_tsdf.py and for its reasons: tsdf.o is built with -ffp-contract=off and
both sides round every fp32 operation once.  The geometry, the helpers and the model are test_gpu_tsdf.py's.  The
entry point hands the colour kernel CAP views per launch: the launch-edge case runs CAP, CAP + 1 and 4 CAP + 1 views.
Lattices stay at 2010 points except the 24^3 sphere case, whose reference is computed once per process."""
import math

import numpy as np
import pytest
import torch

import mesh_reference as MR
import mesh_smooth_reference as MS
import test_gpu_tsdf as G
import tsdf_color_reference as TC
import tsdf_reference as T
from test_gpu_tsdf import model  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = np.float32
SHAPE, LO, HI = G.SHAPE, G.LO, G.HI
NAN, INF = G.NAN, G.INF
CAP = 8  # COLOR_VIEWS_PER_LAUNCH of csrc/tsdf.hip
_dev, _bits, _same = G._dev, G._bits, G._same


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from nerf_amd import kernels
    return kernels


def _run(K, vol, lo, hi, depth, rgb, c2w, k, trunc):
    """the device on copies of vol = (tsdf, weight, color) numpy arrays -> device tensors"""
    t, w, c = (_dev(a).clone() for a in vol)
    K.tsdf_integrate_color(t, w, c, lo, hi, _dev(np.asarray(depth, F32)), _dev(np.asarray(rgb, F32)),
                           _dev(np.asarray(c2w, F32)), *k, trunc)
    return t, w, c


def _fresh(shape):
    return (*T.fresh(shape), TC.fresh_color(shape))


def main_color_case():
    """test_gpu_tsdf.main_case with colours: uniform in [0,1), and at three pixels whose depth is valid in every view a
    NaN, a +inf and a -inf channel"""
    c2w, depth, k, trunc = G.main_case()
    rgb = np.random.default_rng(17).uniform(0.0, 1.0, depth.shape + (3,)).astype(F32)
    for v in range(3):
        rgb[v, 2, 3, 1], rgb[v, 1, 4, 0], rgb[v, 3, 1, 2] = NAN, INF, -INF
        assert np.isfinite(depth[v, [2, 1, 3], [3, 4, 1]]).all() and (depth[v, [2, 1, 3], [3, 4, 1]] > 0).all()
    return c2w, depth, rgb, k, trunc


def _color_pattern(shape, seed):
    """a used-looking colour volume: arbitrary colours, cw 0..3, and a NaN payload in r, g, b where cw = 0"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.0, 1.0, tuple(shape) + (4,)).astype(F32)
    c[..., 3] = rng.integers(0, 4, shape).astype(F32)
    cb = c.view(np.uint32)
    cb[c[..., 3] == 0, :3] = 0x7FC54321
    return c


# ------------------------------------------------------------------ the fusion rule


def test_main_case(K):
    c2w, depth, rgb, k, trunc = main_color_case()
    ref = TC.integrate(*_fresh(SHAPE), LO, HI, depth, rgb, c2w, *k, trunc)
    t, w, c = ref
    cw = c[..., 3]
    # the case reaches every branch of the colour rule: voxels some view clamped and another coloured, voxels updated
    # but never coloured, voxels coloured by several views, and updates inside the band whose pixel is not finite
    assert ((w > cw) & (cw > 0)).any() and ((cw == 0) & (w > 0)).any() and (cw >= 2).any() and (w == 0).any()
    clean = np.where(np.isfinite(rgb), rgb, F32(0.5))
    cw_clean = TC.integrate(*_fresh(SHAPE), LO, HI, depth, clean, c2w, *k, trunc)[2][..., 3]
    assert (cw_clean >= cw).all() and (cw_clean > cw).any()
    assert (c[cw == 0] == 0).all() and np.isfinite(c).all()
    plain = T.integrate(*T.fresh(SHAPE), LO, HI, depth, c2w, *k, trunc)
    assert np.array_equal(_bits(t), _bits(plain[0])) and np.array_equal(_bits(w), _bits(plain[1]))
    got = _run(K, _fresh(SHAPE), LO, HI, depth, rgb, c2w, k, trunc)
    _same(got, ref)
    # tsdf and weight are the plain kernel's on the device too
    _same(G._run(K, T.fresh(SHAPE), LO, HI, depth, c2w, k, trunc), [x.cpu().numpy() for x in got[:2]])


def test_minimum_lattice(K):
    c2w = G._look((0.0, 0.0, 3.0), up=(0.0, 1.0, 0.0))
    lo, hi = (-0.1, -0.1, -0.1), (0.1, 0.1, 0.1)
    depth = np.full((1, 1, 1), 3.0, F32)
    rgb = np.array([[[[0.2, 0.4, 0.6]]]], F32)
    k = (1.0, 1.0, 0.5, 0.5)
    ref = TC.integrate(*_fresh((2, 2, 2)), lo, hi, depth, rgb, c2w, *k, 0.25)
    assert (ref[1] == 1).all() and (ref[2] == np.array([0.2, 0.4, 0.6, 1.0], F32)).all()
    _same(_run(K, _fresh((2, 2, 2)), lo, hi, depth, rgb, c2w, k, 0.25), ref)
    _same(_run(K, _fresh((2, 2, 2)), lo, hi, depth[0], rgb[0], c2w[None], k, 0.25), ref)  # (H,W), (H,W,3), (1,3,4)


@pytest.mark.parametrize("n", [CAP, CAP + 1, 4 * CAP + 1])
def test_views_across_launches(K, n):
    """CAP views per launch: a full launch, one view more, and four launches and one view; 3x3 pixels, cameras on a
    ring around the box.  A batch equals the reference and one-by-one integration, and accumulates on a used volume."""
    rng = np.random.default_rng(33)
    c2w = np.stack([G._look((3.0 * math.cos(a), 3.0 * math.sin(a), z), roll=r) for a, z, r in
                    zip(np.linspace(0.0, 6.0, n), rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n))])
    depth = rng.uniform(2.0, 3.6, (n, 3, 3)).astype(F32)
    depth[rng.uniform(size=depth.shape) < 0.15] = INF
    rgb = rng.uniform(0.0, 1.0, (n, 3, 3, 3)).astype(F32)
    rgb[rng.uniform(size=rgb.shape) < 0.05] = NAN
    k = (2.5, 2.0, 1.4, 1.6)
    ref = TC.integrate(*_fresh(SHAPE), LO, HI, depth, rgb, c2w, *k, 0.4)
    cw = ref[2][..., 3]
    assert cw.max() >= 4 and len(np.unique(cw)) > 3 and (cw < ref[1]).any() and ref[1].max() >= 6
    batch = _run(K, _fresh(SHAPE), LO, HI, depth, rgb, c2w, k, 0.4)
    _same(batch, ref)
    t, w, c = (_dev(a) for a in _fresh(SHAPE))
    for v in range(n):
        K.tsdf_integrate_color(t, w, c, LO, HI, _dev(depth[v]), _dev(rgb[v]), _dev(c2w[v]), *k, 0.4)
    _same((t, w, c), ref)
    # the same views in reverse onto the used volume
    ref2 = TC.integrate(*ref, LO, HI, depth[::-1], rgb[::-1], c2w[::-1], *k, 0.4)
    assert ref2[2][..., 3].max() > cw.max()
    K.tsdf_integrate_color(t, w, c, LO, HI, _dev(depth[::-1].copy()), _dev(rgb[::-1].copy()), _dev(c2w[::-1].copy()),
                           *k, 0.4)
    _same((t, w, c), ref2)


def test_untouched_voxels_keep_their_bits(K):
    c2w, depth, rgb, k, trunc = main_color_case()
    vol = (*G._pattern(SHAPE, 11), _color_pattern(SHAPE, 12))
    # no views: nothing changes
    _same(_run(K, vol, LO, HI, np.zeros((0, 5, 7), F32), np.zeros((0, 5, 7, 3), F32), np.zeros((0, 3, 4), F32), k,
               trunc), vol)
    # views that see nothing: nothing changes
    _same(_run(K, vol, LO, HI, np.full_like(depth, INF), rgb, c2w, k, trunc), vol)
    # one real view: what it does not colour keeps its bits, the NaN payloads among them
    ref = TC.integrate(*vol, LO, HI, depth[0], rgb[0], c2w[0], *k, trunc)
    kept = ref[2][..., 3] == vol[2][..., 3]
    updated = ref[1] != vol[1]
    assert kept.any() and (~kept).any() and (kept & (vol[2][..., 3] == 0)).any() and (kept & updated).any()
    got = _run(K, vol, LO, HI, depth[0], rgb[0], c2w[0], k, trunc)
    assert np.array_equal(_bits(got[1]), _bits(ref[1]))
    assert np.array_equal(_bits(got[0])[~updated], _bits(vol[0])[~updated])
    assert np.array_equal(_bits(got[2])[kept], _bits(vol[2])[kept])
    assert np.array_equal(_bits(got[2][..., 3]), _bits(ref[2][..., 3]))
    # a NaN payload that a view did touch stays NaN; its bits are the hardware's choice
    for g, r in ((got[0], ref[0]), (got[2], ref[2])):
        live = ~np.isnan(r)
        assert np.array_equal(np.isnan(g.cpu().numpy()), ~live)
        assert np.array_equal(_bits(g)[live], _bits(r)[live])


# ------------------------------------------------------------------ the sampling rule


def sample_case():
    """a colour volume with cw in 0..3 (one cell unobserved at all 8 corners) and 257 points: the special ones first
    -> color, points, the indices of the all-unobserved point and of the NaN point"""
    rng = np.random.default_rng(21)
    color = rng.uniform(0.0, 1.0, SHAPE + (4,)).astype(F32)  # arbitrary colours where cw = 0 too: they must not count
    color[..., 3] = rng.integers(0, 4, SHAPE).astype(F32)
    color[1:3, 1:3, 10:12, 3] = 0
    X = T.lattice(SHAPE, LO, HI)
    half = F32(0.5)
    pts = [X[0, 0, 0], X[4, 5, 66], X[2, 3, 30], X[4, 0, 66], X[0, 5, 1], X[3, 5, 65]]       # lattice points
    for i, j, m in ((0, 0, 0), (3, 4, 65), (2, 2, 33), (1, 4, 63)):
        for d in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):          # edges, face diagonals
            a, b = X[i, j, m], X[i + d[0], j + d[1], m + d[2]]
            pts.append(a + (b - a) * half)
            pts.append(a + (b - a) * F32(0.3))
    unobserved = len(pts)
    pts.append((X[1, 1, 10] + X[2, 2, 11]) * half)                                           # all 8 corners unobserved
    pts.append((X[2, 2, 11] + X[3, 3, 12]) * half)                                           # some unobserved
    lo, hi = np.asarray(LO, F32), np.asarray(HI, F32)
    for a in range(3):
        for side, out in ((lo, -1.0), (hi, 1.0)):
            p = rng.uniform(lo, hi).astype(F32)
            p[a] = side[a]
            pts.append(p.copy())                                                             # on a box face
            p[a] = side[a] + F32(out * 0.3)
            pts.append(p.copy())                                                             # outside it
    pts += [np.array([1e30, -1e30, 0.1], F32), np.array([INF, 0.0, -INF], F32), np.array([-0.7, 1.0, 2.0], F32)]
    nan_at = len(pts)
    pts.append(np.array([0.1, NAN, 0.2], F32))
    pts = np.stack(pts).astype(F32)
    inside = rng.uniform(lo, hi, (257 - len(pts), 3)).astype(F32)
    return color, np.concatenate([pts, inside]), unobserved, nan_at


def test_sample_case_reference():
    """the reference on the 257 points shows every case the device test relies on"""
    color, pts, unobserved, nan_at = sample_case()
    rgb, cover = TC.sample(color, LO, HI, pts)
    assert len(pts) == 257 and cover[unobserved] == 0 and cover[nan_at] == 0 and (rgb[[unobserved, nan_at]] == 0).all()
    assert (cover > 0).sum() > 240 and np.isfinite(rgb).all() and rgb.min() >= 0 and rgb.max() <= 1 + 1e-6
    on_lattice = pts[:6]
    idx = [(0, 0, 0), (4, 5, 66), (2, 3, 30), (4, 0, 66), (0, 5, 1), (3, 5, 65)]
    assert np.array_equal(on_lattice, np.stack([T.lattice(SHAPE, LO, HI)[i] for i in idx]))
    for p, i in enumerate(idx):
        # on a lattice point: that voxel alone, but for the rounding of g = (x - lo) / h, which lies within 2 ulp of
        # the index (at most 66 * 2^-22 = 1.6e-5 off) and gives the neighbours, cw <= 3 each, that share per axis
        assert abs(cover[p] - color[i][3]) < 3 * 3 * 1.6e-5, i
        if color[i][3] > 0:
            assert np.allclose(rgb[p], color[i][:3], atol=3 * 3 * 1.6e-5), i


@pytest.mark.parametrize("N", [1, 255, 256, 257])
def test_sample_color(K, N):
    color, pts, unobserved, nan_at = sample_case()
    pts = pts[::-1][:N] if N == 1 else pts[:N]  # the single point: a random one inside the box
    ref = TC.sample(color, LO, HI, pts)
    assert N == 1 or (ref[1][unobserved] == 0 and ref[1][nan_at] == 0 and (ref[1] > 0).sum() > N - 20)
    rgb, cover = K.tsdf_sample_color(_dev(color), LO, HI, _dev(pts))
    assert tuple(rgb.shape) == (N, 3) and tuple(cover.shape) == (N,)
    _same((rgb, cover), ref)


def test_sample_no_points(K):
    color = _dev(sample_case()[0])
    rgb, cover = K.tsdf_sample_color(color, LO, HI, torch.zeros((0, 3), device=DEV))
    assert tuple(rgb.shape) == (0, 3) and tuple(cover.shape) == (0,) and rgb.dtype == cover.dtype == torch.float32


# ------------------------------------------------------------------ TSDFVolume


@pytest.fixture(scope="module")
def sphere_volume(K):
    from nerf_amd import TSDFVolume
    case = TC.sphere_color_case()
    vol = TSDFVolume(T.SPHERE_LO, T.SPHERE_HI, 24, color=True)
    assert tuple(vol.color.shape) == (24, 24, 24, 4) and bool((vol.color == 0).all())
    for s in (slice(0, 8), slice(8, 14)):
        vol.integrate(_dev(case["depth"][s]), *case["k"], _dev(case["c2w"][s]), rgb=_dev(case["rgb"][s]))
    return vol


def test_volume_on_the_sphere(K, sphere_volume):
    from nerf_amd import TSDFVolume
    case = TC.sphere_color_case()
    vol = sphere_volume
    _same((vol.tsdf, vol.weight, vol.color), (case["tsdf"], case["weight"], case["color"]))
    plain = vol.extract_mesh(normals=None)
    mesh = vol.extract_mesh(normals=None, colors="fused")
    assert plain.colors is None and torch.equal(mesh.vertices, plain.vertices) and torch.equal(mesh.faces, plain.faces)
    assert np.array_equal(mesh.faces.cpu().numpy(), case["kept"][1])
    assert np.array_equal(_bits(mesh.vertices), _bits(case["kept"][0]))
    _same((mesh.colors,), (case["vert_rgb"],))  # every vertex is seen, so no colour is the fill
    rgb, seen = vol.sample_colors(mesh.vertices)
    assert bool(seen.all()) and seen.dtype == torch.bool and torch.equal(rgb, mesh.colors)
    # moved vertices: colours at the final positions, inside the range of what the volume observed
    moved = vol.extract_mesh(normals=None, colors="fused", simplify=2.5 * T.sphere_h(), smooth=3)
    V = moved.vertices.shape[0]
    assert 0 < V < mesh.vertices.shape[0] and tuple(moved.colors.shape) == (V, 3)
    assert bool(torch.isfinite(moved.colors).all())
    obs = vol.color[vol.color[..., 3] > 0][:, :3]
    assert bool((moved.colors >= obs.amin(0) - 4e-6).all()) and bool((moved.colors <= obs.amax(0) + 4e-6).all())
    # a point no view coloured: the fill, and seen says so
    rgb, seen = vol.sample_colors(torch.tensor([[0.0, 0.0, 0.0], [0.0, 0.0, 0.6]], device=DEV), fill=0.25)
    assert seen.tolist() == [False, True] and rgb[0].tolist() == [0.25] * 3
    # depth without rgb on a colour volume: the plain kernel, .color stays
    v2 = TSDFVolume(T.SPHERE_LO, T.SPHERE_HI, 24, color=True)
    v2.integrate(_dev(case["depth"]), *case["k"], _dev(case["c2w"]))
    _same((v2.tsdf, v2.weight), (case["tsdf"], case["weight"]))
    assert bool((v2.color == 0).all())
    v2.integrate(_dev(case["depth"][0]), *case["k"], _dev(case["c2w"][0]), rgb=_dev(case["rgb"][0]))
    assert float(v2.color[..., 3].max()) == 1
    v2.reset()
    assert bool((v2.color == 0).all()) and bool((v2.weight == 0).all()) and bool((v2.tsdf == 1).all())


def test_round_trip_through_the_ray_caster(K):
    """a closed mesh with vertex colours 0.5 + 0.4 v / |v|, rendered by Mesh.render from the 14 cameras at 48x48, its
    depth and colour fused at 24^3: every kept vertex was seen.  The colour error against the source's analytic colour
    is printed, not gated: the source's facets are about 2 h, and its colour is linear across each of them."""
    from nerf_amd import Mesh, TSDFVolume
    v, f, _ = MS.sphere_mesh(12)
    col = (0.5 + 0.4 * v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F32)
    src = Mesh(_dev(v), _dev(f), colors=_dev(col))
    case = T.sphere_case()
    n = T.SPHERE_HW
    views = [src.render(n, n, *case["k"], _dev(M)) for M in case["c2w"]]
    depth, rgb = torch.stack([r["depth"] for r in views]), torch.stack([r["color"] for r in views])
    vol = TSDFVolume(T.SPHERE_LO, T.SPHERE_HI, 24, color=True)
    vol.integrate(depth, *case["k"], _dev(case["c2w"]), rgb=rgb)
    out = vol.extract_mesh(normals=None, colors="fused")
    assert MR.is_closed(out.faces.cpu().numpy())
    _, seen = vol.sample_colors(out.vertices)
    assert out.vertices.shape[0] > 0 and bool(seen.all())
    p = out.vertices.double()
    want = 0.5 + 0.4 * p / p.norm(dim=1, keepdim=True)
    err = float((out.colors.double() - want).abs().max())
    print(f"round trip: max colour error {err:.4f} over {out.vertices.shape[0]} vertices "
          f"(one cell diagonal of gradient: {(0.4 / T.SPHERE_R) * math.sqrt(3.0) * T.sphere_h():.4f})")
    assert bool(torch.isfinite(out.colors).all())


# ------------------------------------------------------------------ a model


def test_model_extract_mesh_tsdf_fused(K, model):  # noqa: F811
    from nerf_amd.ray_rendering import fuse_depth_views
    from nerf_amd.scene import hemisphere_poses
    poses = hemisphere_poses(4, seed=0)
    n = 16
    focal = 0.5 * n / math.tan(0.5 * 0.6911112)
    cam = dict(H=n, W=n, fx=focal, fy=focal, cx=n / 2.0, cy=n / 2.0, near=2.0, far=6.0)
    kw = dict(resolution=16, ray_samples=32, batch=3)
    plain = fuse_depth_views(model, poses, lo=[-1.5] * 3, hi=[1.5] * 3, **cam, **kw)
    vol = fuse_depth_views(model, poses, lo=[-1.5] * 3, hi=[1.5] * 3, colors=True, **cam, **kw)
    assert plain.color is None and tuple(vol.color.shape) == (16, 16, 16, 4)
    assert torch.equal(vol.tsdf, plain.tsdf) and torch.equal(vol.weight, plain.weight)
    assert float(vol.color[..., 3].max()) >= 1 and bool((vol.color[..., 3] <= vol.weight).all())
    a = model.extract_mesh_tsdf(poses, **cam, colors="fused", **kw)
    b = model.extract_mesh_tsdf(poses, **cam, colors="fused", **kw)
    c = model.extract_mesh_tsdf(poses, **cam, **kw)
    assert a.vertices.shape[0] > 0 and tuple(a.colors.shape) == tuple(a.vertices.shape) and c.colors is None
    assert float(a.colors.min()) >= 0.0 and float(a.colors.max()) <= 1.0
    assert torch.equal(a.vertices, c.vertices) and torch.equal(a.faces, c.faces) and torch.equal(a.normals, c.normals)
    assert torch.equal(a.colors, b.colors) and torch.equal(a.vertices, b.vertices)
    assert torch.equal(a.colors, vol.extract_mesh(normals=None, colors="fused").colors)
    with pytest.raises(ValueError):
        model.extract_mesh_tsdf(poses, **cam, colors="rgb", **kw)


# ------------------------------------------------------------------ argument checks


def test_argument_checks(K):
    from nerf_amd import TSDFVolume
    c2w, depth, rgb, k, trunc = main_color_case()
    t, w, c = (_dev(a) for a in _fresh(SHAPE))
    d, r, M = _dev(depth), _dev(rgb), _dev(c2w)
    before = (t.clone(), w.clone(), c.clone())

    def bad(**kw):
        a = dict(tsdf=t, weight=w, color=c, lo=LO, hi=HI, depth=d, rgb=r, c2w=M, fx=k[0], fy=k[1], cx=k[2], cy=k[3],
                 trunc=trunc)
        a.update(kw)
        with pytest.raises(ValueError):
            K.tsdf_integrate_color(**a)

    bad(color=c.double())
    bad(color=c[..., :3].contiguous())
    bad(color=torch.zeros((5, 6, 66, 4), device=DEV))
    bad(color=torch.zeros(SHAPE, device=DEV))
    bad(color=torch.zeros(SHAPE + (8,), device=DEV)[..., ::2])
    bad(color=torch.zeros((4,) + SHAPE, device=DEV).permute(1, 2, 3, 0))
    bad(color=c.cpu())
    bad(rgb=r.half())
    bad(rgb=r[..., :2].contiguous())
    bad(rgb=r[:2])                                    # view-count mismatch
    bad(rgb=r[:, :4])                                 # H mismatch
    bad(rgb=r[0])                                     # (H,W,3) with (3,H,W) depth
    bad(rgb=d)
    bad(rgb=r.permute(0, 2, 1, 3))
    bad(rgb=torch.zeros((3, 5, 7, 6), device=DEV)[..., ::2])
    bad(rgb=r.cpu())
    bad(rgb=None)
    # tsdf_integrate's own checks hold here too
    bad(tsdf=t.double())
    bad(weight=torch.zeros((5, 6, 66), device=DEV))
    bad(depth=d[:2])
    bad(c2w=M[:1])
    bad(trunc=0.0)
    bad(fx=NAN)
    bad(lo=(0.0, 2.0, 0.0), hi=(1.0, 1.0, 1.0))
    nan_M = M.clone()
    nan_M[1, 2, 3] = NAN
    bad(c2w=nan_M)
    assert all(torch.equal(x, y) for x, y in zip((t, w, c), before))  # nothing was launched

    pts = torch.zeros((4, 3), device=DEV)
    for args in ((c.double(), LO, HI, pts), (c[..., :3].contiguous(), LO, HI, pts), (t, LO, HI, pts),
                 (torch.zeros(SHAPE + (8,), device=DEV)[..., ::2], LO, HI, pts), (c.cpu(), LO, HI, pts),
                 (torch.zeros((1, 6, 67, 4), device=DEV), LO, HI, pts), (c, LO, HI, pts.double()),
                 (c, LO, HI, pts[:, :2].contiguous()), (c, LO, HI, torch.zeros((4, 6), device=DEV)[:, ::2]),
                 (c, LO, HI, pts.reshape(-1)), (c, LO, HI, pts.cpu()), (c, HI, LO, pts), (c, LO[:2], HI, pts)):
        with pytest.raises(ValueError):
            K.tsdf_sample_color(*args)

    plain = TSDFVolume(LO, HI, SHAPE)
    assert plain.color is None
    with pytest.raises(ValueError):
        plain.integrate(d, *k, M, rgb=r)
    with pytest.raises(ValueError):
        plain.extract_mesh(colors="fused")
    with pytest.raises(ValueError):
        plain.sample_colors(pts)
    assert bool((plain.weight == 0).all()) and bool((plain.tsdf == 1).all())
    with_color = TSDFVolume(LO, HI, SHAPE, color=True)
    with pytest.raises(ValueError):
        with_color.extract_mesh(colors="linear")
    with pytest.raises(ValueError):
        with_color.integrate(d, *k, M, rgb=rgb)  # a numpy array
    assert bool((with_color.color == 0).all()) and bool((with_color.weight == 0).all())
