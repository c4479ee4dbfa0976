"""kernels.tsdf_integrate / tsdf_face_observed (csrc/tsdf.hip), mesh_extract(face_offsets=True), TSDFVolume,
ray_rendering.fuse_depth_views and InstantNGP.extract_mesh_tsdf on the device (-m gpu), against the numpy restatement
of the rule in tests/tsdf_reference.py.

tsdf and weight are compared bitwise (np.array_equal on the uint32 views): tsdf.o is built with -ffp-contract=off, the
rule is fp32 with every operation rounded once on both sides, and the fp32 divide and sqrt are the correctly rounded
ones on both sides.  The entry point hands the kernel 8 views per launch: the chunk-edge case runs 8, 9 and 33 views.
Lattices stay at 2010 points except the 24^3 sphere case, whose reference is computed once per process."""
import math

import numpy as np
import pytest
import torch

import mesh_reference as MR
import mesh_smooth_reference as MS
import tsdf_reference as T

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = np.float32
SHAPE = (5, 6, 67)  # 2010 voxels: no multiple of 64 or 256, and the iz axis crosses a wave
LO, HI = (-0.5, -0.75, -1.5), (0.5, 0.75, 1.5)
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from nerf_amd import kernels
    return kernels


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)  # a copy: the shared reference arrays are read-only


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same(got, ref):
    for g, r in zip(got, ref):
        assert g.dtype == torch.float32 and tuple(g.shape) == tuple(r.shape)
        assert np.array_equal(_bits(g), _bits(r)), int((_bits(g) != _bits(r)).sum())


def _run(K, vol, lo, hi, depth, c2w, k, trunc):
    """the device on copies of vol = (tsdf, weight) numpy arrays -> device tensors"""
    t, w = _dev(vol[0]).clone(), _dev(vol[1]).clone()
    K.tsdf_integrate(t, w, lo, hi, _dev(np.asarray(depth, F32)), _dev(np.asarray(c2w, F32)), *k, trunc)
    return t, w


def _look(pos, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0), roll=0.0):
    from nerf_amd.scene import look_at
    M = look_at(torch.tensor(pos, dtype=torch.float64), target=target, up=up).numpy().astype(np.float64)
    c, s = math.cos(roll), math.sin(roll)
    R = M[:, :3] @ np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return np.concatenate([R, M[:, 3:]], 1).astype(F32)


def main_case():
    """3 views of 7x5 pixels (H = 5, W = 7), fx != fy, the principal point off centre: a camera outside the box, one
    inside it (voxels behind it and at zc near 0), one rolled.  The depth entries include +inf, NaN, 0, a negative
    value, and ranges that put voxels on both sides of -trunc and of t = 1."""
    c2w = np.stack([_look((0.3, -0.2, 4.0), up=(0.0, 1.0, 0.0)),
                    _look((0.1, 0.05, 0.2), target=(0.0, 0.3, -1.0), up=(0.0, 1.0, 0.0)),
                    _look((2.5, 1.5, 1.0), roll=0.7)])
    H, W = 5, 7
    k = (9.0, 6.5, 3.2, 2.7)
    rng = np.random.default_rng(7)
    depth = np.stack([rng.uniform(3.0, 5.0, (H, W)), rng.uniform(0.2, 1.5, (H, W)), rng.uniform(2.0, 4.0, (H, W))])
    depth = depth.astype(F32)
    for v in range(3):
        depth[v, 0, 0], depth[v, 1, 2], depth[v, 2, 1], depth[v, 4, 6], depth[v, 3, 3] = INF, NAN, 0.0, -1.5, -INF
    return c2w, depth, k, 0.3


def _pattern(shape, seed):
    """a used-looking volume: arbitrary tsdf bits, weights 0..3, and a NaN payload in tsdf where weight = 0"""
    rng = np.random.default_rng(seed)
    t = rng.uniform(-1.0, 1.0, shape).astype(F32)
    w = rng.integers(0, 4, shape).astype(F32)
    tb = t.view(np.uint32)
    tb[w == 0] = 0x7FC12345
    return t, w


# ------------------------------------------------------------------ the rule


def test_main_case(K):
    c2w, depth, k, trunc = main_case()
    ref = T.integrate(*T.fresh(SHAPE), LO, HI, depth, c2w, *k, trunc)
    t, w = ref
    # the case reaches every branch: untouched and touched voxels, t clamped to 1 and t < 0, several views on one voxel
    assert (w == 0).any() and (w >= 2).any() and (t == 1).any() and (t < 0).any() and ((t > 0) & (t < 1)).any()
    for v in range(3):  # every view updates some voxels and leaves some alone
        one = T.integrate(*T.fresh(SHAPE), LO, HI, depth[v], c2w[v], *k, trunc)[1]
        assert 0 < one.sum() < one.size, v
    _same(_run(K, T.fresh(SHAPE), LO, HI, depth, c2w, k, trunc), ref)


def test_minimum_lattice(K):
    c2w = _look((0.0, 0.0, 3.0), up=(0.0, 1.0, 0.0))
    lo, hi = (-0.1, -0.1, -0.1), (0.1, 0.1, 0.1)
    depth = np.full((1, 1, 1), 3.0, F32)
    k = (1.0, 1.0, 0.5, 0.5)
    ref = T.integrate(*T.fresh((2, 2, 2)), lo, hi, depth, c2w, *k, 0.25)
    assert (ref[1] == 1).all() and (ref[0] < 1).any()
    _same(_run(K, T.fresh((2, 2, 2)), lo, hi, depth, c2w, k, 0.25), ref)
    _same(_run(K, T.fresh((2, 2, 2)), lo, hi, depth[0], c2w[None], k, 0.25), ref)  # (H,W) with (1,3,4)


def test_batch_equals_sequence_and_accumulates(K):
    c2w, depth, k, trunc = main_case()
    batch = _run(K, T.fresh(SHAPE), LO, HI, depth, c2w, k, trunc)
    t, w = _dev(T.fresh(SHAPE)[0]), _dev(T.fresh(SHAPE)[1])
    for v in range(3):
        M = np.concatenate([c2w[v], [[0, 0, 0, 1]]]).astype(F32) if v == 1 else c2w[v]  # (4,4) too
        K.tsdf_integrate(t, w, LO, HI, _dev(depth[v]), _dev(M), *k, trunc)
    _same((t, w), [x.cpu().numpy() for x in batch])
    # a second integrate on the used volume accumulates
    ref = T.integrate(*T.fresh(SHAPE), LO, HI, depth, c2w, *k, trunc)
    ref2 = T.integrate(*ref, LO, HI, depth[::-1], c2w[::-1], *k, trunc)
    assert ref2[1].max() > ref[1].max()
    K.tsdf_integrate(t, w, LO, HI, _dev(depth[::-1].copy()), _dev(c2w[::-1].copy()), *k, trunc)
    _same((t, w), ref2)


@pytest.mark.parametrize("n", [8, 9, 33])
def test_views_across_launches(K, n):
    """8 views per launch: a full launch, one view more, and four launches and one view; 3x3 pixels, cameras on a ring
    around the box"""
    rng = np.random.default_rng(33)
    c2w = np.stack([_look((3.0 * math.cos(a), 3.0 * math.sin(a), z), roll=r) for a, z, r in
                    zip(np.linspace(0.0, 6.0, n), rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n))])
    depth = rng.uniform(2.0, 3.6, (n, 3, 3)).astype(F32)
    depth[rng.uniform(size=depth.shape) < 0.15] = INF
    k = (2.5, 2.0, 1.4, 1.6)
    ref = T.integrate(*T.fresh(SHAPE), LO, HI, depth, c2w, *k, 0.4)
    assert ref[1].max() >= 6 and len(np.unique(ref[1])) > 3
    _same(_run(K, T.fresh(SHAPE), LO, HI, depth, c2w, k, 0.4), ref)


def test_untouched_voxels_keep_their_bits(K):
    c2w, depth, k, trunc = main_case()
    vol = _pattern(SHAPE, 11)
    # no views: nothing changes
    _same(_run(K, vol, LO, HI, np.zeros((0, 5, 7), F32), np.zeros((0, 3, 4), F32), k, trunc), vol)
    # views that see nothing: nothing changes
    blind = np.full_like(depth, INF)
    _same(_run(K, vol, LO, HI, blind, c2w, k, trunc), vol)
    # one real view: the voxels it does not touch keep their bits, the NaN payloads among them
    ref = T.integrate(*vol, LO, HI, depth[0], c2w[0], *k, trunc)
    untouched = ref[1] == vol[1]
    assert untouched.any() and (~untouched).any() and (untouched & (vol[1] == 0)).any()
    got = _run(K, vol, LO, HI, depth[0], c2w[0], k, trunc)
    assert np.array_equal(_bits(got[0])[untouched], _bits(vol[0])[untouched])
    assert np.array_equal(_bits(got[1]), _bits(ref[1]))
    live = ~np.isnan(ref[0])  # a NaN payload that a view did touch stays NaN; its bits are the hardware's choice
    assert np.array_equal(np.isnan(got[0].cpu().numpy()), ~live)
    assert np.array_equal(_bits(got[0])[live], _bits(ref[0])[live])


def test_argument_checks(K):
    c2w, depth, k, trunc = main_case()
    t, w = (_dev(a) for a in T.fresh(SHAPE))
    d, M = _dev(depth), _dev(c2w)
    before = (t.clone(), w.clone())

    def bad(**kw):
        a = dict(tsdf=t, weight=w, lo=LO, hi=HI, depth=d, c2w=M, fx=k[0], fy=k[1], cx=k[2], cy=k[3], trunc=trunc)
        a.update(kw)
        with pytest.raises(ValueError):
            K.tsdf_integrate(**a)

    bad(tsdf=t.double())
    bad(weight=w.to(torch.int32))
    bad(depth=d.half())
    bad(c2w=M.double())
    bad(weight=torch.zeros((5, 6, 66), device=DEV))
    bad(tsdf=torch.ones((5, 6), device=DEV), weight=torch.zeros((5, 6), device=DEV))
    bad(tsdf=torch.ones((1, 6, 67), device=DEV), weight=torch.zeros((1, 6, 67), device=DEV))
    bad(tsdf=torch.ones((5, 6, 134), device=DEV)[:, :, ::2], weight=torch.zeros((5, 6, 134), device=DEV)[:, :, ::2])
    bad(depth=d[:, :, ::2])
    bad(depth=d[:2])                       # view-count mismatch
    bad(c2w=M[:1])
    bad(depth=d[0], c2w=M)
    bad(c2w=M[:, :, :3])
    bad(depth=d.reshape(3, 5, 7, 1))
    nan_M = M.clone()
    nan_M[1, 2, 3] = NAN
    bad(c2w=nan_M)
    inf_M = M.clone()
    inf_M[0, 0, 0] = INF
    bad(c2w=inf_M)
    for name in ("trunc", "fx", "fy"):
        for v in (0.0, -1.0, NAN, INF, 1e39, 1e-50):  # the last two are inf and 0 in fp32
            bad(**{name: v})
    for name in ("cx", "cy"):
        for v in (NAN, INF, -INF):
            bad(**{name: v})
    bad(lo=(0.0, 0.0, 0.0), hi=(1.0, 0.0, 1.0))
    bad(lo=(0.0, 2.0, 0.0), hi=(1.0, 1.0, 1.0))
    bad(lo=(0.0, 0.0), hi=(1.0, 1.0))
    with pytest.raises(ValueError, match="no CPU fallback"):
        K.tsdf_integrate(t.cpu(), w.cpu(), LO, HI, d.cpu(), M.cpu(), *k, trunc)
    bad(depth=d.cpu())
    bad(c2w=M.cpu())
    assert torch.equal(t, before[0]) and torch.equal(w, before[1])  # nothing was launched
    wt = _dev(np.zeros(SHAPE, F32))
    off = torch.zeros(2011, dtype=torch.int32, device=DEV)
    for args in ((off[:-1], wt, 1), (off.long(), wt, 1), (off, wt[:, :, :66], 1), (off, wt, NAN), (off.cpu(), wt, 1),
                 (off, wt.cpu(), 1), (off + 2 ** 30, wt, 1)):
        with pytest.raises(ValueError):
            K.tsdf_face_observed(*args)
    assert K.tsdf_face_observed(off, wt, 1).shape == (0,)


# ------------------------------------------------------------------ the face filter


@pytest.mark.parametrize("seed", [0, 1])
def test_face_offsets_and_filter(K, seed):
    field = MR.noise_field(SHAPE, seed)
    if seed == 1:  # the last cells of the lattice (and the first) hold 12 faces: every tetrahedron has two inside
        for ix, iy, iz in ((3, 4, 65), (0, 0, 0)):
            for c in range(8):
                field[ix + (c & 1), iy + ((c >> 1) & 1), iz + ((c >> 2) & 1)] = 0.5 if c in (0, 7) else -0.5
    ref_off = T.face_offsets(field, 0.1)
    if seed == 1:
        assert np.diff(ref_off).max() == 12
        p_last = (3 * 6 + 4) * 67 + 65
        assert ref_off[p_last + 1] - ref_off[p_last] == 12 and ref_off[p_last + 1] == ref_off[-1]
    fd = _dev(field)
    lo, hi = (0.0, -1.0, 2.0), (1.0, 1.5, 9.0)
    plain = K.mesh_extract(fd, 0.1, lo, hi)
    with_off = K.mesh_extract(fd, 0.1, lo, hi, face_offsets=True)
    with_nrm = K.mesh_extract(fd, 0.1, lo, hi, normals=True, face_offsets=True)
    assert len(plain) == 2 and len(with_off) == 3 and len(with_nrm) == 4
    assert all(torch.equal(a, b) for a, b in zip(plain, with_off))
    assert all(torch.equal(a, b) for a, b in zip(K.mesh_extract(fd, 0.1, lo, hi, normals=True), with_nrm))
    off = with_off[2]
    assert off.dtype == torch.int32 and tuple(off.shape) == (2011,) and torch.equal(off, with_nrm[3])
    assert np.array_equal(off.cpu().numpy(), ref_off) and int(off[-1]) == plain[1].shape[0]
    weight = np.random.default_rng(seed).choice([0, 1, 2], size=SHAPE, p=[0.1, 0.45, 0.45]).astype(F32)
    weight[1:3, 1:3, 10:12] = 2  # a cell that every min_weight keeps
    if seed == 1:
        weight[3:5, 4:6, 65:67] = 2
    for mw in (0, 1, 2):
        keep = K.tsdf_face_observed(off, _dev(weight), mw)
        ref = T.face_observed(ref_off, weight, mw)
        assert keep.dtype == torch.uint8 and np.array_equal(keep.cpu().numpy(), ref), mw
        assert ref.all() if mw == 0 else 0 < ref.sum() < len(ref)


# ------------------------------------------------------------------ TSDFVolume


@pytest.fixture(scope="module")
def sphere_volume(K):
    from nerf_amd import TSDFVolume
    case = T.sphere_case()
    vol = TSDFVolume(T.SPHERE_LO, T.SPHERE_HI, 24)
    assert vol.trunc == case["trunc"] and np.allclose(vol.spacing, T.sphere_h())
    assert bool((vol.tsdf == 1).all()) and bool((vol.weight == 0).all())
    vol.integrate(_dev(case["depth"][:8]), *case["k"], _dev(case["c2w"][:8]))
    vol.integrate(_dev(case["depth"][8:]), *case["k"], _dev(case["c2w"][8:]))
    return vol


def test_volume_on_the_sphere(K, sphere_volume):
    case = T.sphere_case()
    vol = sphere_volume
    _same((vol.tsdf, vol.weight), (case["tsdf"], case["weight"]))
    mesh = vol.extract_mesh(normals=None)
    v_ref, f_ref = case["kept"]
    v, f = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()
    assert np.array_equal(f, f_ref) and np.array_equal(_bits(v), _bits(v_ref))
    h = T.sphere_h()
    assert MR.is_closed(f)
    assert T.sphere_errors(v).max() < h
    full = vol.extract_mesh(min_weight=0, normals=None)
    assert np.array_equal(full.faces.cpu().numpy(), case["full"][1])
    assert np.array_equal(_bits(full.vertices), _bits(case["full"][0]))
    assert T.sphere_errors(full.vertices.cpu().numpy()).max() > 2 * h
    vol_ref = MR.signed_volume(v_ref, f_ref)
    assert vol_ref > 0 and abs(mesh.volume() - vol_ref) <= 1e-12 * vol_ref  # both are float64 sums over equal meshes
    # normals point outwards, and the options of mesh.extract_mesh apply
    with_n = vol.extract_mesh()
    assert torch.equal(with_n.vertices, mesh.vertices) and with_n.normals is not None
    cos = (with_n.normals * torch.nn.functional.normalize(with_n.vertices, dim=1)).sum(1)
    assert float(cos.mean()) > 0.5
    one = vol.extract_mesh(min_weight=0, normals=None, keep_largest=1, smooth=2)
    assert 0 < one.faces.shape[0] < full.faces.shape[0]
    with pytest.raises(ValueError):
        vol.extract_mesh(normals="field")
    with pytest.raises(ValueError):
        vol.extract_mesh(min_faces=1, keep_largest=1)
    # reset gives a fresh volume
    from nerf_amd import TSDFVolume
    v2 = TSDFVolume(T.SPHERE_LO, T.SPHERE_HI, (4, 5, 6), trunc=0.5)
    v2.integrate(_dev(case["depth"][0]), *case["k"], _dev(case["c2w"][0]))
    assert float(v2.weight.sum()) > 0
    v2.reset()
    assert bool((v2.tsdf == 1).all()) and bool((v2.weight == 0).all()) and v2.trunc == 0.5
    assert v2.extract_mesh().faces.shape[0] == 0
    for kw in (dict(trunc=0.0), dict(trunc=NAN), dict(resolution=1)):
        with pytest.raises(ValueError):
            TSDFVolume(T.SPHERE_LO, T.SPHERE_HI, **{"resolution": 8, **kw})


def test_round_trip_through_the_ray_caster(K):
    """a closed mesh rendered by Mesh.render from the 14 cameras at 48x48, its depth fused at 24^3: the result lies
    within one voxel of the original in Hausdorff distance, measured against the triangles"""
    from nerf_amd import Mesh, TSDFVolume
    v, f, _ = MS.sphere_mesh(12)  # the marching-tetrahedra sphere of radius 0.6 on 12^3: closed, facets of about 2 h
    src = Mesh(_dev(v), _dev(f))
    case = T.sphere_case()
    n = T.SPHERE_HW
    depth = torch.stack([src.render(n, n, *case["k"], _dev(M))["depth"] for M in case["c2w"]])
    assert bool(torch.isinf(depth).any()) and bool(torch.isfinite(depth).any())
    vol = TSDFVolume(T.SPHERE_LO, T.SPHERE_HI, 24)
    vol.integrate(depth, *case["k"], _dev(case["c2w"]))
    out = vol.extract_mesh(normals=None)
    assert MR.is_closed(out.faces.cpu().numpy())
    d = out.distance_to(src, n_samples=2 ** 14, exact=True)
    print(f"round trip: hausdorff {d['hausdorff']:.4f} = {d['hausdorff'] / T.sphere_h():.2f} h, chamfer {d['chamfer']:.4f}")
    assert d["hausdorff"] < T.sphere_h()


# ------------------------------------------------------------------ a model


@pytest.fixture(scope="module")
def model(K):
    import ngp_grad_cases as C
    from nerf_amd import ngp as N
    st = C.prod_state()
    st["sigma_head.bias"] = torch.full((1,), math.log(10.0))
    net = N.InstantNGP(occ_conf={}, scene_box=C.AABB, **C.PROD)
    net.load_reference_state(st)
    return net.to(DEV).eval()


def test_model_extract_mesh_tsdf(K, model):
    from nerf_amd import Mesh, TSDFVolume
    from nerf_amd.ray_rendering import fuse_depth_views
    from nerf_amd.scene import hemisphere_poses
    poses = hemisphere_poses(4, seed=0)
    n = 16
    focal = 0.5 * n / math.tan(0.5 * 0.6911112)
    cam = dict(H=n, W=n, fx=focal, fy=focal, cx=n / 2.0, cy=n / 2.0, near=2.0, far=6.0)
    kw = dict(resolution=16, ray_samples=32, batch=3)
    a = model.extract_mesh_tsdf(poses, **cam, **kw)
    b = model.extract_mesh_tsdf(poses, **cam, **kw)
    assert isinstance(a, Mesh) and a.vertices.shape[0] > 0 and a.faces.shape[0] > 0
    assert bool(torch.isfinite(a.vertices).all()) and a.normals is not None and a.colors is None
    assert tuple(a.normals.shape) == tuple(a.vertices.shape)
    for x, y in ((a.vertices, b.vertices), (a.faces, b.faces), (a.normals, b.normals)):
        assert torch.equal(x, y)
    c = model.extract_mesh_tsdf(poses, **cam, normals="grid", colors="srgb", **kw)
    assert torch.equal(c.vertices, a.vertices) and tuple(c.colors.shape) == tuple(c.vertices.shape)
    vol = fuse_depth_views(model, poses, lo=[-1.5] * 3, hi=[1.5] * 3, **cam, **kw)
    assert isinstance(vol, TSDFVolume) and float(vol.weight.max()) >= 1
    assert torch.equal(vol.extract_mesh(normals=None).vertices, a.vertices)
    # nothing seen: no view updates a voxel, the mesh is empty
    blind = fuse_depth_views(model, poses, lo=[-1.5] * 3, hi=[1.5] * 3, acc_min=2.0, **cam, **kw)
    assert bool((blind.weight == 0).all()) and bool((blind.tsdf == 1).all())
    empty = model.extract_mesh_tsdf(poses, **cam, acc_min=2.0, **kw)
    assert empty.vertices.shape == (0, 3) and empty.faces.shape == (0, 3)
