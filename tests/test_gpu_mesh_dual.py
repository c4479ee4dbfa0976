"""Dual contouring on the device (-m gpu): kernels.mesh_dual_hermite / mesh_dual_vertices / mesh_extract_dual
(csrc/mesh_dual.hip: nerf_mesh_dual_classify -> scans -> nerf_mesh_dual_edges -> nerf_mesh_dual_cells),
mesh.extract_mesh(method="dual") and InstantNGP.extract_mesh(method="dual"), against the numpy restatement of the rule
in tests/mesh_dual_reference.py.

Parity is index for index and bit for bit: E, V, F, the keys, the Hermite points, the faces, the vertices and the
fallback bytes; mesh_dual.o is built with -ffp-contract=off and both sides round every fp32 and double operation once,
in the same order.  Normals (of the edges and of the cells) are compared to 1e-5, as test_gpu_mesh.py compares them.
Lattices stay at or below about 2.5k points so the looped reference takes seconds; every reference is computed once
per module.

The cube's bounds are those of test_mesh_dual_reference.py (4 x the reference's own 1.32e-8 / 1.56e-8).  The refined
sphere's bound is 4 x what the reference gives for the same settings, computed here; that check runs on a density
that is exponential in the distance (see _sphere_sigma for why)."""
import functools

import numpy as np
import pytest
import torch

import mesh_dual_reference as D
import mesh_reference as M
from mesh_dual_reference import CUBE_CORNER_BOUND, CUBE_SURFACE_BOUND

pytestmark = pytest.mark.gpu

DEV = "cuda"
UNIT_LO, UNIT_HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
BOX_LO, BOX_HI = (-1.0, -0.5, 0.25), (1.5, 0.75, 2.0)  # non-cubic, lo != -hi
SHAPES = [(2, 2, 2), (3, 3, 3), (5, 4, 3), (3, 2, 9), (33, 5, 4), (17, 16, 9)]
SPHERE_R = 0.6


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from nerf_amd import kernels
    return kernels


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def _field(kind, shape):
    if kind == "noise":
        return M.noise_field(shape, seed=1 + shape[0]), 0.0
    if kind == "integers":
        return M.integer_field(shape, seed=4 + shape[2]), 0.0
    return M.sines_field(shape, BOX_LO, BOX_HI), 0.2


@functools.lru_cache(maxsize=None)
def _reference(kind, shape, placement):
    f, iso = _field(kind, shape)
    return D.dual_contour(f, iso, BOX_LO, BOX_HI, placement)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run(K, field, iso, lo, hi, placement, points=None, normals=None):
    """Everything the three kernels write, on the host."""
    rec, pts, nrm, keys = K.mesh_dual_hermite(_dev(field), iso, lo, hi, normals=True)
    assert pts.dtype == torch.float32 and nrm.dtype == torch.float32 and keys.dtype == torch.int32
    assert tuple(pts.shape) == (rec.E, 3) and tuple(nrm.shape) == (rec.E, 3) and tuple(keys.shape) == (rec.E,)
    use_p = pts if points is None else _dev(points)
    use_n = nrm if normals is None else _dev(normals)
    v, f, vn, fb = K.mesh_dual_vertices(rec, use_p, use_n, placement=placement, vertex_normals=True,
                                        return_fallback=True)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and vn.dtype == torch.float32 and fb.dtype == torch.uint8
    assert tuple(v.shape) == (rec.V, 3) and tuple(f.shape) == (rec.F, 3) and tuple(vn.shape) == (rec.V, 3)
    assert tuple(fb.shape) == (rec.V,)
    host = lambda t: t.cpu().numpy()
    return dict(E=rec.E, V=rec.V, F=rec.F, keys=host(keys), points=host(pts), normals=host(nrm), verts=host(v),
                faces=host(f), vertex_normals=host(vn), fallback=host(fb))


def _assert_parity(got, ref, hermite_replaced=False):
    assert (got["E"], got["V"], got["F"]) == (ref["E"], ref["V"], ref["F"])
    assert np.array_equal(got["keys"], ref["keys"])
    if not hermite_replaced:
        assert np.array_equal(_bits(got["points"]), _bits(ref["points"]))
        assert got["E"] == 0 or np.abs(got["normals"] - ref["normals"]).max() <= 1e-5
    assert np.array_equal(got["faces"], ref["faces"])
    assert np.array_equal(got["fallback"], ref["fallback"])
    assert np.array_equal(_bits(got["verts"]), _bits(ref["verts"]))
    assert got["V"] == 0 or np.abs(got["vertex_normals"] - ref["vertex_normals"]).max() <= 1e-5


# ------------------------------------------------------------------ parity


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("placement", ["qef", "mean"])
@pytest.mark.parametrize("kind", ["noise", "sines", "integers"])
def test_parity_with_reference(K, kind, placement, shape):
    f, iso = _field(kind, shape)
    ref = _reference(kind, shape, placement)
    got = _run(K, f, iso, BOX_LO, BOX_HI, placement)
    print(f"{kind} {shape} {placement}: E={got['E']} V={got['V']} F={got['F']} fallback={int(got['fallback'].sum())}")
    _assert_parity(got, ref)
    if kind != "integers":
        assert got["V"] > 0
    if shape == (2, 2, 2):
        assert got["F"] == 0
    if shape == (3, 3, 3) and kind == "noise":
        assert got["F"] > 0
    # the one-call wrapper returns the same bits
    v, fc, vn = K.mesh_extract_dual(_dev(f), iso, BOX_LO, BOX_HI, placement=placement, normals=True)
    assert np.array_equal(_bits(v.cpu().numpy()), _bits(got["verts"])) and np.array_equal(fc.cpu().numpy(), got["faces"])
    assert np.array_equal(_bits(vn.cpu().numpy()), _bits(got["vertex_normals"]))


def test_cube_with_replaced_hermite_data(K):
    f, ref = D.case("cube", "qef")
    got = _run(K, f, 0.0, D.BOX_LO, D.BOX_HI, "qef", points=ref["points"], normals=ref["normals"])
    _assert_parity(got, ref, hermite_replaced=True)
    surface, corner = D.cube_surface_distance(got["verts"]).max(), D.cube_corner_distance(got["verts"]).max()
    print(f"cube: surface {surface:.3g}, corners {corner:.3g}, fallbacks {int(got['fallback'].sum())}")
    assert int(got["fallback"].sum()) == 0
    assert surface <= CUBE_SURFACE_BOUND and corner <= CUBE_CORNER_BOUND
    _, mean = D.case("cube", "mean")
    _assert_parity(_run(K, f, 0.0, D.BOX_LO, D.BOX_HI, "mean", points=ref["points"], normals=ref["normals"]), mean,
                   hermite_replaced=True)


@pytest.mark.parametrize("value", [1.0, -1.0], ids=["all_inside", "all_outside"])
def test_no_crossing_gives_empty_mesh(K, value):
    field = torch.full((4, 3, 5), value, device=DEV)
    rec, pts, nrm, keys = K.mesh_dual_hermite(field, 0.0, UNIT_LO, UNIT_HI)
    assert (rec.E, rec.V, rec.F) == (0, 0, 0)
    assert tuple(pts.shape) == (0, 3) and tuple(nrm.shape) == (0, 3) and tuple(keys.shape) == (0,)
    out = K.mesh_dual_vertices(rec, pts, nrm, vertex_normals=True, return_fallback=True)
    assert [tuple(o.shape) for o in out] == [(0, 3), (0, 3), (0, 3), (0,)]
    v, f = K.mesh_extract_dual(field, 0.0, UNIT_LO, UNIT_HI)
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and f.dtype == torch.int32


# ------------------------------------------------------------------ mesh.extract_mesh


def _sphere_density(x):
    return SPHERE_R - torch.linalg.norm(x, dim=-1, keepdim=True)


def _sphere_normals(x):
    return x / torch.linalg.norm(x, dim=-1, keepdim=True)


# The refinement check runs on a density that is exponential in the distance, sigma = exp(k (r - |x|)) with the
# threshold 1, the shape of the fields this project extracts (InstantNGP's sigma is an exponential of its network).
# Along a lattice edge such a field is far from linear: with k h = 3 the crossing that marching tetrahedra's linear
# interpolation finds is off by up to a third of a cell, outwards (the exponential is convex, its chord lies above
# it), so the data error (5.6e-2 on the reference) is several times the bias of the placement and bisection has
# something to remove.  The signed distance r - |x| cannot show that: it is linear along an edge to h^2 / 8r = 5e-3,
# less than the placement's own bias, see test_sphere_refined_improves_radius.
SIGMA_K, SIGMA_ISO = 20.0, 1.0


def _sphere_sigma(x):
    return torch.exp(SIGMA_K * (SPHERE_R - torch.linalg.norm(x, dim=-1, keepdim=True)))


@functools.lru_cache(maxsize=None)
def _sphere_reference_errors():
    """(unrefined with grid normals, refined 12 times with analytic normals): the reference's max radius errors on the
    exponential density."""
    x = M.lattice_points(D.SHAPE, UNIT_LO, UNIT_HI)
    f = np.exp(SIGMA_K * (SPHERE_R - np.linalg.norm(x, axis=-1))).astype(np.float32)
    grid = D.dual_contour(f, SIGMA_ISO, UNIT_LO, UNIT_HI, "qef")
    dens = lambda p: np.exp(np.float32(SIGMA_K) * (np.float32(SPHERE_R) - np.sqrt((p * p).sum(1, dtype=np.float32))))
    pts = D.refine(dens, grid["keys"], f, SIGMA_ISO, D.SHAPE, UNIT_LO, UNIT_HI, 12)
    nrm = (pts / np.linalg.norm(pts, axis=1, keepdims=True)).astype(np.float32)
    fine = D.dual_contour(f, SIGMA_ISO, UNIT_LO, UNIT_HI, "qef", points=pts, normals=nrm)
    err = lambda r: float(np.abs(np.linalg.norm(r["verts"].astype(np.float64), axis=1) - SPHERE_R).max())
    return err(grid), err(fine)


def _radius_error(m):
    return float((torch.linalg.norm(m.vertices.double(), dim=1) - SPHERE_R).abs().max())


@pytest.fixture(scope="module")
def spheres(K):
    from nerf_amd import mesh
    plain = mesh.extract_mesh(_sphere_sigma, UNIT_LO, UNIT_HI, D.SHAPE, SIGMA_ISO, method="dual")
    fine = mesh.extract_mesh(_sphere_sigma, UNIT_LO, UNIT_HI, D.SHAPE, SIGMA_ISO, method="dual", refine=12,
                             hermite=_sphere_normals)
    return plain, fine


def test_sphere_refined_improves_radius(spheres):
    """With refine=12 and analytic normals the maximum radius error of the "qef" vertices is smaller than unrefined
    (reference: 5.54e-2 unrefined, 1.567e-2 refined; crossing points 5.6e-2 -> 1.9e-5).

    This test first ran on the signed distance r - |x| and failed there, on the device and on the reference alike:
    1.487e-2 unrefined, 1.567e-2 refined (tol 1e-3; 1.422e-2 / 1.507e-2 at tol 1e-1; the same order at r = 0.3, 0.45,
    0.8 and on a 10^3 lattice).  That was a mistake in the test's choice of field, not in the extractor.  The planes
    of exact Hermite data are tangent to the sphere, so their least-squares meeting point lies outside it by about
    spread^2 / 2r whatever the accuracy of the data: 1.567e-2 is that bias, and no refinement goes below it.  A signed
    distance is linear along an edge to 5e-3, so its unrefined data is already better than the placement, and its small
    inward error (the field is concave along an edge) happens to cancel part of the outward bias.  A field that is not
    nearly linear along an edge is what refine is for, and the check is made on one (see _sphere_sigma); the lattice,
    the sphere, the 12 steps, the normals and the bounds are unchanged."""
    plain, fine = spheres
    print(f"sphere radius error: grid {_radius_error(plain):.4g}, refined {_radius_error(fine):.4g}")
    assert _radius_error(fine) < _radius_error(plain)


def test_sphere_refined_mean(K):
    from nerf_amd import mesh
    kw = dict(method="dual", placement="mean", normals=None)
    plain = mesh.extract_mesh(_sphere_density, UNIT_LO, UNIT_HI, D.SHAPE, 0.0, **kw)
    fine = mesh.extract_mesh(_sphere_density, UNIT_LO, UNIT_HI, D.SHAPE, 0.0, refine=12, **kw)
    print(f"sphere radius error, mean: grid {_radius_error(plain):.4g}, refined {_radius_error(fine):.4g}")
    assert _radius_error(fine) < _radius_error(plain)


def test_sphere_refined(spheres):
    from nerf_amd import mesh
    plain, fine = spheres
    ref_plain, ref_fine = _sphere_reference_errors()
    for m in (plain, fine):
        f = m.faces.cpu().numpy()
        assert M.is_closed(f) and M.euler_characteristic(m.vertices.shape[0], f) == 2
        assert M.signed_volume(m.vertices.cpu().numpy(), f) > 0
    err = _radius_error
    print(f"sphere radius error: grid {err(plain):.3g} (reference {ref_plain:.3g}), refined {err(fine):.3g} "
          f"(reference {ref_fine:.3g})")
    assert err(fine) <= 4 * ref_fine and err(plain) <= 4 * ref_plain
    assert plain.normals is not None and tuple(plain.normals.shape) == tuple(plain.vertices.shape)
    outward = (plain.normals * plain.vertices).sum(1)
    assert bool((outward > 0).all())
    mean = mesh.extract_mesh(_sphere_sigma, UNIT_LO, UNIT_HI, D.SHAPE, SIGMA_ISO, method="dual", placement="mean",
                             normals=None)
    assert mean.normals is None and torch.equal(mean.faces, plain.faces)


def test_downstream_options(K, tmp_path):
    from nerf_amd import mesh
    m = mesh.extract_mesh(_sphere_density, UNIT_LO, UNIT_HI, D.SHAPE, 0.0, method="dual")
    assert m.filter_components(keep_largest=1).faces.shape[0] == m.faces.shape[0]
    s = m.simplify(0.3)
    assert 0 < s.faces.shape[0] < m.faces.shape[0]
    q = m.simplify(0.3, placement="quadric")
    assert q.faces.shape[0] == s.faces.shape[0]
    sm = m.smooth(2)
    assert sm.faces.shape[0] == m.faces.shape[0] and bool(torch.isfinite(sm.vertices).all())
    probe = torch.tensor([[0.0, 0.0, 0.0], [0.1, -0.2, 0.3], [0.9, 0.9, 0.9], [0.0, 0.0, 0.8]], device=DEV)
    assert m.contains(probe).cpu().tolist() == [True, True, False, False]
    m.save_ply(str(tmp_path / "dual.ply"))
    assert (tmp_path / "dual.ply").stat().st_size > 0
    both = mesh.extract_mesh(_sphere_density, UNIT_LO, UNIT_HI, D.SHAPE, 0.0, method="dual", keep_largest=1,
                             simplify=0.3, smooth=1, normals=_sphere_normals)
    assert both.faces.shape[0] > 0 and tuple(both.normals.shape) == tuple(both.vertices.shape)


def test_default_method_is_marching_tetrahedra(K):
    from nerf_amd import mesh
    field = mesh.density_lattice(_sphere_density, UNIT_LO, UNIT_HI, D.SHAPE, device=DEV)
    v, f, n = K.mesh_extract(field, 0.0, UNIT_LO, UNIT_HI, normals=True)
    for m in (mesh.extract_mesh(_sphere_density, UNIT_LO, UNIT_HI, D.SHAPE, 0.0),
              mesh.extract_mesh(_sphere_density, UNIT_LO, UNIT_HI, D.SHAPE, 0.0, method="tets")):
        assert torch.equal(m.vertices, v) and torch.equal(m.faces, f) and torch.equal(m.normals, n)
    with pytest.raises(ValueError):
        mesh.extract_mesh(_sphere_density, UNIT_LO, UNIT_HI, D.SHAPE, 0.0, refine=2)


def test_model_extract_mesh_dual(K):
    import math
    import ngp_grad_cases as C
    from nerf_amd import Mesh, density_lattice
    from nerf_amd import ngp as N
    st = C.prod_state()
    st["sigma_head.bias"] = torch.full((1,), math.log(10.0))  # sigma = 10 exp(noise): crosses the threshold 10
    model = N.InstantNGP(occ_conf={}, scene_box=C.AABB, **C.PROD)
    model.load_reference_state(st)
    model = model.to(DEV).eval()
    lo, hi, res = [-1.5] * 3, [1.5] * 3, 16
    m = model.extract_mesh(resolution=res, method="dual", hermite="field", normals="field")
    assert isinstance(m, Mesh) and m.vertices.shape[0] > 0 and m.faces.shape[0] > 0
    assert bool(torch.isfinite(m.vertices).all()) and bool(torch.isfinite(m.normals).all())
    assert int(m.faces.min()) >= 0 and int(m.faces.max()) < m.vertices.shape[0]
    # the same through the kernels, and every vertex inside its own cell
    field = density_lattice(model.density, lo, hi, res)
    rec, pts, _, _ = K.mesh_dual_hermite(field, 10.0, lo, hi, normals=False)
    v, f = K.mesh_dual_vertices(rec, pts, model.normals(pts))
    assert torch.equal(m.vertices, v) and torch.equal(m.faces, f)
    p = torch.nonzero(rec.cell_off[1:] != rec.cell_off[:-1]).reshape(-1).cpu().numpy()
    cells = np.stack([p // (res * res), p // res % res, p % res], 1).astype(np.float32)
    h = M.spacing((res,) * 3, lo, hi)
    a = np.asarray(lo, np.float32) + cells * h
    slack = 4e-7 * (np.abs(a) + np.abs(a + h) + h)  # the roundings of lo + i h and of pa + t h
    vh = v.cpu().numpy()
    assert len(p) == len(vh) and ((vh >= a - slack) & (vh <= a + h + slack)).all()
    grid = model.extract_mesh(resolution=res, method="dual", hermite="grid", normals=None, placement="mean", refine=3)
    assert torch.equal(grid.faces, f) and grid.normals is None
    with pytest.raises(ValueError):
        model.extract_mesh(resolution=res, method="dual", hermite="vertex")
    with pytest.raises(ValueError):
        model.extract_mesh(resolution=res, method="cubes")


def test_tsdf_rejects_dual(K):
    from nerf_amd.tsdf import TSDFVolume
    vol = TSDFVolume(UNIT_LO, UNIT_HI, 4, trunc=0.5, device=DEV)
    with pytest.raises(ValueError, match="dual"):
        vol.extract_mesh(method="dual")


def test_bad_arguments(K):
    f, _ = D.case("cube", "qef")
    rec, pts, nrm, _ = K.mesh_dual_hermite(_dev(f), 0.0, D.BOX_LO, D.BOX_HI)
    assert K.mesh_dual_vertices(rec, pts, nrm)[1].shape[0] > 0
    assert K.mesh_dual_vertices(rec, pts, placement="mean")[1].shape[0] > 0
    nan = pts.clone()
    nan[3, 1] = float("nan")
    bad = [
        dict(points=pts),                                      # qef without normals
        dict(points=pts, placement="mean", vertex_normals=True),   # cell normals without normals
        dict(points=pts, normals=nrm, tol=0.0),
        dict(points=pts, normals=nrm, tol=1.0),
        dict(points=pts, normals=nrm, tol=float("nan")),
        dict(points=pts, normals=nrm, placement="median"),
        dict(points=pts[:-1], normals=nrm),                    # wrong shapes
        dict(points=pts, normals=nrm[:, :2].contiguous()),
        dict(points=pts.reshape(-1), normals=nrm),
        dict(points=pts.cpu(), normals=nrm),                   # wrong devices
        dict(points=pts, normals=nrm.cpu()),
        dict(points=pts.double(), normals=nrm),                # wrong dtype
        dict(points=nan, normals=nrm),                         # not finite
        dict(points=pts, normals=torch.full_like(nrm, float("inf"))),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            K.mesh_dual_vertices(rec, **kw)
    with pytest.raises(ValueError):
        K.mesh_dual_vertices(None, pts, nrm)
    ok = torch.zeros((3, 3, 3), device=DEV)
    for field, lo, hi in [(ok.cpu(), UNIT_LO, UNIT_HI), (ok.double(), UNIT_LO, UNIT_HI),
                          (torch.zeros((3, 3), device=DEV), UNIT_LO, UNIT_HI),
                          (torch.zeros((1, 4, 4), device=DEV), UNIT_LO, UNIT_HI),
                          (ok, (0.0, 2.0, 0.0), (1.0, 1.0, 1.0)),
                          (torch.full((3, 3, 3), float("nan"), device=DEV), UNIT_LO, UNIT_HI)]:
        with pytest.raises(ValueError):
            K.mesh_dual_hermite(field, 0.5, lo, hi)
    with pytest.raises(ValueError):
        K.mesh_extract_dual(ok, 0.5, UNIT_LO, UNIT_HI, placement="median")
