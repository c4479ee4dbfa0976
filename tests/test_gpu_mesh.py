"""kernels.mesh_extract (csrc/mesh.hip: nerf_mesh_classify -> scans -> nerf_mesh_emit), nerf_amd.mesh and
InstantNGP.extract_mesh on the device (-m gpu), against the numpy restatement of the rule in tests/mesh_reference.py.

Parity is index for index: V, F and the faces array exactly, and the positions bitwise, because mesh.o is built with
-ffp-contract=off and a vertex is pa + t (pb - pa) with every operation rounded once on both sides (IEEE division on
both).  Lattices stay at or below about 2.5k points so the looped reference takes seconds; every reference is computed
once per module."""
import functools

import numpy as np
import pytest
import torch

import mesh_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
UNIT_LO, UNIT_HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
BOX_LO, BOX_HI = (-1.0, -0.5, 0.25), (1.5, 0.75, 2.0)  # non-cubic, lo != -hi
SHAPES = [(2, 2, 2), (5, 4, 3), (3, 2, 9), (33, 5, 4), (17, 16, 9)]  # the last: 2448 points > one 2048 scan tile
SPHERE_SHAPE = (14, 13, 12)


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from nerf_amd import kernels
    return kernels


def _extract(K, field, iso, lo, hi, normals=False):
    out = K.mesh_extract(torch.from_numpy(np.ascontiguousarray(field, np.float32)).to(DEV), iso, lo, hi,
                         normals=normals)
    assert out[0].dtype == torch.float32 and out[1].dtype == torch.int32
    assert out[0].dim() == 2 and out[0].shape[1] == 3 and out[1].dim() == 2 and out[1].shape[1] == 3
    return tuple(o.cpu().numpy() for o in out)


def _field(kind, shape):
    if kind == "noise":
        return R.noise_field(shape, seed=1 + shape[0]), 0.0
    return R.sines_field(shape, BOX_LO, BOX_HI), 0.2


@functools.lru_cache(maxsize=None)
def _parity_reference(kind, shape):
    f, iso = _field(kind, shape)
    return R.marching_tets(f, iso, BOX_LO, BOX_HI, normals=True)


@functools.lru_cache(maxsize=None)
def _sphere_reference():
    return R.marching_tets(R.sphere_field(SPHERE_SHAPE, UNIT_LO, UNIT_HI), 0.0, UNIT_LO, UNIT_HI, normals=True)


# ------------------------------------------------------------------ parity


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", ["noise", "sines"])
def test_parity_with_reference(K, kind, shape):
    f, iso = _field(kind, shape)
    rv, rf, rn = _parity_reference(kind, shape)
    v, fc, n = _extract(K, f, iso, BOX_LO, BOX_HI, normals=True)
    print(f"{kind} {shape}: V={len(v)} (ref {len(rv)}) F={len(fc)} (ref {len(rf)})")
    assert len(rv) > 0 and len(rf) > 0
    assert v.shape == rv.shape and fc.shape == rf.shape
    assert np.array_equal(fc, rf)
    assert np.array_equal(v.view(np.uint32), rv.view(np.uint32))
    assert np.abs(n - rn).max() <= 1e-5
    v2, f2 = _extract(K, f, iso, BOX_LO, BOX_HI)
    assert np.array_equal(v2.view(np.uint32), v.view(np.uint32)) and np.array_equal(f2, fc)


# ------------------------------------------------------------------ known answers on the device output


def test_sphere(K):
    """Closed and consistently oriented, a topological sphere, positive volume; the radius error is within the
    linear-interpolation bound of a distance field, |h|^2 / (8 (r0 - |h|)) = 0.034 here (the reference: 0.0151)."""
    v, f = _extract(K, R.sphere_field(SPHERE_SHAPE, UNIT_LO, UNIT_HI), 0.0, UNIT_LO, UNIT_HI)
    assert len(f) > 0
    assert all(k == 2 for k in R.undirected_edge_counts(f).values())
    assert all(k == 1 for k in R.directed_edge_counts(f).values())
    assert R.euler_characteristic(len(v), f) == 2
    assert R.signed_volume(v, f) > 0
    h = R.spacing(SPHERE_SHAPE, UNIT_LO, UNIT_HI).astype(np.float64)
    hh = float(np.sum(h * h))
    err = np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - 0.6).max()
    print(f"sphere radius error {err:.4f}, bound {hh / (8.0 * (0.6 - np.sqrt(hh))):.4f}")
    assert err <= hh / (8.0 * (0.6 - np.sqrt(hh)))


def test_torus(K):
    v, f = _extract(K, R.torus_field((16, 16, 10), UNIT_LO, UNIT_HI), 0.0, UNIT_LO, UNIT_HI)
    assert R.is_closed(f)
    assert R.euler_characteristic(len(v), f) == 0


def test_two_spheres(K):
    lo, hi, shape = (-1.6, -0.8, -0.8), (1.6, 0.8, 0.8), (20, 11, 11)
    field = np.maximum(R.sphere_field(shape, lo, hi, 0.5, (-0.9, 0.0, 0.0)),
                       R.sphere_field(shape, lo, hi, 0.5, (0.9, 0.0, 0.0)))
    v, f = _extract(K, field, 0.0, lo, hi)
    assert R.is_closed(f)
    assert R.euler_characteristic(len(v), f) == 4


def _on_common_box_face(va, vb, lo, hi, tol):
    return any(abs(va[a] - side[a]) <= tol and abs(vb[a] - side[a]) <= tol for a in range(3) for side in (lo, hi))


def test_sphere_cut_by_box(K):
    """The surface is open only where the box cuts it: every boundary edge has both ends on one box face."""
    shape = (12, 12, 12)
    v, f = _extract(K, R.sphere_field(shape, UNIT_LO, UNIT_HI, 0.6, (0.7, 0.0, 0.0)), 0.0, UNIT_LO, UNIT_HI)
    be = R.boundary_edges(f)
    assert len(be) > 0
    assert all(k == 1 for k in R.directed_edge_counts(f).values())
    assert all(_on_common_box_face(v[a], v[b], UNIT_LO, UNIT_HI, 4 * np.finfo(np.float32).eps) for a, b in be)


def test_plane(K):
    shape = (6, 5, 7)
    z0 = np.float32(0.13)
    field = (0.13 - R.lattice_points(shape, UNIT_LO, UNIT_HI)[..., 2]).astype(np.float32)
    v, f, n = _extract(K, field, 0.0, UNIT_LO, UNIT_HI, normals=True)
    assert len(v) > 0
    assert np.abs(v[:, 2] - z0).max() <= 2 * np.spacing(z0)
    assert abs(R.area(v, f) - 4.0) <= 1e-5 * 4.0
    fn = R.face_normals(v, f)
    fn /= np.linalg.norm(fn, axis=1, keepdims=True)
    up = np.array([0.0, 0.0, 1.0])
    assert np.abs(fn - up).max() <= 1e-6
    assert np.abs(n - up).max() <= 1e-6


def test_grid_normals_on_sphere(K):
    """Unit length; equal to the reference's central-difference normals within 1e-5; within the reference's own worst
    angle to the radial direction on this lattice, 0.0349 rad (2.0 degrees), plus the 2e-5 rad that a 1e-5 difference
    per component can turn a unit vector."""
    rv, _, rn = _sphere_reference()
    v, _, n = _extract(K, R.sphere_field(SPHERE_SHAPE, UNIT_LO, UNIT_HI), 0.0, UNIT_LO, UNIT_HI, normals=True)
    assert np.array_equal(v, rv)
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    assert np.abs(n - rn).max() <= 1e-5

    def worst_angle(nn):
        radial = v / np.linalg.norm(v, axis=1, keepdims=True)
        return float(np.arccos(np.clip((nn.astype(np.float64) * radial).sum(1), -1.0, 1.0)).max())

    ref_worst = worst_angle(rn)
    print(f"worst angle to radial: device {worst_angle(n):.5f}, reference {ref_worst:.5f}")
    assert 0.03 < ref_worst < 0.04
    assert worst_angle(n) <= ref_worst + 2e-5


# ------------------------------------------------------------------ edges of the domain


@pytest.mark.parametrize("value", [1.0, -1.0], ids=["all_inside", "all_outside"])
@pytest.mark.parametrize("normals", [False, True])
def test_no_crossing_gives_empty_mesh(K, value, normals):
    out = K.mesh_extract(torch.full((4, 3, 5), value, device=DEV), 0.0, UNIT_LO, UNIT_HI, normals=normals)
    assert len(out) == (3 if normals else 2)
    assert all(tuple(o.shape) == (0, 3) for o in out)
    assert out[0].dtype == torch.float32 and out[1].dtype == torch.int32


@pytest.mark.parametrize("corner,n_vert,n_face,n_open", [(0, 7, 6, 6), (1, 4, 2, 4), (7, 7, 6, 6)])
def test_single_inside_corner(K, corner, n_vert, n_face, n_open):
    """The smallest crossings of a (2,2,2) lattice.  In the Kuhn split a corner has at least four edges (corners 0 and
    7 have seven), so a lone crossing edge cannot occur; one inside corner is the least.  Its vertices are the
    midpoints of its edges (values +1 / -1), every triangle faces away from it, and the patch is a disk (six triangles
    around the vertex on the body diagonal, or two sharing the one on the face diagonal)."""
    field = -np.ones((2, 2, 2), np.float32)
    c = np.array([corner & 1, (corner >> 1) & 1, (corner >> 2) & 1])
    field[tuple(c)] = 1.0
    v, f = _extract(K, field, 0.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    assert v.shape == (n_vert, 3) and f.shape == (n_face, 3)
    other = 2.0 * (v - c) + c  # the far end of each crossing edge
    assert np.array_equal(other, np.round(other)) and (other >= 0).all() and (other <= 1).all()
    assert len({tuple(o) for o in other.tolist()}) == n_vert
    centroid = v[f].mean(axis=1)
    assert (np.einsum("ij,ij->i", R.face_normals(v, f), centroid - c) > 0).all()
    assert len(R.boundary_edges(f)) == n_open and R.euler_characteristic(n_vert, f) == 1
    assert sorted(np.unique(f).tolist()) == list(range(n_vert))


def test_integer_field_iso_on_lattice_values(K):
    v, f = _extract(K, R.integer_field((8, 7, 6), 4), 0.0, UNIT_LO, UNIT_HI)
    assert len(f) > 100
    assert np.isfinite(v).all()
    assert R.is_closed(f)


def test_deterministic(K):
    f, iso = _field("noise", (17, 16, 9))
    a = _extract(K, f, iso, BOX_LO, BOX_HI, normals=True)
    b = _extract(K, f, iso, BOX_LO, BOX_HI, normals=True)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_bad_arguments(K):
    ok = torch.zeros((3, 3, 3), device=DEV)
    ok[1, 1, 1] = 1.0
    assert K.mesh_extract(ok, 0.5, UNIT_LO, UNIT_HI)[1].shape[0] > 0
    bad = [
        (ok.cpu(), UNIT_LO, UNIT_HI),                                   # CPU tensor
        (ok.double(), UNIT_LO, UNIT_HI),                                # wrong dtype
        (torch.zeros((3, 3, 6), device=DEV)[:, :, ::2], UNIT_LO, UNIT_HI),  # not contiguous
        (torch.zeros((3, 3), device=DEV), UNIT_LO, UNIT_HI),            # wrong number of dimensions
        (torch.zeros((1, 3, 3, 3), device=DEV), UNIT_LO, UNIT_HI),
        (torch.zeros((1, 4, 4), device=DEV), UNIT_LO, UNIT_HI),         # a dimension below 2
        (torch.zeros((4, 4, 1), device=DEV), UNIT_LO, UNIT_HI),
        (ok, (0.0, 0.0, 0.0), (1.0, 0.0, 1.0)),                         # lo >= hi
        (ok, (0.0, 2.0, 0.0), (1.0, 1.0, 1.0)),
        (ok, (0.0, 0.0), (1.0, 1.0)),
        (torch.full((3, 3, 3), float("nan"), device=DEV), UNIT_LO, UNIT_HI),  # not finite
    ]
    for field, lo, hi in bad:
        with pytest.raises(ValueError):
            K.mesh_extract(field, 0.5, lo, hi)


# ------------------------------------------------------------------ end to end


@pytest.fixture(scope="module")
def model(K):
    import math
    import ngp_grad_cases as C
    from nerf_amd import ngp as N
    st = C.prod_state()
    st["sigma_head.bias"] = torch.full((1,), math.log(10.0))  # sigma = 10 exp(noise): crosses the threshold 10
    net = N.InstantNGP(occ_conf={}, scene_box=C.AABB, **C.PROD)
    net.load_reference_state(st)
    return net.to(DEV).eval()


def test_model_extract_mesh(K, model):
    from nerf_amd import Mesh, density_lattice
    lo, hi = [-1.5] * 3, [1.5] * 3
    res = 20
    field = density_lattice(model.density, lo, hi, res)
    assert field.shape == (res, res, res) and field.is_contiguous()
    assert torch.equal(field, density_lattice(model.density, lo, hi, res, chunk=1000))
    v, f = K.mesh_extract(field, 10.0, lo, hi)
    assert v.shape[0] > 0 and f.shape[0] > 0

    mesh = model.extract_mesh(resolution=res, normals="field")
    assert isinstance(mesh, Mesh) and mesh.vertices.is_cuda
    assert torch.equal(mesh.vertices, v) and torch.equal(mesh.faces, f)
    assert torch.equal(mesh.normals, model.normals(v))
    small = model.extract_mesh(resolution=res, normals="field", chunk=1000)
    assert torch.equal(small.vertices, v) and torch.equal(small.faces, f) and torch.equal(small.normals, mesh.normals)

    grid = model.extract_mesh(resolution=(res, res, res), normals="grid")
    assert torch.equal(grid.vertices, v) and torch.equal(grid.faces, f)
    assert torch.equal(grid.normals, K.mesh_extract(field, 10.0, lo, hi, normals=True)[2])
    assert model.extract_mesh(resolution=res, normals=None).normals is None
    with pytest.raises(ValueError):
        model.extract_mesh(resolution=res, normals="vertex")

    # closed wherever it does not touch the box
    vh, fh = v.cpu().numpy(), f.cpu().numpy()
    assert all(k == 1 for k in R.directed_edge_counts(fh).values())
    tol = 4 * np.finfo(np.float32).eps * 1.5
    assert all(_on_common_box_face(vh[a], vh[b], lo, hi, tol) for a, b in R.boundary_edges(fh))
    host = mesh.cpu()
    assert not host.vertices.is_cuda and torch.equal(host.faces, f.cpu())
