"""kernels.mesh_cluster_quadric (csrc/mesh_simplify.hip, csrc/mesh_quadric_core.hpp), Mesh.simplify(placement="quadric")
and the ``simplify_placement`` option of extract_mesh on the device (-m gpu), against the numpy restatement of the
contract in tests/mesh_quadric_reference.py.

Every comparison is bitwise: the reference does the same float64 operations in the same order.  The inputs are a few
thousand items at most and every reference is computed once per process."""
import numpy as np
import pytest
import torch

import mesh_quadric_reference as Q
import mesh_simplify_reference as S

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from nerf_amd import kernels
    return kernels


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.cpu().numpy().tobytes()


def _same_bits(got, ref):
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(ref.shape)
    assert _bits(got) == np.ascontiguousarray(ref, np.float32).tobytes()


def _device_inputs(K, v, f, lo, cell, dims):
    """The device pipeline up to the placement: (vertices, faces, labels, row_off, col, mean)."""
    dv, df = _dev(v), _dev(f)
    labels = K.mesh_cluster_labels(dv, lo, cell, dims)
    mean, _, _ = K.mesh_cluster_reduce(dv, labels, lo, cell, dims, ranges_checked=True)
    g, _ = K.mesh_cluster_faces(df, labels, ranges_checked=True)
    row_off, col = K.mesh_vertex_faces(g, len(v), ranges_checked=True)
    return dv, df, labels, row_off, col, mean


def _check(K, v, f, lo, cell, dims, tol=Q.TOL):
    """The kernel against the reference on one input; returns the reference's (position, placed, info)."""
    lo = [float(x) for x in lo]
    dims = [int(d) for d in dims]
    labels = S.cluster_labels(v, lo, cell, dims)
    row_off, col = Q.cluster_rows(f, labels)
    mean, _, _ = S.cluster_reduce(v, labels, lo, cell, dims)
    rp, rf, info = Q.cluster_quadric(v, f, labels, row_off, col, mean, lo, cell, dims, tol, return_info=True)
    dv, df, dl, dro, dcol, dmean = _device_inputs(K, v, f, lo, cell, dims)
    assert np.array_equal(dl.cpu().numpy(), labels)
    assert np.array_equal(dro.cpu().numpy(), row_off) and np.array_equal(dcol.cpu().numpy(), col)
    _same_bits(dmean, mean)
    pos, placed = K.mesh_cluster_quadric(dv, df, dl, dro, dcol, dmean, lo, cell, dims, tol=tol)
    assert placed.dtype == torch.uint8 and tuple(placed.shape) == (len(v),)
    assert np.array_equal(placed.cpu().numpy(), rf)
    _same_bits(pos, rp)
    again, again_placed = K.mesh_cluster_quadric(dv, df, dl, dro, dcol, dmean, lo, cell, dims, tol=tol,
                                                 ranges_checked=True)
    assert _bits(again) == _bits(pos) and _bits(again_placed) == _bits(placed)  # equal inputs, equal bits
    other = torch.from_numpy(labels != np.arange(len(v)))
    if other.any():
        assert not pos.cpu()[other].any() and not placed.cpu()[other].any()  # zeros where no representative
    kept = (rf == 0) & (labels == np.arange(len(v)))
    assert _bits(pos[_dev(kept)]) == mean[kept].tobytes()  # a kept mean keeps its bits
    return rp, rf, info


def _soup(V, F, seed):
    return np.random.default_rng(seed).integers(0, V, (F, 3)).astype(np.int32)


# ------------------------------------------------------------------ the kernel


@pytest.mark.parametrize("name,factor", S.MESH_CASES)
def test_extracted(K, name, factor):
    v, f, _ = S.extracted(name)
    cell = np.float32(factor * S.lattice_spacing(name))
    lo, dims = S.simplify_grid(v, cell)
    _, placed, info = _check(K, v, f, lo, cell, dims)
    print(f"{name} x{factor}: {len(info['reps'])} clusters, {int(placed.sum())} placed, "
          f"ranks {np.bincount(info['rank'], minlength=4).tolist()}, longest row {int(info['rows'].max())}")


def test_cube(K):
    v, f, cell, origin = Q.cube_case()
    lo, dims = S.simplify_grid(v, cell, origin)
    _, placed, info = _check(K, v, f, lo, cell, dims)
    assert int(placed.sum()) == len(info["reps"])
    assert np.bincount(info["rank"], minlength=4).tolist() == [0, 96, 48, 8]  # faces, edges, corners


@pytest.mark.parametrize("cell", Q.SPHERE_CELLS)
def test_sphere(K, cell):
    v, f = Q.sphere_mesh()
    lo, dims = S.simplify_grid(v, np.float32(cell))
    _check(K, v, f, lo, np.float32(cell), dims)


@pytest.mark.parametrize("kind", ["random", "own_cell", "outside"])
@pytest.mark.parametrize("V", S.SIZES)
def test_sizes(K, kind, V):
    """Across the wave (64) and the workgroup (256); ``outside``: vertices beyond the grid, in border cells."""
    v, lo, cell, dims = S.vertex_case(kind, V)
    _, placed, info = _check(K, v, _soup(V, 2 * V + 1, V), lo, cell, dims)
    print(f"{kind} V={V}: {len(info['reps'])} clusters, {int(placed.sum())} placed")


def test_one_cell(K):
    """Everything in one cell: one thread walks all F faces, and every one of them lies inside the cell."""
    v, lo, cell, dims = S.vertex_case("one_cell", 257)
    f = _soup(257, 2049, 3)
    _, placed, info = _check(K, v, f, lo, cell, dims)
    assert len(info["reps"]) == 1 and int(info["rows"][0]) == 2049


def test_special_rows(K):
    """An empty row, a row of zero-area faces only, a face (a,a,b) and a face with two corners in one cluster."""
    lo, cell, dims = S.LO, S.CELL, S.DIMS
    pts = S._points(np.array([[0.5, 0.5, 0.5], [0.6, 0.4, 0.5], [1.5, 0.5, 0.5], [2.5, 0.5, 0.5], [3.5, 0.5, 0.5],
                              [0.5, 1.5, 0.5]]))
    faces = np.array([[0, 1, 2], [3, 3, 3], [0, 0, 5]], np.int32)
    _, placed, info = _check(K, pts, faces, lo, cell, dims)
    assert placed.tolist() == [1, 0, 1, 0, 0, 0] and info["rows"].tolist() == [2, 1, 1, 0, 1]  # each face once


def test_large_triangle(K):
    """A triangle thousands of cells wide next to small ones: the local coordinates are large, nothing overflows."""
    v, lo, cell, dims = S.vertex_case("random", 65)
    v = v.copy()
    v[:3] = np.array([[-900.0, 2.0, 3.0], [1.0, 1200.0, 2.5], [0.5, 0.7, -1500.0]], np.float32)
    f = np.concatenate([np.array([[0, 1, 2], [0, 5, 2], [1, 7, 9]], np.int32), _soup(65, 100, 5)])
    _, placed, _ = _check(K, v, f, lo, cell, dims)
    assert bool(np.isfinite(v).all())


def _ridge():
    """Two members of cell (2,1,1), each on a plane; the planes meet in a ridge 0.82 cells above the cell's centre,
    outside the cell: the solution is rejected and the cluster keeps its mean."""
    a = np.deg2rad(70.0)
    A, B = np.array([2.2, 1.5, 1.5]), np.array([2.8, 1.5, 1.5])
    d1, d2 = np.array([np.cos(a), np.sin(a), 0.0]), np.array([-np.cos(a), np.sin(a), 0.0])
    ez = np.array([0.0, 0.0, 1.0])
    cells = np.stack([A, A + 3 * d1, A + 3 * ez, B, B + 3 * d2, B + 3 * ez])
    return S._points(cells), np.array([[0, 1, 2], [3, 4, 5]], np.int32)


def test_solution_outside_the_cell(K):
    v, f = _ridge()
    pos, placed, info = _check(K, v, f, S.LO, S.CELL, (5, 5, 5))
    labels = S.cluster_labels(v, S.LO, S.CELL, (5, 5, 5))
    assert labels[3] == 0 and info["rank"][0] == 2 and placed[0] == 0  # two planes were solved for, then rejected
    mean, _, _ = S.cluster_reduce(v, labels, S.LO, S.CELL, (5, 5, 5))
    assert pos[0].tobytes() == mean[0].tobytes()


def test_tol_changes_the_rank(K):
    v, f = Q.sphere_mesh()
    cell = np.float32(0.2)
    lo, dims = S.simplify_grid(v, cell)
    fine_pos, _, fine = _check(K, v, f, lo, cell, dims, tol=1e-3)
    coarse_pos, _, coarse = _check(K, v, f, lo, cell, dims, tol=0.3)
    assert (coarse["rank"] <= fine["rank"]).all() and (coarse["rank"] < fine["rank"]).any()
    assert fine_pos.tobytes() != coarse_pos.tobytes()


def test_arguments(K):
    v, lo, cell, dims = S.vertex_case("random", 65)
    f = _soup(65, 131, 1)
    dv, df, labels, row_off, col, mean = _device_inputs(K, v, f, lo, cell, dims)
    ok = dict(vertices=dv, faces=df, labels=labels, row_off=row_off, col=col, mean=mean, lo=lo, cell=cell, dims=dims)
    pos, placed = K.mesh_cluster_quadric(**ok)
    assert tuple(pos.shape) == (65, 3) and tuple(placed.shape) == (65,)
    bad_f = df.clone()
    bad_f[5, 1] = 65
    bad_col = col.clone()
    bad_col[0] = 131
    bad = [dict(vertices=dv.double()), dict(vertices=dv.cpu()), dict(vertices=dv.reshape(-1)), dict(vertices=dv[:64]),
           dict(faces=df.long()), dict(faces=df.cpu()), dict(faces=df.reshape(-1)), dict(faces=bad_f),
           dict(labels=labels.long()), dict(labels=labels[:64]), dict(labels=labels.cpu()), dict(labels=labels + 65),
           dict(row_off=row_off[:-1]), dict(row_off=row_off.long()), dict(row_off=row_off.flip(0).contiguous()),
           dict(col=col.long()), dict(col=col.cpu()), dict(col=col[:-1]), dict(col=col.reshape(1, -1)),
           dict(col=bad_col),
           dict(mean=mean[:64]), dict(mean=mean.double()), dict(mean=mean.cpu()), dict(mean=mean.reshape(-1)),
           dict(tol=0.0), dict(tol=1.0), dict(tol=-1e-3), dict(tol=2.0), dict(tol=float("nan")),
           dict(tol=float("inf")), dict(tol="small"),
           dict(cell=0.0), dict(dims=(5, 4)), dict(lo=(0.0, 1.0))]
    for kw in bad:
        with pytest.raises(ValueError):
            K.mesh_cluster_quadric(**{**ok, **kw})
    e3 = torch.empty((0, 3), device=DEV)
    ei = torch.empty(0, dtype=torch.int32, device=DEV)
    zero = torch.zeros(1, dtype=torch.int32, device=DEV)
    pos, placed = K.mesh_cluster_quadric(e3, df[:0], ei, zero, ei, e3, lo, cell, dims)
    assert tuple(pos.shape) == (0, 3) and tuple(placed.shape) == (0,) and placed.dtype == torch.uint8
    # no face at all: every representative keeps its mean
    none_ro, none_col = K.mesh_vertex_faces(df[:0], 65)
    pos, placed = K.mesh_cluster_quadric(dv, df[:0], labels, none_ro, none_col, mean, lo, cell, dims)
    assert _bits(pos) == _bits(mean) and not bool(placed.any())


# ------------------------------------------------------------------ Mesh.simplify


def _mesh(name, attributes=True):
    from nerf_amd import Mesh
    v, f, n = S.extracted(name)
    if not attributes:
        return Mesh(_dev(v), _dev(f))
    return Mesh(_dev(v), _dev(f), _dev(n), _dev(S.vertex_colors(len(v))))


def _assert_mesh(mesh, rv, rf, rn, rc):
    assert mesh.faces.dtype == torch.int32 and np.array_equal(mesh.faces.cpu().numpy(), rf)
    _same_bits(mesh.vertices, rv)
    for got, ref in ((mesh.normals, rn), (mesh.colors, rc)):
        if ref is None:
            assert got is None
        else:
            _same_bits(got, ref)


@pytest.mark.parametrize("name,factor", S.MESH_CASES)
def test_simplify_quadric(K, name, factor):
    mesh = _mesh(name)
    cell = np.float32(factor * S.lattice_spacing(name))
    rv, rf, rn, rc, _ = Q.simplified(name, factor)
    out = mesh.simplify(cell, placement="quadric")
    _assert_mesh(out, rv, rf, rn, rc)
    mean = mesh.simplify(cell)
    assert torch.equal(out.faces, mean.faces) and torch.equal(out.normals, mean.normals)
    assert torch.equal(out.colors, mean.colors) and not torch.equal(out.vertices, mean.vertices)


def test_simplify_mean_is_unchanged(K):
    """placement="mean" and the default: the reference of the mean placement, bit for bit."""
    mesh = _mesh("noise")
    cell = np.float32(1.5 * S.lattice_spacing("noise"))
    rv, rf, rn, rc, _ = S.simplified("noise", 1.5)
    _assert_mesh(mesh.simplify(cell), rv, rf, rn, rc)
    _assert_mesh(mesh.simplify(cell, placement="mean"), rv, rf, rn, rc)
    _assert_mesh(mesh.simplify(cell, placement="mean", tol=0.5), rv, rf, rn, rc)


def test_simplify_options(K):
    v, f, _ = S.extracted("spheres")
    mesh = _mesh("spheres", False)
    cell = np.float32(1.5 * S.lattice_spacing("spheres"))
    origin = (v.min(0) - np.float32(0.37) * cell).astype(np.float32)
    rv, rf, _, _, _ = Q.simplify(v, f, cell, origin=origin, tol=0.05)
    _assert_mesh(mesh.simplify(cell, origin=origin.tolist(), placement="quadric", tol=0.05), rv, rf, None, None)
    for kw in (dict(placement="median"), dict(placement=None), dict(placement="quadric", tol=0.0),
               dict(placement="quadric", tol=1.0), dict(placement="quadric", tol=float("nan"))):
        with pytest.raises(ValueError):
            mesh.simplify(cell, **kw)
    from nerf_amd import Mesh
    empty = Mesh(_dev(v), torch.empty((0, 3), dtype=torch.int32, device=DEV)).simplify(0.1, placement="quadric")
    assert tuple(empty.vertices.shape) == (0, 3) and tuple(empty.faces.shape) == (0, 3)


def test_cube_volume(K):
    """The cube on the device: faces stay planes, edges edges and corners corners, so the volume is the cube's."""
    from nerf_amd import Mesh
    v, f, cell, origin = Q.cube_case()
    mesh = Mesh(_dev(v), _dev(f))
    quad = mesh.simplify(cell, origin=origin.tolist(), placement="quadric")
    mean = mesh.simplify(cell, origin=origin.tolist())
    print(f"cube volume: {quad.volume():.9f} (quadric), {mean.volume():.6f} (mean); "
          f"V {len(v)} -> {quad.vertices.shape[0]}")
    assert abs(quad.volume() - 1.0) <= 1e-5
    assert mean.volume() < 0.98
    assert Q.cube_surface_distance(quad.vertices.cpu().numpy()).max() <= 1e-6


# ------------------------------------------------------------------ extract_mesh


def _sphere_density(x):
    return 0.6 - x.norm(dim=-1, keepdim=True)


def test_extract_mesh_placement(K):
    from nerf_amd import extract_mesh
    lo, hi, res, cell = [-1.0] * 3, [1.0] * 3, 16, 0.2
    plain = extract_mesh(_sphere_density, lo, hi, res, 0.0, device=DEV)
    ref = plain.simplify(cell, placement="quadric")
    got = extract_mesh(_sphere_density, lo, hi, res, 0.0, device=DEV, simplify=cell, simplify_placement="quadric")
    assert torch.equal(got.vertices, ref.vertices) and torch.equal(got.faces, ref.faces)
    assert torch.equal(got.normals, ref.normals)
    mean = extract_mesh(_sphere_density, lo, hi, res, 0.0, device=DEV, simplify=cell)
    named = extract_mesh(_sphere_density, lo, hi, res, 0.0, device=DEV, simplify=cell, simplify_placement="mean")
    assert torch.equal(mean.vertices, named.vertices) and torch.equal(mean.vertices, plain.simplify(cell).vertices)
    assert torch.equal(mean.faces, got.faces) and not torch.equal(mean.vertices, got.vertices)
    exact = 4.0 * np.pi * 0.6 ** 3 / 3.0
    print(f"sphere r=0.6: volume {plain.volume():.4f} extracted, {got.volume():.4f} quadric, {mean.volume():.4f} mean, "
          f"{exact:.4f} exact")
    assert abs(got.volume() - plain.volume()) < abs(mean.volume() - plain.volume())
    with pytest.raises(ValueError):
        extract_mesh(_sphere_density, lo, hi, res, 0.0, device=DEV, simplify=cell, simplify_placement="qem")


# ------------------------------------------------------------------ a model


@pytest.fixture(scope="module")
def model(K):
    import math
    import ngp_grad_cases as G
    from nerf_amd import ngp as N
    st = G.prod_state()
    st["sigma_head.bias"] = torch.full((1,), math.log(10.0))  # sigma = 10 exp(noise): crosses the threshold 10
    net = N.InstantNGP(occ_conf={}, scene_box=G.AABB, **G.PROD)
    net.load_reference_state(st)
    return net.to(DEV).eval()


RES, CELL = 20, 0.3  # the lattice spacing is 3 / 19


def test_model_extraction_placement(K, model):
    full = model.extract_mesh(resolution=RES, normals=None)
    ref = full.simplify(CELL, placement="quadric")
    got = model.extract_mesh(resolution=RES, normals="field", colors="linear", simplify=CELL,
                             simplify_placement="quadric")
    assert 0 < got.faces.shape[0] < full.faces.shape[0]
    assert torch.equal(got.vertices, ref.vertices) and torch.equal(got.faces, ref.faces)
    assert torch.equal(got.normals, model.normals(got.vertices))  # the networks ran at the placed vertices
    mean = model.extract_mesh(resolution=RES, normals=None, simplify=CELL)
    assert torch.equal(mean.vertices, full.simplify(CELL).vertices) and torch.equal(mean.faces, got.faces)
    assert not torch.equal(mean.vertices, got.vertices)
    with pytest.raises(ValueError):
        model.extract_mesh(resolution=RES, simplify=CELL, simplify_placement="qem")


def test_tsdf_extraction_placement(K, model):
    import math
    from nerf_amd.ray_rendering import fuse_depth_views
    from nerf_amd.scene import hemisphere_poses
    poses = hemisphere_poses(4, seed=0)
    n = 16
    focal = 0.5 * n / math.tan(0.5 * 0.6911112)
    cam = dict(H=n, W=n, fx=focal, fy=focal, cx=n / 2.0, cy=n / 2.0, near=2.0, far=6.0)
    kw = dict(resolution=16, ray_samples=32, batch=3)
    vol = fuse_depth_views(model, poses, lo=[-1.5] * 3, hi=[1.5] * 3, **cam, **kw)
    plain = vol.extract_mesh(normals=None)
    assert plain.faces.shape[0] > 0
    ref = plain.simplify(CELL, placement="quadric")
    got = vol.extract_mesh(normals=None, simplify=CELL, simplify_placement="quadric")
    assert torch.equal(got.vertices, ref.vertices) and torch.equal(got.faces, ref.faces)
    assert torch.equal(vol.extract_mesh(normals=None, simplify=CELL).vertices, plain.simplify(CELL).vertices)
    through = model.extract_mesh_tsdf(poses, **cam, normals=None, simplify=CELL, simplify_placement="quadric", **kw)
    assert torch.equal(through.vertices, ref.vertices) and torch.equal(through.faces, ref.faces)
    for call in (lambda: vol.extract_mesh(simplify=CELL, simplify_placement="qem"),
                 lambda: model.extract_mesh_tsdf(poses, **cam, simplify=CELL, simplify_placement="qem", **kw)):
        with pytest.raises(ValueError):
            call()
