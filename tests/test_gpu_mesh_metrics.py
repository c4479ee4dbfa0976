"""kernels.mesh_face_areas / mesh_sample_surface / points_grid / points_nearest (csrc/mesh_metrics.hip), the Mesh
methods face_areas / area / sample_surface / distance_to and nerf_amd.mesh_metrics on the device (-m gpu), against the
numpy restatement of the contract in tests/mesh_metrics_reference.py.

Samples, areas and nearest neighbours are exact: bitwise floats, equal integers.  The float64 reductions of the metric
dict are compared at rel 1e-9: a float64 sum of fewer than 2^20 terms differs between two orders by at most
n 2^-53 ~ 1.2e-10 relative, with a margin of 8.  Every input has a few thousand items at most and every reference is
computed once per process."""
import math

import numpy as np
import pytest
import torch

import mesh_metrics_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
REL = 1e-9
MESHES = tuple(R.sample_meshes())
NN = tuple(R.nn_cases())


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from nerf_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def MM(K):
    from nerf_amd import mesh_metrics
    return mesh_metrics


@pytest.fixture(scope="module")
def Mesh(K):
    from nerf_amd import Mesh
    return Mesh


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same_bits(got, ref, dtype=torch.float32):
    assert got.dtype == dtype and tuple(got.shape) == tuple(ref.shape)
    assert got.cpu().numpy().tobytes() == np.ascontiguousarray(ref).tobytes()


def _same_ints(got, ref, dtype=torch.int32):
    assert got.dtype == dtype and tuple(got.shape) == tuple(ref.shape)
    assert np.array_equal(got.cpu().numpy(), ref)


def _mesh(Mesh, name, normals=False):
    v, f, vn = R.sample_meshes()[name]
    return Mesh(_dev(v), _dev(f), _dev(vn) if normals else None)


# ------------------------------------------------------------------ areas and samples


@pytest.mark.parametrize("name", MESHES)
def test_face_areas(K, Mesh, name):
    v, f, _ = R.sample_meshes()[name]
    ref = R.face_areas(v, f)
    mesh = _mesh(Mesh, name)
    _same_bits(mesh.face_areas(), ref, torch.float64)
    total = mesh.area()
    assert isinstance(total, float) and abs(total - ref.sum()) <= REL * ref.sum()
    cdf, tot = K.mesh_area_cdf(mesh.face_areas())
    _same_ints(cdf, R.area_cdf(ref)[1], torch.int64)
    assert tot == R.area_cdf(ref)[2]


@pytest.mark.parametrize("seed", R.SAMPLE_SEEDS)
@pytest.mark.parametrize("n", R.SAMPLE_N)
@pytest.mark.parametrize("name", MESHES)
def test_sample_surface(Mesh, name, n, seed):
    mesh = _mesh(Mesh, name, normals=True)
    for kind in (None, "face", "vertex"):
        pts, face, nrm, _ = R.sampled(name, n, seed, kind)
        got = mesh.sample_surface(n, seed=seed, normals=kind)
        assert len(got) == (2 if kind is None else 3)
        _same_bits(got[0], pts)
        _same_ints(got[1], face)
        if kind is not None:
            _same_bits(got[2], nrm)
    if name == "tiny_face" and n:
        assert (got[1] == 1).all()  # the face 2^-34 times the other's area is never picked


def test_sample_arguments(K, Mesh):
    v, f, vn = R.sample_meshes()["soup60"]
    vd, fd = _dev(v), _dev(f)
    mesh = Mesh(vd, fd)
    for bad_n in (-1, 1.5, True, "3", 2 ** 31):
        with pytest.raises(ValueError):
            mesh.sample_surface(bad_n)
    for bad_seed in (-1, 2 ** 64, 0.5):
        with pytest.raises(ValueError):
            mesh.sample_surface(4, seed=bad_seed)
    with pytest.raises(ValueError):
        mesh.sample_surface(4, normals="grid")
    with pytest.raises(ValueError):
        mesh.sample_surface(4, normals="vertex")  # the mesh has no vertex normals
    with pytest.raises(ValueError):
        K.mesh_sample_surface(vd, fd, 4, normals="vertex", vertex_normals=_dev(vn)[:-1])
    bad_v = vd.clone()
    bad_v[3, 1] = float("nan")
    for bad in (Mesh(vd.cpu(), fd.cpu()), Mesh(vd.double(), fd), Mesh(vd, fd.long()), Mesh(bad_v, fd),
                Mesh(vd[:20].contiguous(), fd)):  # the last: indices out of range
        with pytest.raises(ValueError):
            bad.sample_surface(4)
        with pytest.raises(ValueError):
            bad.face_areas()
    dead = Mesh(vd, _dev(f[list(R.SOUP_DEAD)]))
    assert dead.area() == 0.0
    with pytest.raises(ValueError):
        dead.sample_surface(4)  # no face with area
    empty = Mesh(vd, torch.empty((0, 3), dtype=torch.int32, device=DEV))
    assert tuple(empty.face_areas().shape) == (0,) and empty.face_areas().dtype == torch.float64 and empty.area() == 0.0
    with pytest.raises(ValueError):
        empty.sample_surface(1)
    for m in (mesh, dead, empty):
        pts, face, nrm = m.sample_surface(0, normals="face")
        assert tuple(pts.shape) == (0, 3) and pts.dtype == torch.float32
        assert tuple(face.shape) == (0,) and face.dtype == torch.int32
        assert tuple(nrm.shape) == (0, 3) and nrm.dtype == torch.float32


# ------------------------------------------------------------------ nearest neighbour


@pytest.mark.parametrize("sort_queries", (True, False))
@pytest.mark.parametrize("name", NN)
def test_nearest(K, MM, name, sort_queries):
    q, ref, cell = R.nn_cases()[name]
    d2, idx = R.nn_reference(name)
    grid = K.points_grid(_dev(ref), cell)
    print(f"{name}: n={len(q)} m={len(ref)} cell={grid['cell']:.4g} dims={grid['dims']}")
    assert max(grid["dims"]) <= 1024 and min(grid["dims"]) >= 1
    if name == "flat":
        assert grid["dims"][2] == 1
    if name.startswith("one_cell"):
        assert grid["dims"] == [1, 1, 1]
    got = K.points_nearest(_dev(q), grid, sort_queries=sort_queries)
    _same_bits(got[0], d2)
    _same_ints(got[1], idx)
    if sort_queries:
        again = MM.nearest_points(_dev(q), _dev(ref), cell)
        assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])


def test_default_cell_rule(K):
    pts = _dev(R.nn_cases()["random3000"][1])
    grid = K.points_grid(pts)
    k = math.ceil(math.sqrt(3000) / 2)
    ext = (pts.max(0).values - pts.min(0).values).cpu().numpy()
    assert grid["cell"] == float(ext.max() / np.float32(k)) and grid["inv"] == float(np.float32(1) / np.float32(grid["cell"]))
    assert grid["lo"] == pts.min(0).values.tolist() and max(grid["dims"]) in (k, k + 1)
    assert grid["keys"].dtype == torch.int64 and bool((grid["keys"][1:] > grid["keys"][:-1]).all())
    order = (grid["keys"] & 0xffffffff)
    assert torch.equal(grid["points"], pts[order]) and sorted(order.tolist()) == list(range(3000))
    same = K.points_grid(_dev(np.tile(np.float32([[1, 2, 3]]), (7, 1))))
    assert same["cell"] == 1.0 and same["dims"] == [1, 1, 1]


def test_nearest_arguments(K, MM):
    q, ref, _ = R.nn_cases()["n65"]
    qd, rd = _dev(q), _dev(ref)
    nan = rd.clone()
    nan[5, 2] = float("inf")
    wide = torch.zeros((65, 6), dtype=torch.float32, device=DEV)
    for bad in (qd.cpu(), qd.double(), wide[:, ::2], qd.reshape(-1), qd[:, :2].contiguous(), nan):
        with pytest.raises(ValueError):
            MM.nearest_points(bad, rd)
        with pytest.raises(ValueError):
            MM.nearest_points(qd, bad)
        with pytest.raises(ValueError):
            MM.point_set_metrics(bad, rd)
        with pytest.raises(ValueError):
            MM.point_set_metrics(qd, bad)
    for bad_cell in (0.0, -1.0, float("nan"), float("inf"), 1e-4, "x"):  # 1e-4: about 20000 cells along an axis
        with pytest.raises(ValueError):
            MM.nearest_points(qd, rd, cell_size=bad_cell)
        with pytest.raises(ValueError):
            K.points_grid(rd, bad_cell)
    with pytest.raises(ValueError):
        K.points_nearest(qd, {"keys": None})
    with pytest.raises(ValueError):
        MM.point_set_metrics(qd, rd, thresholds=(-1.0,))
    with pytest.raises(ValueError):
        MM.point_set_metrics(qd, rd, normals_a=qd)
    with pytest.raises(ValueError):
        MM.point_set_metrics(qd, rd[:0])
    d2, idx = MM.nearest_points(qd[:0], rd)
    assert tuple(d2.shape) == (0,) and d2.dtype == torch.float32 and tuple(idx.shape) == (0,) and idx.dtype == torch.int32
    d2, idx = MM.nearest_points(qd, rd[:0])
    assert d2.dtype == torch.float32 and bool(torch.isinf(d2).all()) and idx.dtype == torch.int32 and bool((idx == -1).all())


# ------------------------------------------------------------------ metrics


def _close(got, ref):
    assert list(got) == list(ref)
    for key, want in ref.items():
        assert isinstance(got[key], float)
        if key.startswith(("precision@", "recall@")):
            assert got[key] == want, key  # a share of exact comparisons
        else:
            assert abs(got[key] - want) <= REL * abs(want), (key, got[key], want)


def test_point_set_metrics(MM):
    a, b, na, nb = R.metric_sets()
    ref = R.metric_reference()
    got = MM.point_set_metrics(_dev(a), _dev(b), R.THRESHOLDS, _dev(na), _dev(nb))
    print({k: round(v, 6) for k, v in got.items()})
    _close(got, ref)
    plain = MM.point_set_metrics(_dev(a), _dev(b))
    assert "normal_consistency" not in plain and plain == {k: got[k] for k in plain}
    assert 0 < got["precision@0.01"] < 1 and got["precision@0.5"] == 1.0 and 0 < got["normal_consistency"] <= 1


def test_mesh_distance(MM, Mesh):
    v, f, _ = R.sample_meshes()["spheres"]
    moved = (v * np.float32(1.05)).astype(np.float32)
    ref = R.mesh_distance((v, f), (moved, f), 2000, seed=3, thresholds=(0.02, 0.1), normals=True)
    a, b = Mesh(_dev(v), _dev(f)), Mesh(_dev(moved), _dev(f))
    got = MM.mesh_distance(a, b, 2000, seed=3, thresholds=(0.02, 0.1), normals=True)
    _close(got, ref)
    # reproducible: two runs give identical dicts, and the method is the function
    assert MM.mesh_distance(a, b, 2000, seed=3, thresholds=(0.02, 0.1), normals=True) == got
    assert a.distance_to(b, n_samples=2000, seed=3, thresholds=(0.02, 0.1), normals=True) == got
    # a mesh against itself with the same seed: exactly zero
    zero = a.distance_to(a, n_samples=2000, seed=3, thresholds=(0.0,))
    assert zero["chamfer"] == 0.0 and zero["chamfer_sq"] == 0.0 and zero["hausdorff"] == 0.0 and zero["fscore@0.0"] == 1.0
    assert a.distance_to(b, n_samples=2000, seed=3, thresholds=(1e-6,))["fscore@1e-06"] == 0.0  # P + R == 0
    for bad in (0, -5, 2.5, True):
        with pytest.raises(ValueError):
            MM.mesh_distance(a, b, bad)
    with pytest.raises(ValueError):
        a.distance_to((v, f))


# ------------------------------------------------------------------ end to end

# The sampling spacing allowed on top of the geometric bound: SPACING_FACTOR sqrt(area / n_samples).  A sample's nearest
# sample of the other set lies within rho with probability 1 - exp(-pi rho^2 n / area); over n samples the largest
# such rho is about sqrt(ln(n) / pi) = 1.78 spacings at n = 20000, and 3 spacings are exceeded with probability
# n exp(-9 pi) ~ 1e-8.  Measured on the reference (two sample sets of the 24^3 sphere, seeds 0 and 1, n = 20000):
# hausdorff = 1.72 spacings (the mean nearest-sample distance 0.50).
SPACING_FACTOR = 3.0


def test_simplify_distance_end_to_end(Mesh):
    v, f = R.sphere()
    mesh = Mesh(_dev(v), _dev(f))
    n = R.E2E_SAMPLES
    hausdorff, chamfer = [], []
    for cell in R.E2E_CELLS:
        simple = mesh.simplify(cell)
        m = simple.distance_to(mesh, n_samples=n)
        spacing = math.sqrt(max(mesh.area(), simple.area()) / n)
        bound = math.sqrt(3.0) * cell + SPACING_FACTOR * spacing
        print(f"cell {cell}: V {simple.vertices.shape[0]}, hausdorff {m['hausdorff']:.4f} <= {bound:.4f}, "
              f"chamfer {m['chamfer']:.4f}, spacing {spacing:.4f}")
        assert m["hausdorff"] <= bound  # clustering moves a vertex by at most a cell diagonal
        hausdorff.append(m["hausdorff"])
        chamfer.append(m["chamfer"])
    assert hausdorff[0] < hausdorff[1] < hausdorff[2] and chamfer[0] < chamfer[1] < chamfer[2]
