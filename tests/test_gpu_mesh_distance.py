"""kernels.mesh_face_grid / mesh_nearest_faces (csrc/mesh_distance.hip), mesh_metrics.nearest_on_mesh,
Mesh.closest_points and mesh_distance(exact=True) on the device (-m gpu), against the numpy restatement of the contract
in tests/mesh_distance_reference.py.

d2 (float64), face and closest point are exact: bitwise equal to the reference's brute force over all faces.  The
float64 reductions of the metric dict are compared at rel 1e-9, the tolerance of tests/test_gpu_mesh_metrics.py: a
float64 sum of fewer than 2^20 terms differs between two orders by at most n 2^-53 ~ 1.2e-10 relative, with a margin
of 8.  Every input has a few thousand items at most and every reference is computed once per process.

The grid of 1024 cells per axis.  A query r cells from the surface walks r shells, about 4/3 r^3 columns, and measures
every face key of those cells, so on that grid only queries within a few cells of a face finish in seconds: the case
runs on tiny_face_mesh (2^18 + 1 keys) with mesh_distance_reference.cap_queries, 900 queries around the faces and 100
below the box, all within 24 cells per axis of a face.  soup60 has 1.4e9 keys on that grid (11 GB, and a far query
would measure every one of them), so its fine grid has 32 cells per axis (54244 keys, faces spanning up to 20 cells
per axis) with the full query set, the 100 far queries included."""
import numpy as np
import pytest
import torch

import mesh_distance_reference as D
import mesh_metrics_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
REL = 1e-9
MESHES = {"soup60": D.soup60, "tiny_face": D.tiny_face_mesh}


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


def _same(got, ref):
    """(d2, face, closest) of the device against the reference's, bit for bit"""
    assert len(got) == 3
    for g, r, dtype in zip(got, ref, (torch.float64, torch.int32, torch.float32)):
        assert g.dtype == dtype and tuple(g.shape) == tuple(r.shape)
        assert g.cpu().numpy().tobytes() == np.ascontiguousarray(r).tobytes()


# ------------------------------------------------------------------ the closest point


def test_single_triangle_regions(Mesh, MM):
    v, f = D.TRIANGLE
    q = np.array([row[0] for row in D.TABLE], np.float32)
    mesh = Mesh(_dev(v), _dev(f))
    got = mesh.closest_points(_dev(q))
    _same(got, D.nearest_faces(v, f, q))
    assert got[0].tolist() == [row[1] for row in D.TABLE]
    for i, (_, _, point) in enumerate(D.TABLE):
        if point is not None:
            assert got[2][i].tolist() == list(point)
    again = MM.nearest_on_mesh(_dev(q), mesh)
    assert all(torch.equal(a, b) for a, b in zip(again, got))
    import nerf_amd
    assert nerf_amd.nearest_on_mesh is MM.nearest_on_mesh


@pytest.mark.parametrize("cell", ("default", "one_cell", "fine"))
@pytest.mark.parametrize("name", tuple(MESHES))
def test_meshes_with_flat_and_spanning_faces(K, name, cell):
    v, f = MESHES[name]()
    if cell == "fine" and name == "tiny_face":
        cell_size, q, ref, dims = D.cap_cell(v), D.cap_queries(), D.brute(name, "cap"), 1024
    else:
        cell_size = {"default": None, "one_cell": D.one_cell(v), "fine": D.cap_cell(v, 32)}[cell]
        q, ref, dims = D.queries(name), D.brute(name), {"default": None, "one_cell": 1, "fine": 32}[cell]
    vd, fd = _dev(v), _dev(f)
    grid = K.mesh_face_grid(vd, fd, cell_size)
    print(f"{name} {cell}: cell={grid['cell']:.4g} dims={grid['dims']} n_keys={grid['n_keys']}")
    assert dims is None or max(grid["dims"]) == dims
    assert grid["n_keys"] == int(D.face_cell_counts(v, f, D.face_grid(v, f, cell_size)).sum())
    _same(K.mesh_nearest_faces(_dev(q), vd, fd, grid), ref)
    assert np.isfinite(ref[0]).all()


def test_more_keys_than_the_limit(K):
    # three faces whose bounding box is the whole grid of 1024^3 cells: 3 2^30 keys
    v = np.array([[0, 0, 0], [1, 1, 0], [0, 1, 1]], np.float32)
    f = np.array([[0, 1, 2]] * 3, np.int32)
    with pytest.raises(ValueError, match="2\\^31"):
        K.mesh_face_grid(_dev(v), _dev(f), D.cap_cell(v))


def test_ties_take_the_smaller_face(Mesh):
    v, f = D.soup60()
    q = D.queries("soup60")[:300]
    twice = np.concatenate([f, f[::-1]])  # face 60 + k is face 59 - k again
    got = Mesh(_dev(v), _dev(twice)).closest_points(_dev(q))
    _same(got, D.nearest_faces(v, twice, q))
    assert int(got[1].max()) < 60
    rng = np.random.default_rng(23)
    for _ in range(4):
        mv, mf = D.mirror_pair(rng)
        mq = rng.uniform(-2, 2, (500, 3)).astype(np.float32)
        mq[:, 0] = 0
        ref = D.nearest_faces(mv, mf, mq)
        for faces in (mf, mf[::-1].copy()):  # either triangle first: index 0 wins
            got = Mesh(_dev(mv), _dev(faces)).closest_points(_dev(mq))
            assert bool((got[1] == 0).all()) and got[0].cpu().numpy().tobytes() == ref[0].tobytes()
        _same(Mesh(_dev(mv), _dev(mf)).closest_points(_dev(mq)), ref)


def test_empty_inputs(K, Mesh):
    v, f = D.soup60()
    q = _dev(D.queries("soup60")[:70])
    none = Mesh(_dev(v), torch.empty((0, 3), dtype=torch.int32, device=DEV))
    d2, face, closest = none.closest_points(q)
    assert d2.dtype == torch.float64 and bool(torch.isinf(d2).all()) and bool((d2 > 0).all())
    assert face.dtype == torch.int32 and bool((face == -1).all()) and torch.equal(closest, q)
    grid = K.mesh_face_grid(none.vertices, none.faces)
    assert grid["n_keys"] == 0 and grid["F"] == 0 and grid["dims"] == [1, 1, 1] and tuple(grid["keys"].shape) == (0,)
    d2, face, closest = Mesh(_dev(v), _dev(f)).closest_points(q[:0])
    assert tuple(d2.shape) == (0,) and d2.dtype == torch.float64
    assert tuple(face.shape) == (0,) and face.dtype == torch.int32
    assert tuple(closest.shape) == (0, 3) and closest.dtype == torch.float32
    assert len(K.mesh_nearest_faces(q, none.vertices, none.faces, grid, closest=False)) == 2


@pytest.mark.parametrize("n", (255, 256, 257))
def test_block_edges(Mesh, n):
    v, f = D.soup60()
    got = Mesh(_dev(v), _dev(f)).closest_points(_dev(D.queries("soup60")[:n]))
    _same(got, tuple(r[:n] for r in D.brute("soup60")))


def test_query_sorting_changes_nothing(K):
    v, f = D.soup60()
    vd, fd, q = _dev(v), _dev(f), _dev(D.queries("soup60"))
    grid = K.mesh_face_grid(vd, fd, D.cap_cell(v, 32))
    a = K.mesh_nearest_faces(q, vd, fd, grid, sort_queries=True)
    b = K.mesh_nearest_faces(q, vd, fd, grid, sort_queries=False)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    _same(b, D.brute("soup60"))
    short = K.mesh_nearest_faces(q, vd, fd, grid, closest=False)
    assert len(short) == 2 and torch.equal(short[0], a[0]) and torch.equal(short[1], a[1])


@pytest.mark.parametrize("name", tuple(MESHES))
def test_keys(K, name):
    v, f = MESHES[name]()
    for cell_size in (None, D.cap_cell(v, 32)):
        ref_grid = D.face_grid(v, f, cell_size)
        grid = K.mesh_face_grid(_dev(v), _dev(f), cell_size)
        assert set(grid) == {"keys", "lo", "cell", "inv", "dims", "n_keys", "F"} and grid["F"] == len(f)
        assert grid["lo"] == ref_grid["lo"].tolist() and grid["dims"] == ref_grid["dims"]
        assert grid["cell"] == float(ref_grid["cell"]) and grid["inv"] == float(ref_grid["inv"])
        keys = grid["keys"]
        assert keys.dtype == torch.int64 and tuple(keys.shape) == (grid["n_keys"],)
        assert bool((keys[1:] > keys[:-1]).all())
        want = D.face_keys(v, f, ref_grid)  # sorted: equal arrays are equal sets of (cell, face) pairs
        assert grid["n_keys"] == len(want) and np.array_equal(keys.cpu().numpy(), want)


def test_arguments(K, MM, Mesh):
    v, f = D.soup60()
    vd, fd, qd = _dev(v), _dev(f), _dev(D.queries("soup60")[:65])
    mesh = Mesh(vd, fd)
    grid = K.mesh_face_grid(vd, fd)
    nan_q, nan_v = qd.clone(), vd.clone()
    nan_q[5, 2] = float("inf")
    nan_v[3, 1] = float("nan")
    wide = torch.zeros((65, 6), dtype=torch.float32, device=DEV)
    for bad in (qd.cpu(), qd.double(), wide[:, ::2], qd.reshape(-1), qd[:, :2].contiguous(), nan_q):
        with pytest.raises(ValueError):
            MM.nearest_on_mesh(bad, mesh)
        with pytest.raises(ValueError):
            mesh.closest_points(bad)
        with pytest.raises(ValueError):
            K.mesh_nearest_faces(bad, vd, fd, grid)
    for bad in (Mesh(vd.cpu(), fd.cpu()), Mesh(vd.double(), fd), Mesh(vd, fd.long()), Mesh(nan_v, fd),
                Mesh(vd[:20].contiguous(), fd)):  # the last: indices out of range
        with pytest.raises(ValueError):
            bad.closest_points(qd)
        with pytest.raises(ValueError):
            K.mesh_face_grid(bad.vertices, bad.faces)
        with pytest.raises(ValueError):
            K.mesh_nearest_faces(qd, bad.vertices, bad.faces, grid)
    for bad_cell in (0.0, -1.0, float("nan"), float("inf"), 1e-4, "x"):  # 1e-4: about 20000 cells along an axis
        with pytest.raises(ValueError):
            mesh.closest_points(qd, cell_size=bad_cell)
        with pytest.raises(ValueError):
            K.mesh_face_grid(vd, fd, bad_cell)
    for bad_grid in ({"keys": None}, None, K.points_grid(vd), {**grid, "F": 59}, {**grid, "keys": grid["keys"][:-1]},
                     {**grid, "keys": grid["keys"].cpu()}, {**grid, "keys": grid["keys"].to(torch.int32)}):
        with pytest.raises(ValueError):
            K.mesh_nearest_faces(qd, vd, fd, bad_grid)
    with pytest.raises(ValueError):
        mesh.distance_to((v, f), exact=True)


# ------------------------------------------------------------------ against the point-set distance


def test_exact_never_exceeds_point_set(Mesh, MM):
    v, f = D.spheres()
    moved = (v + np.float32(0.02)).astype(np.float32)
    a, b = Mesh(_dev(v), _dev(f)), Mesh(_dev(moved), _dev(f))
    m = D.margin(v, moved)
    sa, sb = a.sample_surface(3000, seed=1)[0], b.sample_surface(3000, seed=2)[0]
    for samples, other, other_samples in ((sa, b, sb), (sb, a, sa)):
        exact = torch.sqrt(other.closest_points(samples)[0])
        point_set = torch.sqrt(MM.nearest_points(samples, other_samples)[0].to(torch.float64))
        print(f"exact mean {float(exact.mean()):.6f}, point-set mean {float(point_set.mean()):.6f}, m {m:.3g}")
        assert bool((exact <= point_set + m).all())
        assert float(exact.mean()) < float(point_set.mean())


def test_self_distance_has_no_sampling_floor(Mesh, MM):
    # the reference alone, n = 1500: the largest exact distance is 5.6e-8, m = 2.9e-7, the point-set mean 0.0257
    v, f = D.spheres()
    mesh = Mesh(_dev(v), _dev(f))
    m = D.margin(v)
    n = 1500
    d = torch.sqrt(mesh.closest_points(mesh.sample_surface(n, seed=1)[0])[0])
    floor = MM.point_set_metrics(mesh.sample_surface(n, seed=1)[0], mesh.sample_surface(n, seed=2)[0])["a_to_b_mean"]
    print(f"largest exact self-distance {float(d.max()):.3g} <= m = {m:.3g}; point-set a_to_b_mean {floor:.3g}")
    assert bool((d <= m).all())
    assert floor > 100 * m
    same = mesh.distance_to(mesh, n_samples=n, seed=1, exact=True)
    assert same["hausdorff"] <= m and same["chamfer"] <= m


def _close(got, ref):
    assert list(got) == list(ref)
    for key, want in ref.items():
        assert isinstance(got[key], float)
        if key.startswith(("precision@", "recall@")):
            assert got[key] == want, key  # a share of exact comparisons
        else:
            assert abs(got[key] - want) <= REL * abs(want), (key, got[key], want)


def test_mesh_distance_exact(MM, Mesh):
    # 2048 samples: a share of them is a count times a power of two, exact however the division is carried out
    v, f = D.spheres()
    moved = (v * np.float32(1.05)).astype(np.float32)
    ref = D.mesh_distance_exact((v, f), (moved, f), 2048, seed=3, thresholds=(0.02, 0.1), normals=True)
    a, b = Mesh(_dev(v), _dev(f)), Mesh(_dev(moved), _dev(f))
    got = MM.mesh_distance(a, b, 2048, seed=3, thresholds=(0.02, 0.1), normals=True, exact=True)
    print({k: round(x, 6) for k, x in got.items()})
    _close(got, ref)
    assert a.distance_to(b, n_samples=2048, seed=3, thresholds=(0.02, 0.1), normals=True, exact=True) == got
    assert MM.mesh_distance(a, b, 2048, seed=3, thresholds=(0.02, 0.1), normals=True, exact=True, cell_size=0.3) == got
    plain = MM.mesh_distance(a, b, 2048, seed=3, exact=True)
    assert "normal_consistency" not in plain and plain == {k: got[k] for k in plain}
    point_set = MM.mesh_distance(a, b, 2048, seed=3)
    assert got["chamfer"] < point_set["chamfer"] and got["hausdorff"] <= point_set["hausdorff"] + D.margin(v, moved)


def test_exact_false_is_the_point_set_path(MM, Mesh):
    v, f = D.spheres()
    moved = (v * np.float32(1.05)).astype(np.float32)
    a, b = Mesh(_dev(v), _dev(f)), Mesh(_dev(moved), _dev(f))
    kwargs = dict(seed=3, thresholds=(0.02, 0.1), normals=True)
    want = MM.mesh_distance(a, b, 2000, **kwargs)
    assert MM.mesh_distance(a, b, 2000, exact=False, **kwargs) == want
    assert a.distance_to(b, n_samples=2000, exact=False, **kwargs) == want
    _close(want, R.mesh_distance((v, f), (moved, f), 2000, **kwargs))
