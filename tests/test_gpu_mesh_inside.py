"""kernels.mesh_point_crossings / box_points (csrc/mesh_inside.hip), mesh_metrics.points_in_mesh /
signed_distance_to_mesh / volume_iou and Mesh.contains / signed_distance / volume / iou on the device (-m gpu), against
the restatement of the contract in tests/mesh_inside_reference.py.

crossings and winding are exact: equal to the reference's brute force over all faces, whose in-projection test is
rational arithmetic.  Every query set has one to two and a half thousand queries, every mesh at most 1388 faces, and
every reference is computed once per process.  The grids are those of the distance tests: one cell, the default,
and the cap, 1024 cells per axis for tiny_face and 32 per axis for the others."""
import math

import numpy as np
import pytest
import torch

import mesh_inside_reference as R
import mesh_raycast_reference as RC

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAMES = ("sphere12", "spheres", "soup60", "tiny_face")
GRIDS = ("one_cell", "default", "cap")


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
    """(crossings, winding) of the device against the reference's, exactly"""
    assert len(got) == 2
    for g, r in zip(got, ref):
        assert g.dtype == torch.int32 and tuple(g.shape) == tuple(r.shape)
        assert np.array_equal(g.cpu().numpy(), r)


# ------------------------------------------------------------------ the rule


def test_table_on_one_triangle(K):
    v, f = R.TRIANGLE
    xy = np.array([q for q, _ in R.TABLE], np.float32)
    want = np.array([c for _, c in R.TABLE], np.int32)
    for faces, sign in ((f, 1), (np.ascontiguousarray(f[:, ::-1]), -1)):
        vd, fd = _dev(v), _dev(faces)
        grid = K.mesh_face_grid(vd, fd)
        for qz, counts in ((-1.0, want), (0.0, 0 * want), (1.0, 0 * want)):
            q = np.concatenate([xy, np.full((len(xy), 1), qz, np.float32)], 1)
            got = K.mesh_point_crossings(_dev(q), vd, fd, grid)
            _same(got, (counts, sign * counts))
            _same(got, R.brute(v, faces, q))


def test_octahedron(K, Mesh):
    v, f = RC.octahedron()
    mesh = Mesh(_dev(v), _dev(f))
    q = np.array([q for q, _ in R.OCTAHEDRON], np.float32)
    got = K.mesh_point_crossings(_dev(q), mesh.vertices, mesh.faces, K.mesh_face_grid(mesh.vertices, mesh.faces))
    _same(got, tuple(np.array([w[k] for _, w in R.OCTAHEDRON], np.int32) for k in range(2)))
    assert mesh.contains(_dev(q)).tolist() == [True, False, False, False, False, True]
    assert mesh.volume() == pytest.approx(4.0, rel=1e-12)


# ------------------------------------------------------------------ the walk


@pytest.mark.parametrize("which", GRIDS)
@pytest.mark.parametrize("name", NAMES)
def test_counts_equal_brute_force_on_three_grids(K, name, which):
    v, f = R.mesh(name)
    vd, fd = _dev(v), _dev(f)
    grid = K.mesh_face_grid(vd, fd, R.grid_cell(name, which))
    print(f"{name} {which}: cell={grid['cell']:.4g} dims={grid['dims']} n_keys={grid['n_keys']}")
    if which != "default":
        assert max(grid["dims"]) == (1 if which == "one_cell" else 1024 if name == "tiny_face" else 32)
    q, ref = R.queries(name), R.brute_of(name)
    assert len(q) == (2528 if name == "sphere12" else len(q)) and len(q) >= 1000
    qd = _dev(q)
    for sort_queries in (True, False):
        _same(K.mesh_point_crossings(qd, vd, fd, grid, sort_queries=sort_queries), ref)
        for n in (0, 1, 255, 256, 257):  # the block edge
            _same(K.mesh_point_crossings(qd[:n].contiguous(), vd, fd, grid, sort_queries=sort_queries),
                  tuple(r[:n] for r in ref))


def test_no_faces_and_no_queries(K, MM, Mesh):
    v, f = R.mesh("soup60")
    q = _dev(R.queries("soup60")[:70])
    none = Mesh(_dev(v), torch.empty((0, 3), dtype=torch.int32, device=DEV))
    grid = K.mesh_face_grid(none.vertices, none.faces)
    for got in K.mesh_point_crossings(q, none.vertices, none.faces, grid):
        assert got.dtype == torch.int32 and tuple(got.shape) == (70,) and not bool(got.any())
    assert not bool(none.contains(q).any()) and none.volume() == 0.0
    sd, face, closest = none.signed_distance(q)
    assert bool((sd == float("inf")).all()) and bool((face == -1).all()) and torch.equal(closest, q)
    mesh = Mesh(_dev(v), _dev(f))
    empty = torch.empty((0, 3), dtype=torch.float32, device=DEV)
    assert tuple(mesh.contains(empty).shape) == (0,) and mesh.contains(empty).dtype == torch.bool
    assert [tuple(t.shape) for t in mesh.signed_distance(empty)] == [(0,), (0,), (0, 3)]


# ------------------------------------------------------------------ the layers above


@pytest.mark.parametrize("name", ("sphere12", "soup60"))
def test_points_in_mesh_under_both_rules(K, MM, Mesh, name):
    v, f = R.mesh(name)
    mesh = Mesh(_dev(v), _dev(f))
    qd = _dev(R.queries(name))
    c, w = R.brute_of(name)
    grid = K.mesh_face_grid(mesh.vertices, mesh.faces)
    keys = grid["keys"].clone()
    for rule, want in (("parity", (c & 1).astype(bool)), ("winding", w != 0)):
        got = MM.points_in_mesh(qd, mesh, rule=rule)
        assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), want)
        assert torch.equal(mesh.contains(qd, rule=rule), got)
        assert torch.equal(mesh.contains(qd, rule=rule, grid=grid), got)  # a grid built once
        assert torch.equal(MM.points_in_mesh(qd, mesh, rule=rule, cell_size=R.grid_cell(name, "cap")), got)
    assert torch.equal(grid["keys"], keys)
    assert torch.equal(MM.points_in_mesh(qd, mesh), mesh.contains(qd))  # parity is the default
    if name == "soup60":
        assert ((c & 1).astype(bool) != (w != 0)).any()  # the two rules differ on a soup
    import nerf_amd
    for fn in ("points_in_mesh", "signed_distance_to_mesh", "volume_iou"):
        assert getattr(nerf_amd, fn) is getattr(MM, fn) and fn in nerf_amd.__all__


@pytest.mark.parametrize("name", ("sphere12", "soup60"))
def test_signed_distance(K, MM, Mesh, name):
    v, f = R.mesh(name)
    mesh = Mesh(_dev(v), _dev(f))
    q = R.queries(name)
    on_surface = v[f[1]].astype(np.float64).mean(0, keepdims=True).astype(np.float32)  # near a face
    q = np.concatenate([q, v[f[1:6, 0]], on_surface])  # five corners of faces: d2 == 0
    qd = _dev(q)
    d2, face, closest = mesh.closest_points(qd)
    c, w = R.brute(v, f, q[-6:])
    c, w = np.concatenate([R.brute_of(name)[0], c]), np.concatenate([R.brute_of(name)[1], w])
    for rule, inside in (("parity", (c & 1).astype(bool)), ("winding", w != 0)):
        for grid in (None, K.mesh_face_grid(mesh.vertices, mesh.faces)):
            sd, sface, sclosest = MM.signed_distance_to_mesh(qd, mesh, rule=rule, grid=grid)
            assert sd.dtype == torch.float64 and torch.equal(sface, face) and torch.equal(sclosest, closest)
            d2h, sdh = d2.cpu().numpy(), sd.cpu().numpy()
            zero = d2h == 0
            assert zero[-6:-1].all() and not np.signbit(sdh[zero]).any() and (sdh[zero] == 0).all()
            assert np.array_equal(sdh[~zero] < 0, inside[~zero]) and (sdh[~zero] != 0).all()  # the sign, exactly
            assert (np.abs(sdh * sdh - d2h) <= 2 * np.spacing(d2h)).all()  # sqrt rounds once, the square once
            assert all(torch.equal(a, b) for a, b in zip(mesh.signed_distance(qd, rule=rule, grid=grid),
                                                         (sd, sface, sclosest)))


def test_box_points(K):
    lo, hi = (-1.0, 0.5, 2.0), (1.0, 0.75, 2.0)
    for seed in (0, 0x9e3779b97f4a7c15):
        for n in (0, 1, 255, 256, 257, 4099):
            got = K.box_points(n, lo, hi, seed=seed, device=DEV)
            assert got.dtype == torch.float32 and tuple(got.shape) == (n, 3) and got.is_cuda
            assert got.cpu().numpy().tobytes() == R.box_points(n, seed, lo, hi).tobytes()
    assert torch.equal(K.box_points(64, lo, hi), K.box_points(64, _dev(np.array(lo, np.float32)), list(hi), seed=0))
    for bad in (dict(n=-1), dict(n=2 ** 31), dict(n=1.5), dict(n=True), dict(seed=-1), dict(seed=2 ** 64),
                dict(lo=(0, 0)), dict(lo=(2.0, 0.5, 2.0)), dict(lo=(float("nan"), 0, 0)), dict(hi=(float("inf"), 1, 3)),
                dict(lo="abc"), dict(device="cpu"), dict(lo=(-3e38, 0, 0), hi=(3e38, 1, 3))):
        args = {"n": 8, "lo": lo, "hi": hi, "seed": 0, **bad}
        with pytest.raises(ValueError):
            K.box_points(args.pop("n"), args.pop("lo"), args.pop("hi"), **args)


def test_volume_iou(K, MM, Mesh):
    v, f = R.sphere()
    sv, _ = R.shifted_sphere()
    a, b = Mesh(_dev(v), _dev(f)), Mesh(_dev(sv), _dev(f))
    same, ref = a.iou(a, n_samples=R.IOU_N, seed=R.IOU_SEED), R.iou_reference("self")
    assert same == ref and same["iou"] == 1.0
    # the Monte Carlo volume against the divergence theorem's: within 5 binomial standard errors
    lo, hi = same["box"]
    vol_box = R.box_volume(lo, hi)
    p = same["count_a"] / R.IOU_N
    se = vol_box * math.sqrt(p * (1 - p) / R.IOU_N)
    print(f"volume {a.volume():.5f} estimate {same['volume_a']:.5f} se {se:.5f}")
    assert a.volume() == pytest.approx(R.volume(v, f), rel=1e-12) and a.volume() > 0
    assert same["volume_a"] == pytest.approx(p * vol_box, rel=1e-12) and abs(same["volume_a"] - a.volume()) <= 5 * se
    other, ref = MM.volume_iou(a, b, n_samples=R.IOU_N, seed=R.IOU_SEED), R.iou_reference("shifted")
    for key in ("count_a", "count_b", "count_intersection", "count_union", "n_samples"):
        assert other[key] == ref[key] and isinstance(other[key], int), key
    assert other == ref and 0.0 < other["iou"] < 1.0
    assert other == a.iou(b, n_samples=R.IOU_N, seed=R.IOU_SEED)  # equal arguments, equal dicts
    assert other != a.iou(b, n_samples=R.IOU_N, seed=R.IOU_SEED + 1)
    assert a.iou(b, n_samples=R.IOU_N, rule="winding")["count_union"] == other["count_union"]
    # nothing inside: an open triangle against itself
    tv, tf = R.TRIANGLE
    flat = Mesh(_dev(tv), _dev(tf))
    empty = flat.iou(flat, n_samples=64)
    assert empty["iou"] == 0.0 and empty["union"] == 0.0 and empty["count_union"] == 0


# ------------------------------------------------------------------ arguments


def test_arguments(K, MM, Mesh):
    v, f = R.mesh("soup60")
    vd, fd, qd = _dev(v), _dev(f), _dev(R.queries("soup60")[:65])
    mesh = Mesh(vd, fd)
    grid = K.mesh_face_grid(vd, fd)

    def changed(row, col, value):
        bad = qd.clone()
        bad[row, col] = value
        return bad

    wide = torch.zeros((65, 6), dtype=torch.float32, device=DEV)
    for bad in (qd.cpu(), qd.double(), wide[:, ::2], qd.reshape(-1), qd[:, :2].contiguous(), changed(5, 2, float("inf")),
                changed(9, 0, float("nan"))):
        for call in (lambda: MM.points_in_mesh(bad, mesh), lambda: mesh.contains(bad, grid=grid),
                     lambda: K.mesh_point_crossings(bad, vd, fd, grid), lambda: MM.signed_distance_to_mesh(bad, mesh),
                     lambda: mesh.signed_distance(bad, grid=grid)):
            with pytest.raises(ValueError):
                call()
    nan_v = vd.clone()
    nan_v[3, 1] = float("nan")
    inf_v = vd.clone()
    inf_v[4, 0] = float("inf")
    for bad in (Mesh(vd.cpu(), fd.cpu()), Mesh(vd.double(), fd), Mesh(vd, fd.long()), Mesh(nan_v, fd), Mesh(inf_v, fd),
                Mesh(vd[:20].contiguous(), fd)):  # the last: indices out of range
        for call in (lambda: bad.contains(qd), lambda: bad.signed_distance(qd),
                     lambda: K.mesh_point_crossings(qd, bad.vertices, bad.faces, grid),
                     lambda: bad.iou(mesh, n_samples=16), lambda: mesh.iou(bad, n_samples=16)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        Mesh(vd[:20].contiguous(), fd).volume()
    for bad_cell in (0.0, -1.0, float("nan"), float("inf"), 1e-4, "x"):  # 1e-4: about 20000 cells along an axis
        for call in (lambda: mesh.contains(qd, cell_size=bad_cell), lambda: mesh.signed_distance(qd, cell_size=bad_cell),
                     lambda: mesh.iou(mesh, n_samples=16, cell_size=bad_cell)):
            with pytest.raises(ValueError):
                call()
    for bad_grid in ({"keys": None}, K.points_grid(vd), {**grid, "F": 59}, {**grid, "keys": grid["keys"][:-1]},
                     {**grid, "keys": grid["keys"].cpu()}, {**grid, "keys": grid["keys"].to(torch.int32)}):
        for call in (lambda: mesh.contains(qd, grid=bad_grid), lambda: mesh.signed_distance(qd, grid=bad_grid),
                     lambda: K.mesh_point_crossings(qd, vd, fd, bad_grid)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        K.mesh_point_crossings(qd, vd, fd, None)
    for rule in ("even-odd", None, 1):
        for call in (lambda: mesh.contains(qd, rule=rule), lambda: MM.points_in_mesh(qd, mesh, rule=rule, grid=grid),
                     lambda: mesh.signed_distance(qd, rule=rule), lambda: mesh.iou(mesh, n_samples=16, rule=rule)):
            with pytest.raises(ValueError, match="rule"):
                call()
    none = Mesh(vd, torch.empty((0, 3), dtype=torch.int32, device=DEV))
    for call in (lambda: mesh.iou(none, n_samples=16), lambda: none.iou(mesh, n_samples=16),
                 lambda: MM.volume_iou(none, none, n_samples=16)):
        with pytest.raises(ValueError, match="faces"):
            call()
    for kwargs in (dict(n_samples=0), dict(n_samples=-4), dict(n_samples=2.5), dict(n_samples=2 ** 31),
                   dict(n_samples=16, seed=-1), dict(n_samples=16, seed=2 ** 64)):
        with pytest.raises(ValueError):
            mesh.iou(mesh, **kwargs)
    with pytest.raises(ValueError):
        mesh.iou((vd, fd), n_samples=16)
