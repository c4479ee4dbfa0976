"""kernels.mesh_winding_bricks / mesh_winding_number (csrc/mesh_winding.hip), mesh_metrics.winding_number and
rule="generalized" of points_in_mesh / signed_distance_to_mesh / volume_iou and of Mesh.contains / signed_distance /
iou on the device (-m gpu), against the restatement of the contract in tests/mesh_winding_reference.py (DESIGN
§3.11.10).

The moments of the bricks are the reference's bit for bit; w is within (F + B) 2^-50 of it, which leaves about a
dozen ulps of 2 pi per term for the device's atan2, every other operation being the same IEEE operation on both
sides.  Every mesh with a reference has at most 1224 faces and every query set at most 2528 queries (the TSDF mesh
of the last test has 4526 faces and 4096 samples); every reference is computed once per process."""
import numpy as np
import pytest
import torch

import mesh_inside_reference as R
import mesh_winding_reference as W
import tsdf_reference as T

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAMES = tuple(W.MESHES)
BRICKS = ("one", "default", "fine")
MODES = ((1.0, False), (3.0, False), (3.0, True))  # (beta, exact)


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


def _k(name, which):
    return {"one": 1, "default": None, "fine": W.fine_bricks_per_axis(name)}[which]


def _close(got, ref, tol, what):
    assert got.dtype == torch.float64 and tuple(got.shape) == tuple(ref.shape)
    err = float(np.abs(got.cpu().numpy() - ref).max()) if len(ref) else 0.0
    print(f"{what}: max |w - reference| = {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol, what


# ------------------------------------------------------------------ the bricks


@pytest.mark.parametrize("which", BRICKS)
@pytest.mark.parametrize("name", NAMES)
def test_bricks_equal_the_reference_bitwise(K, name, which):
    v, f = W.mesh(name)
    ref = W.bricks_of(name, which)
    got = K.mesh_winding_bricks(_dev(v), _dev(f), _k(name, which))
    assert (got["B"], got["F"], got["dims"]) == (ref["B"], ref["F"], ref["dims"])
    assert got["lo"] == ref["lo"].tolist() and got["cell"] == float(ref["cell"]) and got["inv"] == float(ref["inv"])
    for key, dtype in (("keys", torch.int64), ("runs", torch.int32), ("moments", torch.float64), ("soup", torch.float32)):
        assert got[key].dtype == dtype and tuple(got[key].shape) == ref[key].shape, key
        assert got[key].cpu().numpy().tobytes() == ref[key].tobytes(), key  # the moments too: bit for bit
    again = K.mesh_winding_bricks(_dev(v), _dev(f), _k(name, which))
    assert all(torch.equal(got[key], again[key]) for key in ("keys", "runs", "moments", "soup"))


def test_default_bricks_per_axis(K):
    v, f = W.mesh("sphere12")
    got = K.mesh_winding_bricks(_dev(v), _dev(f))
    assert max(got["dims"]) == W.default_bricks_per_axis(len(f)) == 8


# ------------------------------------------------------------------ the kernel against the reference


@pytest.mark.parametrize("which", BRICKS)
@pytest.mark.parametrize("name", NAMES)
def test_winding_number_against_the_reference(K, name, which):
    v, f = W.mesh(name)
    vd, fd = _dev(v), _dev(f)
    q = W.queries(name)
    qd = _dev(q)
    br = K.mesh_winding_bricks(vd, fd, _k(name, which))
    tol = W.tolerance(W.bricks_of(name, which))
    for beta, exact in MODES:
        ref = W.winding_of(name, which, beta, exact)
        got = K.mesh_winding_number(qd, vd, fd, br, beta=beta, exact=exact)
        _close(got, ref, tol, f"{name} {which} beta {beta} exact {exact}")
        assert torch.equal(got, K.mesh_winding_number(qd, vd, fd, br, beta=beta, exact=exact))  # the same call twice
        assert torch.equal(got, K.mesh_winding_number(qd, vd, fd, br, beta=beta, exact=exact, sort_queries=False))


@pytest.mark.parametrize("name", ("sphere12", "cut_sphere"))
def test_query_counts_and_split_calls(K, name):
    """the wave and block edges, and a query set split into two calls: a query's w does not depend on its neighbours"""
    v, f = W.mesh(name)
    vd, fd = _dev(v), _dev(f)
    qd = _dev(W.queries(name))
    br = K.mesh_winding_bricks(vd, fd)
    tol = W.tolerance(W.bricks_of(name, "default"))
    for beta, exact in ((3.0, False), (3.0, True)):
        ref = W.winding_of(name, "default", beta, exact)
        whole = K.mesh_winding_number(qd, vd, fd, br, beta=beta, exact=exact)
        for n in (0, 1, 63, 64, 65, 255, 257):
            for sort_queries in (True, False):
                part = K.mesh_winding_number(qd[:n].contiguous(), vd, fd, br, beta=beta, exact=exact,
                                             sort_queries=sort_queries)
                assert torch.equal(part, whole[:n]), (n, sort_queries)
            _close(part, ref[:n], tol, f"{name} n = {n}")
        for cut in (1, 300, 1999):
            two = torch.cat([K.mesh_winding_number(part.contiguous(), vd, fd, br, beta=beta, exact=exact)
                             for part in (qd[:cut], qd[cut:])])
            assert torch.equal(two, whole), cut


def test_no_faces_and_no_queries(K, MM, Mesh):
    v, f = W.mesh("soup60")
    q = _dev(W.queries("soup60")[:70])
    none = Mesh(_dev(v), torch.empty((0, 3), dtype=torch.int32, device=DEV))
    br = K.mesh_winding_bricks(none.vertices, none.faces)
    assert br["B"] == 0 and br["F"] == 0 and br["dims"] == [1, 1, 1]
    assert [tuple(br[k].shape) for k in ("keys", "runs", "moments", "soup")] == [(0,), (0, 2), (0, 7), (0, 9)]
    for w in (K.mesh_winding_number(q, none.vertices, none.faces, br), none.winding_number(q),
              MM.winding_number(q, none, exact=True)):
        assert w.dtype == torch.float64 and tuple(w.shape) == (70,) and not bool(w.any())
    assert not bool(none.contains(q, rule="generalized").any())
    sd, face, closest = none.signed_distance(q, rule="generalized")
    assert bool((sd == float("inf")).all()) and bool((face == -1).all()) and torch.equal(closest, q)
    mesh = Mesh(_dev(v), _dev(f))
    empty = torch.empty((0, 3), dtype=torch.float32, device=DEV)
    assert tuple(mesh.winding_number(empty).shape) == (0,) and mesh.winding_number(empty).dtype == torch.float64
    assert tuple(mesh.contains(empty, rule="generalized").shape) == (0,)


# ------------------------------------------------------------------ rule="generalized"


def _decided(ref, tol):
    """the queries whose side the reference alone decides: all but 1 % at the most"""
    clear = np.abs(ref - 0.5) > tol
    assert clear.mean() >= 0.99
    return clear


@pytest.mark.parametrize("name", ("sphere12", "hemisphere", "cut_sphere", "soup60"))
def test_generalized_rule_on_every_entry_point(K, MM, Mesh, name):
    v, f = W.mesh(name)
    mesh = Mesh(_dev(v), _dev(f))
    qd = _dev(W.queries(name))
    tol = W.tolerance(W.bricks_of(name, "default"))
    br = K.mesh_winding_bricks(mesh.vertices, mesh.faces)
    d2, face, closest = mesh.closest_points(qd)
    for beta, exact in ((3.0, False), (3.0, True), (1.0, False)):
        ref = W.winding_of(name, "default", beta, exact)
        clear, want = _decided(ref, tol), ref > 0.5
        kw = dict(rule="generalized", beta=beta, exact=exact)
        w = MM.winding_number(qd, mesh, beta=beta, exact=exact)
        _close(w, ref, tol, f"{name} winding_number beta {beta} exact {exact}")
        assert torch.equal(w, mesh.winding_number(qd, beta=beta, exact=exact, bricks=br))
        inside = MM.points_in_mesh(qd, mesh, **kw)
        assert inside.dtype == torch.bool and np.array_equal(inside.cpu().numpy()[clear], want[clear])
        assert torch.equal(inside, w > 0.5)
        assert torch.equal(inside, mesh.contains(qd, **kw)) and torch.equal(inside, mesh.contains(qd, bricks=br, **kw))
        for grid in (None, K.mesh_face_grid(mesh.vertices, mesh.faces)):
            sd, sface, sclosest = MM.signed_distance_to_mesh(qd, mesh, grid=grid, bricks=br, **kw)
            assert torch.equal(sface, face) and torch.equal(sclosest, closest)
            assert torch.equal(sd < 0, inside & (d2 > 0)) and torch.equal(sd.abs(), torch.sqrt(d2))
            assert all(torch.equal(a, b) for a, b in zip(mesh.signed_distance(qd, grid=grid, **kw), (sd, sface, sclosest)))
    # the two old rules and the default are what they were
    if name in R.MESHES:
        c, wn = R.brute_of(name)
        assert np.array_equal(mesh.contains(qd).cpu().numpy(), (c & 1).astype(bool))
        assert np.array_equal(mesh.contains(qd, rule="winding").cpu().numpy(), wn != 0)
    import nerf_amd
    assert nerf_amd.winding_number is MM.winding_number and "winding_number" in nerf_amd.__all__


@pytest.mark.parametrize("name", ("sphere12",))
def test_closed_mesh_generalized_equals_parity(K, MM, Mesh, name):
    """on a closed mesh wound outwards w is the crossing-count winding (the same sign), so off the surface the
    generalized rule, the parity rule and the winding rule agree, exactly and with the far field"""
    v, f = W.mesh(name)
    mesh = Mesh(_dev(v), _dev(f))
    qd = _dev(W.queries(name))
    d2, _, _ = mesh.closest_points(qd)
    off = d2 > 1e-6  # farther than 0.001 from every face
    assert float(off.double().mean()) > 0.99
    parity = mesh.contains(qd)
    c, wn = R.brute_of(name)
    w = mesh.winding_number(qd, exact=True)
    assert float((w - _dev(wn.astype(np.float64)))[off].abs().max()) <= len(f) * 2.0 ** -50
    for kw in (dict(exact=True), dict(beta=3.0), dict(beta=2.0)):
        assert torch.equal(mesh.contains(qd, rule="generalized", **kw)[off], parity[off]), kw
    assert mesh.volume() > 0


def test_open_hemisphere_is_classified_as_a_person_would(K, MM, Mesh):
    """why the feature exists: an open dome.  Points deep under it count as inside and points far away as outside by
    the generalised winding number; parity finds 'inside' by the accident of a ray's direction alone, and so calls
    the whole column under the dome inside, however far below the rim plane."""
    v, f = W.hemisphere()
    mesh = Mesh(_dev(v), _dev(f))
    rng = np.random.default_rng(5)
    d = rng.normal(size=(256, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:, 2] = np.abs(d[:, 2])
    deep = (d * rng.uniform(0.05, 0.6, (256, 1)) + [0, 0, 0.1]).astype(np.float32)  # under the dome, above the rim
    below = deep * np.array([1, 1, -1], np.float32)  # their mirror images: under the rim plane, outside the dome
    far = (d * rng.uniform(2.0, 10.0, (256, 1)) * rng.choice([-1.0, 1.0], (256, 1))).astype(np.float32)
    for beta, exact in ((3.0, False), (3.0, True)):
        kw = dict(rule="generalized", beta=beta, exact=exact)
        w_deep = mesh.winding_number(_dev(deep), beta=beta, exact=exact)
        print(f"deep: w in [{float(w_deep.min()):.3f}, {float(w_deep.max()):.3f}]")
        assert bool(mesh.contains(_dev(deep), **kw).all()) and float(w_deep.min()) > 0.5
        assert not bool(mesh.contains(_dev(far), **kw).any())
        assert not bool(mesh.contains(_dev(below), **kw).any())
        sd = mesh.signed_distance(_dev(deep), **kw)[0]
        assert bool((sd < 0).all()) and bool((mesh.signed_distance(_dev(far), **kw)[0] > 0).all())
    # parity answers the same for deep points (one crossing above them) but it is the ray, not the solid, that says
    # so: a point below the rim plane, straight under the dome, is 'inside' by parity as well
    assert bool(mesh.contains(_dev(deep)).all())
    under = np.array([[0.1, 0.2, -3.0], [-0.3, 0.1, -50.0]], np.float32)
    assert bool(mesh.contains(_dev(under)).all()) and not bool(mesh.contains(_dev(under), rule="generalized").any())
    # and the volume of the dome by Monte Carlo: parity counts the whole column under it, the winding number about
    # the half ball (the region with w > 0.5 ends near the rim plane)
    got = mesh.iou(mesh, n_samples=4096, rule="generalized")
    by_parity = mesh.iou(mesh, n_samples=4096)
    half_ball = 2.0 / 3.0 * np.pi
    print(f"dome volume: generalized {got['volume_a']:.3f}, parity {by_parity['volume_a']:.3f}, half ball {half_ball:.3f}")
    assert got["iou"] == 1.0 and abs(got["volume_a"] - half_ball) < 0.15 * half_ball
    assert by_parity["volume_a"] > 1.3 * half_ball


def test_volume_iou_generalized(K, MM, Mesh):
    v, f = R.sphere()
    sv, _ = R.shifted_sphere()
    a, b = Mesh(_dev(v), _dev(f)), Mesh(_dev(sv), _dev(f))
    by_parity = a.iou(b, n_samples=R.IOU_N, seed=R.IOU_SEED)
    assert by_parity == R.iou_reference("shifted")  # the default is what it was
    for kw in (dict(exact=True), dict()):
        got = MM.volume_iou(a, b, n_samples=R.IOU_N, seed=R.IOU_SEED, rule="generalized", **kw)
        assert got == a.iou(b, n_samples=R.IOU_N, seed=R.IOU_SEED, rule="generalized", **kw)  # equal dicts
        assert got["box"] == by_parity["box"] and got["n_samples"] == R.IOU_N
        # closed meshes: the same points are inside, but for the few within the far field's error of the surface
        for key in ("count_a", "count_b", "count_intersection", "count_union"):
            assert abs(got[key] - by_parity[key]) <= (0 if kw else 0.01 * R.IOU_N), (key, kw)
    bricks = (K.mesh_winding_bricks(a.vertices, a.faces), K.mesh_winding_bricks(b.vertices, b.faces))
    assert got == a.iou(b, n_samples=R.IOU_N, seed=R.IOU_SEED, rule="generalized", bricks=bricks)


def test_tsdf_mesh_is_open_and_has_an_iou(K, Mesh):
    """a 32^3 volume fused from three views of the sphere, all from x > 0: the far side is never seen, the mesh is
    open, and rule="generalized" still gives it a volume: iou 1.0 against itself and equal dicts on two calls"""
    import mesh_reference as MR
    from nerf_amd import TSDFVolume
    case = T.sphere_case()
    views = [0, 6, 7]  # +x and two of the diagonals with x > 0
    vol = TSDFVolume(T.SPHERE_LO, T.SPHERE_HI, 32)
    vol.integrate(_dev(case["depth"][views]), *case["k"], _dev(case["c2w"][views]))
    mesh = vol.extract_mesh(normals=None)
    F = int(mesh.faces.shape[0])
    assert F > 100 and not MR.is_closed(mesh.faces.cpu().numpy())
    one = mesh.iou(mesh, rule="generalized", n_samples=4096)
    two = mesh.iou(mesh, rule="generalized", n_samples=4096)
    print(f"tsdf mesh: {F} faces, count inside {one['count_a']} of 4096, volume {one['volume_a']:.4f}")
    assert one == two and one["iou"] == 1.0 and one["count_a"] == one["count_union"] > 0


# ------------------------------------------------------------------ arguments


def test_arguments(K, MM, Mesh):
    v, f = W.mesh("soup60")
    vd, fd, qd = _dev(v), _dev(f), _dev(W.queries("soup60")[:65])
    mesh = Mesh(vd, fd)
    br = K.mesh_winding_bricks(vd, fd)
    grid = K.mesh_face_grid(vd, fd)
    real = K.lib().nerf_mesh_winding

    def changed(row, col, value):
        bad = qd.clone()
        bad[row, col] = value
        return bad

    gen = dict(rule="generalized")
    wide = torch.zeros((65, 6), dtype=torch.float32, device=DEV)
    for bad in (qd.cpu(), qd.double(), wide[:, ::2], qd.reshape(-1), qd[:, :2].contiguous(), changed(5, 2, float("inf")),
                changed(9, 0, float("nan"))):
        for call in (lambda: K.mesh_winding_number(bad, vd, fd, br), lambda: MM.winding_number(bad, mesh),
                     lambda: mesh.winding_number(bad, bricks=br), lambda: mesh.contains(bad, **gen),
                     lambda: mesh.contains(bad, bricks=br, **gen), lambda: mesh.signed_distance(bad, **gen),
                     lambda: mesh.signed_distance(bad, grid=grid, bricks=br, **gen)):
            with pytest.raises(ValueError):
                call()
    for beta in (0.5, 0.0, -3.0, float("nan"), float("inf"), "3", None, True):
        for call in (lambda: K.mesh_winding_number(qd, vd, fd, br, beta=beta), lambda: mesh.winding_number(qd, beta=beta),
                     lambda: mesh.contains(qd, beta=beta, **gen), lambda: mesh.signed_distance(qd, beta=beta, **gen),
                     lambda: mesh.iou(mesh, n_samples=16, beta=beta, **gen)):
            with pytest.raises(ValueError, match="beta"):
                call()
    other = K.mesh_winding_bricks(vd, fd[:59].contiguous())
    for bad_bricks in ({"keys": None}, grid, K.points_grid(vd), other, {**br, "F": 59}, {**br, "B": br["B"] + 1},
                       {**br, "soup": br["soup"][:-1]}, {**br, "moments": br["moments"].float()},
                       {**br, "runs": br["runs"].cpu()}, {**br, "keys": br["keys"].to(torch.int32)}, None):
        calls = [lambda: K.mesh_winding_number(qd, vd, fd, bad_bricks)]
        if bad_bricks is not None:  # None means "build them here" one level up
            calls += [lambda: mesh.winding_number(qd, bricks=bad_bricks), lambda: mesh.contains(qd, bricks=bad_bricks, **gen),
                      lambda: mesh.signed_distance(qd, bricks=bad_bricks, **gen),
                      lambda: mesh.iou(mesh, n_samples=16, bricks=(br, bad_bricks), **gen)]
        for call in calls:
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        mesh.iou(mesh, n_samples=16, bricks=br, **gen)  # a pair is wanted
    with pytest.raises(ValueError, match="grid"):
        mesh.contains(qd, grid=grid, **gen)  # this rule does not use the face grid
    for kw in (dict(beta=2.0), dict(exact=True), dict(bricks=br)):  # they go with the generalized rule alone
        for call in (lambda: mesh.contains(qd, **kw), lambda: mesh.signed_distance(qd, rule="winding", **kw)):
            with pytest.raises(ValueError):
                call()
    nan_v = vd.clone()
    nan_v[3, 1] = float("nan")
    for bad in (Mesh(vd.cpu(), fd.cpu()), Mesh(vd.double(), fd), Mesh(vd, fd.long()), Mesh(nan_v, fd),
                Mesh(vd[:20].contiguous(), fd)):  # the last: indices out of range
        for call in (lambda: K.mesh_winding_bricks(bad.vertices, bad.faces), lambda: bad.winding_number(qd),
                     lambda: bad.contains(qd, **gen), lambda: K.mesh_winding_number(qd, bad.vertices, bad.faces, br),
                     lambda: bad.iou(mesh, n_samples=16, **gen), lambda: mesh.iou(bad, n_samples=16, **gen)):
            with pytest.raises(ValueError):
                call()
    for k in (0, -1, 1025, 2.0, "8", True):
        with pytest.raises(ValueError, match="bricks_per_axis"):
            K.mesh_winding_bricks(vd, fd, k)
    for rule in ("generalised", "gwn", None):
        with pytest.raises(ValueError, match="rule"):
            mesh.contains(qd, rule=rule)
    # the C entry point refuses what the wrapper refuses
    w = torch.empty(65, dtype=torch.float64, device=DEV)
    for beta, exact, B in ((0.5, 0, br["B"]), (float("nan"), 0, br["B"]), (3.0, 2, br["B"]), (3.0, 0, 0), (3.0, 0, 61)):
        status = real(K.ptr(qd), 65, K.ptr(br["runs"]), K.ptr(br["moments"]), B, K.ptr(br["soup"]), 60, beta, exact,
                      K.ptr(w), K.stream())
        assert status == -1, (beta, exact, B)
