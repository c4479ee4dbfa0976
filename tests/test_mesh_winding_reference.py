"""The numpy restatement of the generalised winding number (tests/mesh_winding_reference.py) against
what the solid angle must give: known values, the rim theorem for an open sheet, the crossing-count winding of
closed meshes, and the far-field error table.  No GPU: the device is compared with this reference in
tests/test_gpu_mesh_winding.py."""
import numpy as np
import pytest

import mesh_distance_reference as D
import mesh_inside_reference as R
import mesh_winding_reference as W

F32 = np.float32


def test_one_triangle_from_the_origin():
    """(1,0,0), (0,1,0), (0,0,1) fill one octant: an eighth of the sphere, positive seen from the side the normal points
    away from"""
    v = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], F32)
    origin = np.zeros((1, 3), F32)
    for faces, sign in (([[0, 1, 2]], 1.0), ([[0, 2, 1]], -1.0)):
        w = W.plain(v, faces, origin)[0]
        assert abs(w - sign * 0.125) <= 2.0 ** -50
        for k in (1, None, 4):
            br = W.bricks(v, faces, k)
            assert br["B"] == 1 and br["runs"].tolist() == [[0, 1]]
            assert W.winding(origin, br, exact=True)[0] == w and W.winding(origin, br, beta=1.0)[0] == w  # r2 > d2: near


def test_open_hemisphere_from_the_centre_of_its_rim():
    """the solid angle of an open sheet depends on its rim alone: the rim is a polygon in z = 0 around the origin, so
    the sheet fills half the sphere whatever its shape"""
    v, f = W.hemisphere()
    origin = np.zeros((1, 3), F32)
    w = W.plain(v, f, origin)[0]
    print(f"hemisphere from the origin: w - 0.5 = {w - 0.5:.3e}, bound {len(f) * 2.0 ** -50:.3e}")
    assert abs(w - 0.5) <= len(f) * 2.0 ** -50
    for which in ("one", "default", "fine"):
        assert abs(W.winding(origin, W.bricks_of("hemisphere", which), exact=True)[0] - 0.5) <= len(f) * 2.0 ** -50
    flipped = np.ascontiguousarray(f[:, ::-1])
    assert abs(W.plain(v, flipped, origin)[0] + 0.5) <= len(f) * 2.0 ** -50


@pytest.mark.parametrize("name", ("sphere12", "spheres"))
def test_closed_meshes_equal_the_crossing_count_winding(name):
    """w = + the winding of mesh_inside_reference (the same sign: +1 inside a mesh of positive volume), within
    F 2^-50, for the queries off the surface"""
    v, f = R.mesh(name)
    q = R.queries(name)
    d2, _, _ = D.nearest_faces(v, f, q)
    off = d2 > 1e-6  # farther than 1e-3 from every face
    assert off.sum() >= 0.99 * len(q) and R.volume(v, f) > 0
    _, winding = R.brute_of(name)
    assert set(np.unique(winding[off])) == {0, 1}
    w = W.plain(v, f, q)
    err = np.abs(w - winding)[off].max()
    print(f"{name}: {off.sum()} of {len(q)} queries off the surface, max |w - winding| = {err:.3e}, "
          f"bound {len(f) * 2.0 ** -50:.3e}")
    assert err <= len(f) * 2.0 ** -50
    br = W.bricks(v, f)
    assert np.abs(W.winding(q, br, exact=True) - winding)[off].max() <= len(f) * 2.0 ** -50
    assert np.array_equal((w > 0.5)[off], R.inside(v, f, q)[off])


@pytest.mark.parametrize("name", W.OPEN)
def test_error_table(name):
    """max and mean |w_beta - w_exact| over 400 box queries on the default bricks: it falls as beta grows, and stays
    within twice what this reference gave when DESIGN §3.11.10's table was written"""
    errors, work = W.error_table(name)
    br = W.bricks_of(name, "default")
    print(f"{name}: F = {br['F']}, B = {br['B']}, dims {br['dims']}")
    for beta, (emax, emean), (far, near) in zip(W.ERROR_BETAS, errors, work):
        print(f"  beta {beta}: max {emax:.4e} mean {emean:.4e}, far bricks {far:.1f}, exact faces {near:.1f} per query")
    for (emax, emean), (tmax, tmean) in zip(errors, W.ERROR_TABLE[name]):
        assert 0 < emax <= 2 * tmax and 0 < emean <= 2 * tmean
    for k in range(len(errors) - 1):
        assert errors[k + 1][0] < errors[k][0] and errors[k + 1][1] < errors[k][1]
        assert work[k + 1][0] < work[k][0] and work[k + 1][1] > work[k][1]  # fewer far bricks, more exact faces
    # the reference alone decides all but 1 % of the queries: none lies within the device tolerance of one half
    exact = W.winding(W.box_queries(), br, exact=True)
    assert (np.abs(exact - 0.5) <= W.tolerance(br)).mean() <= 0.01


@pytest.mark.parametrize("name", tuple(W.MESHES))
def test_bricks_partition_the_faces(name):
    v, f = W.mesh(name)
    for which in ("one", "default", "fine"):
        br = W.bricks_of(name, which)
        runs, keys = br["runs"], br["keys"]
        assert sorted((keys & 0xffffffff).tolist()) == list(range(len(f)))  # every face once
        assert runs[0, 0] == 0 and runs[-1, 1] == len(f) and (runs[1:, 0] == runs[:-1, 1]).all()
        assert (runs[:, 1] > runs[:, 0]).all() and br["B"] == len(np.unique(keys >> 32))
        assert br["B"] == 1 if which == "one" else br["B"] >= 1
        assert max(br["dims"]) <= (1 if which == "one" else W.MAX_DIM)
        if which == "fine" and name not in ("one_face", "tiny_face"):
            assert (runs[:, 1] - runs[:, 0] == 1).mean() > 0.5  # most bricks hold one face
        # the dipole of a brick is the sum of its faces' area vectors, p lies in the box of its corners
        corners = br["soup"].reshape(-1, 3, 3).astype(np.float64)
        area = 0.5 * np.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0])
        for b, (s, e) in enumerate(runs):
            assert np.allclose(br["moments"][b, 3:6], area[s:e].sum(0), rtol=1e-12, atol=1e-300)
            box = corners[s:e].reshape(-1, 3)
            p = br["moments"][b, :3]
            assert (p >= box.min(0) - 1e-12).all() and (p <= box.max(0) + 1e-12).all()
            assert br["moments"][b, 6] == pytest.approx(((box - p) ** 2).sum(1).max(), rel=1e-12, abs=1e-300)
    # exact through the bricks is the plain sum in sorted-face order
    q = W.queries(name)[:64]
    br = W.bricks_of(name, "default")
    assert np.array_equal(W.winding(q, br, exact=True), W.plain(br["soup"].reshape(-1, 3), np.arange(3 * len(f)), q))


def test_strict_compare_and_a_brick_without_area():
    """a face whose corners coincide is a brick with r2 = 0 and no area: p is the plain mean of the centroids, and a
    query at p is near (0 > 0 is false), where the dipole would divide by zero"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]], F32)
    f = np.array([[0, 1, 2], [3, 3, 3]], np.int32)
    br = W.bricks(v, f, 8)
    assert br["B"] == 2 and br["moments"][1].tolist() == [5, 5, 5, 0, 0, 0, 0]
    q = np.array([[5, 5, 5], [0.25, 0.25, 1], [0.25, 0.25, -1]], F32)
    w, count = W.winding(q, br, beta=1.0, counts=True)
    assert np.isfinite(w).all() and count[0].tolist() == [1, 1] and w[1] < 0 < w[2]
    assert np.allclose(w, W.winding(q, br, exact=True), atol=0.05)


def test_host_side_rules_match_the_package():
    """the default bricks per axis and the brick grid of kernels.py (numpy on the host) against the reference's"""
    from nerf_amd import kernels as K
    for F in (1, 2, 16, 17, 360, 1224, 10 ** 5, 10 ** 6, 3 * 10 ** 6, 2 ** 31 - 1):
        assert K._bricks_per_axis(F) == W.default_bricks_per_axis(F)
    assert W.default_bricks_per_axis(1) == 2 and W.default_bricks_per_axis(10 ** 6) == 40
    assert K._bricks_per_axis(2 ** 40) == 1024
    for name in W.MESHES:
        v, f = W.mesh(name)
        box = np.concatenate([v.min(0), v.max(0)]).astype(F32)
        for k in (1, None, W.fine_bricks_per_axis(name)):
            kk = W.default_bricks_per_axis(len(f)) if k is None else k
            lo, cell, inv, dims = K._grid_from_box(box, len(f), None, "vertices", per_axis=kk)
            ref = W.brick_grid(v, f, k)
            assert lo == ref["lo"].tolist() and cell == float(ref["cell"]) and inv == float(ref["inv"])
            assert dims == ref["dims"] and max(dims) <= kk
