"""Dual contouring's yardsticks on the numpy reference alone (tests/mesh_dual_reference.py), without a GPU: known
answers as properties (closedness, Euler characteristic, face counts, the bits of the Hermite points, a plane, a cube
and an oblique wedge with exact Hermite data), the three deliberately broken variants that each must fail one of them,
and the argument checks of mesh.extract_mesh that run before any device use.

Measured on the reference (14 x 13 x 12 lattice, box (-1,-0.8,-0.6)..(1,0.9,0.7), spacings 0.154 / 0.142 / 0.118):
  cube, exact Hermite data, "qef": 0 fallbacks of 242 cells; max surface distance 1.32e-8, max distance from a true
    corner to its nearest vertex 1.56e-8; "mean": 5.9e-2 and 1.13e-1 (0.73 of a cell);
  wedge, exact Hermite data, "qef": max |field| over the 330 solved vertices 3.10e-8 (5.9e-3 without the spacing in the
    local normal);
  plane: max residual of the Hermite points 8.56e-8, of the vertices 8.80e-8, both placements.
The bounds below are 4 x these values, as the issue sets for the cube; the plane's bound is taken from the residual of
the reference's own Hermite points at run time (a vertex is a combination of them, rounded once more to fp32)."""
import numpy as np
import pytest

import mesh_dual_reference as D
import mesh_reference as M

UNIT_LO, UNIT_HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
CUBE_SURFACE_BOUND, CUBE_CORNER_BOUND, WEDGE_BOUND = D.CUBE_SURFACE_BOUND, D.CUBE_CORNER_BOUND, D.WEDGE_BOUND
PLACEMENTS = ["qef", "mean"]


def sphere_ok(r):
    return (r["V"] > 0 and M.is_closed(r["faces"]) and M.euler_characteristic(r["V"], r["faces"]) == 2
            and M.signed_volume(r["verts"], r["faces"]) > 0)


def face_count_ok(field, r):
    return r["F"] == len(r["faces"]) == 2 * D.count_interior_crossings(field, 0.0) == 2 * r["interior"]


def plane_residual(x):
    return np.abs(np.asarray(x, np.float64) @ np.array(D.PLANE_N) - D.PLANE_D)


def wedge_ok(r):
    solved = r["fallback"] == 0
    worst = np.abs(D.planes_value(D.WEDGE, r["verts"][solved])).max()
    print(f"wedge: {int(solved.sum())} solved of {r['V']}, max |field| {worst:.3g}")
    return solved.sum() > 300 and worst <= WEDGE_BOUND


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_sphere_closed_oriented(placement):
    _, r = D.case("sphere", placement)
    assert r["F"] == 488
    assert sphere_ok(r)
    h = M.spacing(D.SHAPE, UNIT_LO, UNIT_HI).astype(np.float64)
    radius = np.linalg.norm(r["verts"].astype(np.float64), axis=1)
    assert np.abs(radius - 0.6).max() < h.max()
    n = r["vertex_normals"].astype(np.float64)
    assert (np.einsum("ij,ij->i", n, r["verts"].astype(np.float64)) > 0).all()  # outwards: towards lower values


def test_face_counts():
    f, r = D.case("sphere")
    assert face_count_ok(f, r)
    tets = M.marching_tets(f, 0.0, UNIT_LO, UNIT_HI)[1]
    assert r["F"] < len(tets)
    for name in ("plane", "cube"):  # the plane leaves the box: crossing edges on the border give no quad
        f, r = D.case(name)
        assert r["E"] > r["interior"] or name == "cube"
        assert face_count_ok(f, r)
    f = M.noise_field((6, 5, 7), 3)
    assert face_count_ok(f, D.dual_contour(f, 0.0, D.BOX_LO, D.BOX_HI))


@pytest.mark.parametrize("kind", ["sphere", "noise", "integers"])
def test_hermite_points_are_the_tets_vertices(kind):
    if kind == "sphere":
        f, lo, hi = D.case("sphere")[0], UNIT_LO, UNIT_HI
    else:
        f = M.noise_field((6, 5, 7), 3) if kind == "noise" else M.integer_field((6, 5, 7), 4)
        lo, hi = D.BOX_LO, D.BOX_HI
    H = D.hermite(f, 0.0, lo, hi)
    want = D.tets_axis_vertices(f, 0.0, lo, hi)
    assert len(want) == len(H["points"]) > 0
    assert np.array_equal(H["points"].view(np.uint32), want.view(np.uint32))
    assert (np.diff(H["keys"]) > 0).all()


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_plane_stays_on_plane(placement):
    _, r = D.case("plane", placement)
    bound = 4 * plane_residual(r["points"]).max()
    worst = plane_residual(r["verts"]).max()
    print(f"plane {placement}: vertices {worst:.3g}, Hermite points {bound / 4:.3g}")
    assert r["V"] > 0 and worst <= bound
    assert int(r["fallback"].sum()) == 0


def test_cube_corners():
    _, r = D.case("cube", "qef")
    surface, corner = D.cube_surface_distance(r["verts"]).max(), D.cube_corner_distance(r["verts"]).max()
    print(f"cube qef: surface {surface:.3g}, corners {corner:.3g}, fallbacks {int(r['fallback'].sum())} of {r['V']}")
    assert int(r["fallback"].sum()) == 0
    assert surface <= CUBE_SURFACE_BOUND and corner <= CUBE_CORNER_BOUND
    assert sphere_ok(r)  # closed, oriented, Euler characteristic 2
    _, m = D.case("cube", "mean")
    cell = M.spacing(D.SHAPE, D.BOX_LO, D.BOX_HI).min()
    assert D.cube_corner_distance(m["verts"]).min() > 0.1 * cell


def test_wedge_crease():
    assert wedge_ok(D.case("wedge", "qef")[1])


def test_vertices_stay_in_their_cells():
    for name in ("sphere", "cube", "wedge"):
        for placement in PLACEMENTS:
            f, r = D.case(name, placement)
            lo, hi = (UNIT_LO, UNIT_HI) if name == "sphere" else (D.BOX_LO, D.BOX_HI)
            h = M.spacing(D.SHAPE, lo, hi)
            a = np.asarray(lo, np.float32) + r["cells"].astype(np.float32) * h
            slack = 4e-7 * (np.abs(a) + np.abs(a + h) + h)
            assert ((r["verts"] >= a - slack) & (r["verts"] <= a + h + slack)).all()


def test_teeth():
    """Each broken variant fails a check that the rule passes."""
    assert not sphere_ok(D.case("sphere", "qef", "reversed")[1])  # the volume turns negative
    f, r = D.case("plane", "qef", "no_boundary")
    assert not face_count_ok(f, r)
    assert not wedge_ok(D.case("wedge", "qef", "no_h")[1])


def test_extract_mesh_argument_checks():
    """method / placement are checked before the density function or the device is touched."""
    from nerf_amd import mesh

    def never(x):
        raise AssertionError("the density function must not be called")

    with pytest.raises(ValueError, match="method"):
        mesh.extract_mesh(never, UNIT_LO, UNIT_HI, 8, 0.0, method="bogus")
    with pytest.raises(ValueError, match="placement"):
        mesh.extract_mesh(never, UNIT_LO, UNIT_HI, 8, 0.0, method="dual", placement="bogus")
    with pytest.raises(ValueError, match="tol"):
        mesh.extract_mesh(never, UNIT_LO, UNIT_HI, 8, 0.0, method="dual", tol=1.5)
    with pytest.raises(ValueError, match="refine"):
        mesh.extract_mesh(never, UNIT_LO, UNIT_HI, 8, 0.0, method="dual", refine=-1)
    with pytest.raises(ValueError, match="hermite"):
        mesh.extract_mesh(never, UNIT_LO, UNIT_HI, 8, 0.0, method="dual", hermite="field")
