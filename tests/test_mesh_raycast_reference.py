"""The numpy reference of nearest-hit ray casting (tests/mesh_raycast_reference.py), pinned to facts that
do not depend on it: a table of rays on one triangle, the geometry of a closed convex mesh, the equality of its grid walk
with its brute force, and a sliver that shows what the box clause of the hit test is for.  No GPU.

The grid walk is a per-ray Python loop, so it runs on the first few hundred rays of every set (1024 layers per ray at
the cap); the device tests run the full sets against the brute force."""
import numpy as np
import pytest

import mesh_distance_reference as D
import mesh_raycast_reference as R

F32, F64 = np.float32, np.float64


def _same(got, want):
    for g, w, dtype in zip(got, want, (F64, np.int32, F32)):
        assert g.dtype == dtype and g.shape == w.shape
        assert g.tobytes() == w.tobytes()


def test_table_on_one_triangle():
    v, f = R.TRIANGLE
    rays = R.table_rays()
    for ray, (_, cull, want) in zip(rays, R.TABLE):
        for cast in (lambda r: R.ray_cast(v, f, r, cull), lambda r: R.grid_ray_cast(v, f, r, D.face_grid(v, f), cull)):
            t, face, bary = cast(ray[None])
            assert t.dtype == F64 and face.dtype == np.int32 and bary.dtype == F32 and bary.shape == (1, 2)
            if want is None:
                assert t[0] == np.inf and face[0] == -1 and bary[0].tolist() == [0.0, 0.0]
            else:
                assert (t[0], face[0], *bary[0].tolist()) == (want[0], 0, want[1], want[2])
    # the rows named by the issue are in the table
    hits = [want is not None for _, _, want in R.TABLE]
    assert sum(hits) >= 10 and len(hits) - sum(hits) >= 9


def test_no_faces_and_no_rays():
    v, f = R.mesh("soup60")
    t, face, bary = R.ray_cast(v, f[:0], R.rays("soup60")[:7])
    assert (t == np.inf).all() and (face == -1).all() and not bary.any() and bary.shape == (7, 2)
    t, face, bary = R.ray_cast(v, f, R.rays("soup60")[:0])
    assert t.shape == (0,) and face.shape == (0,) and bary.shape == (0, 2)
    _same(R.grid_ray_cast(v, f[:0], R.rays("soup60")[:7], D.face_grid(v, f[:0])), R.ray_cast(v, f[:0], R.rays("soup60")[:7]))


def test_dead_faces_are_never_hit():
    v, f = R.mesh("soup60")
    dead = np.flatnonzero(R.dead_faces(v, f))
    assert dead.tolist() == [0, 5, 17, 30, 41, 59]
    for which in ("rays", "axis", "inside"):
        assert not np.isin(R.brute("soup60", which)[1], dead).any()


def test_closed_convex_mesh():
    v, f = R.octahedron()
    rng = np.random.default_rng(2)
    n = 400
    # interior points: convex combinations of the six vertices with every weight positive
    aim = rng.dirichlet(np.ones(6), n) @ v.astype(F64)
    direction = rng.normal(size=(n, 3))
    o = aim + direction / np.linalg.norm(direction, axis=1, keepdims=True) * rng.uniform(5, 9, (n, 1))
    rays = R.pack(o, aim - o)  # the aim point is at t = 1
    plain, culled = R.ray_cast(v, f, rays), R.ray_cast(v, f, rays, cull=True)
    _same(plain, culled)  # the nearest hit of an outward-wound convex mesh is a front hit
    assert (plain[1] >= 0).all() and (plain[0] > 0).all() and (plain[0] < 1).all()
    assert len(np.unique(plain[1])) == 8
    # the same line from the aim point outwards leaves through a back face: det < 0, culled away
    back = R.pack(aim, o - aim)
    out = R.ray_cast(v, f, back)
    assert (out[1] >= 0).all() and (R.ray_cast(v, f, back, cull=True)[1] == -1).all()
    r = back.astype(F64)
    corners = v[f[out[1]]].astype(F64)
    e1, e2 = corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0]
    assert (R.dot(e1, R.cross(r[:, 3:6], e2)) < 0).all()
    rr = rays.astype(F64)
    p_in = rr[:, 0:3] + plain[0][:, None] * rr[:, 3:6]
    w = np.abs(p_in[:, 0]) + np.abs(p_in[:, 1]) / 1.5 + np.abs(p_in[:, 2]) / 2
    assert np.abs(w - 1).max() < 1e-5  # on |x| + |y| / 1.5 + |z| / 2 = 1 (fp32 rays: 9 units long, 2^-24 relative)


@pytest.mark.parametrize("which", ("one_cell", "default", "cap"))
@pytest.mark.parametrize("name", ("soup60", "tiny_face", "spheres"))
def test_grid_walk_equals_brute_force(name, which):
    v, f = R.mesh(name)
    grid = D.face_grid(v, f, R.grid_cell(name, which))
    if which != "default":
        assert max(grid["dims"]) == (1 if which == "one_cell" else 1024 if name == "tiny_face" else 32)
    sets = {"rays": R.rays(name)[:200], "axis": R.axis_rays(name)[:60], "plane": R.plane_rays(name, grid, 60),
            "inside": R.inside_rays(name)[:50], "outside": R.outside_rays(name)[:30], "far": R.far_rays(name)[:30],
            "second": R.second_hit_rays(name)[:80]}
    for kind, rays in sets.items():
        for cull in (False, True):
            want = R.ray_cast(v, f, rays, cull)
            got = R.grid_ray_cast(v, f, rays, grid, cull, counts=True)
            _same(got[:3], want)
            if kind == "outside":
                assert (want[1] == -1).all()
                if which == "cap":  # the grid's box ends within a cell (0.032 extents) of the vertices' box and the
                    assert (got[3] == 0).all()  # rays pass 0.05 extents outside: clipped away, no layer, no face
    hits = R.brute(name)[1] >= 0
    assert 0.25 <= hits.mean() <= 0.75


def test_second_hit():
    for name in ("soup60", "spheres"):
        first, second = R.brute(name), R.ray_cast(*R.mesh(name), R.second_hit_rays(name))
        was = first[1] >= 0
        assert (second[0][was] > first[0][was]).all() and (second[1][was] != first[1][was]).all()
        assert (second[1][was] >= 0).sum() >= 100  # a good share of the rays has a second face behind the first


def test_a_stop_leaves_layers_unwalked():
    # on the fine grids a hit ends the walk early: fewer layers than a ray that crosses the whole box
    v, f = R.mesh("spheres")
    grid = D.face_grid(v, f, R.grid_cell("spheres", "cap"))
    rays = R.rays("spheres")[400:600]  # aimed rays, which all hit, and random ones
    t, face, _, count = R.grid_ray_cast(v, f, rays, grid, counts=True)
    assert (face >= 0).any() and (face < 0).any()
    assert count[face >= 0, 0].mean() < count[face < 0, 0].max() and count[:, 0].max() <= 32
    assert count[:, 1].max() < len(f)


@pytest.mark.parametrize("scale", (1.0, 2.0 ** 10, 2.0 ** -6))
def test_sliver(scale):
    v, f, ray = R.sliver(scale)
    cross = D.MR.face_cross(v, f)[0]
    assert cross.tolist() == [0.0, -(2.0 ** -100) * scale * scale, 0.0] and not R.dead_faces(v, f)[0]
    loose = R.ray_cast(v, f, ray, box_clause=False)
    assert loose[1][0] == 0 and loose[0][0] == 1.0 and not loose[2].any()  # "hit" at u = v = 0: corner a ...
    point = ray[0, :3].astype(F64) + loose[0][0] * ray[0, 3:6].astype(F64)
    assert point.tolist() == [100 * scale, 0.0, 0.0]  # ... while o + t d is 98 units past the face's box
    assert R.margin(v) == 2.0 ** -29 * scale
    strict = R.ray_cast(v, f, ray)
    assert strict[1][0] == -1 and strict[0][0] == np.inf
    for cell in (None, 0.25 * scale):
        _same(R.grid_ray_cast(v, f, ray, D.face_grid(v, f, cell)), strict)
    # a ray that does cross the sliver's box is still judged by the same rule in both searches
    through = R.pack([[scale, scale, scale]], [[0, -scale, -scale]])
    _same(R.grid_ray_cast(v, f, through, D.face_grid(v, f, 0.25 * scale)), R.ray_cast(v, f, through))
