"""The numpy reference of the exact point-to-surface distance (tests/mesh_distance_reference.py) against
values known in closed form, on the CPU: the device tests compare the kernels with this reference bit for bit, so the
reference itself is pinned here."""
import numpy as np

import mesh_distance_reference as D

F32 = np.float32


def test_table_on_one_triangle():
    v, f = D.TRIANGLE
    q = np.array([row[0] for row in D.TABLE], F32)
    d2, face, closest = D.nearest_faces(v, f, q)
    assert d2.dtype == np.float64 and face.dtype == np.int32 and closest.dtype == F32
    assert (face == 0).all()
    for i, (_, want_d2, want_point) in enumerate(D.TABLE):
        assert d2[i] == want_d2, (i, d2[i])
        if want_point is not None:
            assert closest[i].tolist() == list(want_point), (i, closest[i])


def test_mirror_images_tie_bitwise():
    rng = np.random.default_rng(17)
    for _ in range(2000):
        v, f = D.mirror_pair(rng)
        q = rng.uniform(-2, 2, (1, 3)).astype(F32)
        q[0, 0] = 0
        d2, closest = D.closest_points(v, f, q)
        assert d2[0, 0].tobytes() == d2[0, 1].tobytes()
        assert closest[0, 0, 0] == -closest[0, 1, 0] and (closest[0, 0, 1:] == closest[0, 1, 1:]).all()
    assert D.nearest_faces(v, f, q)[1][0] == 0  # the smaller index wins the tie


def test_faces_without_area_stay_finite():
    v, f = D.soup60()
    q = D.queries("soup60")
    d2, closest = D.closest_points(v, f, q)
    assert np.isfinite(d2).all() and np.isfinite(closest).all() and (d2 >= 0).all()
    # a face with a repeated index is a segment (or a point): (20, 20, 20) is the distance to vertex 20
    d = q.astype(np.float64) - v[20].astype(np.float64)
    assert (d2[:, 41] == (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).all()
    # the three windings of the collinear face give one distance (up to the rounding of a reversed segment)
    assert np.allclose(d2[:, 0], d2[:, 30], rtol=1e-12, atol=0) and np.allclose(d2[:, 0], d2[:, 59], rtol=1e-12, atol=0)


def test_closest_point_is_never_farther_than_a_corner():
    v, f = D.soup60()
    q = D.queries("soup60")[:200]
    d2, _ = D.closest_points(v, f, q)
    corner = ((q[:, None, None, :].astype(np.float64) - v[f][None].astype(np.float64)) ** 2).sum(-1).min(-1)
    assert (d2 <= corner * (1 + 1e-12)).all()


def test_grid_search_equals_brute_force():
    v, f = D.soup60()
    q = np.concatenate([D.queries("soup60")[:30], D.queries("soup60")[-10:]])
    want = D.nearest_faces(v, f, q)
    for cell_size in (None, D.cap_cell(v, 12)):
        grid = D.face_grid(v, f, cell_size)
        got = D.grid_nearest_faces(v, f, q, grid)
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes()
    assert max(grid["dims"]) == 12
    keys = D.face_keys(v, f, grid)
    assert len(keys) == D.face_cell_counts(v, f, grid).sum() and (keys[1:] > keys[:-1]).all()


def test_shared_inputs():
    v, _ = D.tiny_face_mesh()
    grid = D.face_grid(v, D.tiny_face_mesh()[1], D.cap_cell(v))
    assert grid["dims"] == [1024, 1024, 1024]
    assert D.face_grid(v, D.tiny_face_mesh()[1], D.one_cell(v))["dims"] == [1, 1, 1]
    q = D.cap_queries()
    assert q.shape == (1000, 3) and (q[:100, 2] < 0).all()  # below the box, whose lower face is z = 0
    d2 = D.brute("tiny_face", "cap")[0]
    assert np.sqrt(d2.max()) <= 24 * np.sqrt(3.0) * D.cap_cell(v) * 1.01  # every query within a few cells of a face
    far = D.queries("soup60")[-100:]
    sv = D.soup60()[0]
    assert (np.abs(far - (sv.min(0) + sv.max(0)) / 2).max(1) > 2 * (sv.max(0) - sv.min(0)).max()).all()
