"""The numpy reference of the mesh metrics (tests/mesh_metrics_reference.py) checked against facts
that do not depend on it: integer arithmetic against Python's, the sampler's geometry and statistics, and the metric
dict on configurations whose answer is known.  No GPU."""
import numpy as np

import mesh_metrics_reference as R

F64 = np.float64


def test_integer_helpers_match_python_ints():
    rng = np.random.default_rng(0)
    a = rng.integers(0, 2 ** 64, 200, dtype=np.uint64)
    b = rng.integers(0, 2 ** 64, 200, dtype=np.uint64)
    b[:4] = (0, 1, 2 ** 63 - 1, 2 ** 64 - 1)
    assert R.umulhi64(a, b).tolist() == [(int(x) * int(y)) >> 64 for x, y in zip(a, b)]

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) % 2 ** 64
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) % 2 ** 64
        return z ^ (z >> 31)

    for seed in R.SAMPLE_SEEDS:
        got = R.rand64(seed, R.STREAM + 1, np.arange(50, dtype=np.uint64)).tolist()
        assert got == [mix((seed * 0x9e3779b97f4a7c15 + mix(((R.STREAM + 1) * 0xd1b54a32d192ed03 + i) % 2 ** 64))
                           % 2 ** 64) for i in range(50)]
    # the 24 bits the project's uniform takes are the top 24 of rand64
    assert int(R.rand64(0, 0, 0) >> np.uint64(40)) < 2 ** 24


def test_points_are_barycentric_and_in_plane():
    v, f = R.soup60()
    pts, face, nrm, (u1, u2) = R.sample_surface(v, f, 5000, 3, "face")
    assert (u1 >= 0).all() and (u2 >= 0).all() and (u1 + u2 <= 1).all()
    p = v.astype(F64)
    p0, p1, p2 = (p[f[face, c]] for c in range(3))
    rebuilt = (1 - u1 - u2)[:, None] * p0 + u1[:, None] * p1 + u2[:, None] * p2
    scale = np.abs(np.stack([p0, p1, p2])).max(0).max(1)
    assert (np.abs(pts - rebuilt).max(1) <= 2.0 ** -23 * scale + 1e-30).all()
    # the distance to the face's plane, against fp32 rounding of the point (half an ulp per axis, three axes)
    n = np.cross(p1 - p0, p2 - p0)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    off = np.abs(((pts.astype(F64) - p0) * n).sum(1))
    assert (off <= 3 * 2.0 ** -24 * scale + 1e-30).all(), off.max()
    assert np.allclose(np.linalg.norm(nrm.astype(F64), axis=1), 1.0, atol=1e-6)
    assert np.allclose(nrm, n, atol=1e-6)


def test_face_counts_follow_the_areas():
    v, f = R.soup60()
    n = 20000
    area = R.face_areas(v, f)
    w, cdf, total = R.area_cdf(area)
    assert sorted(np.nonzero(w == 0)[0].tolist()) == list(R.SOUP_DEAD) and (area[list(R.SOUP_DEAD)] == 0).all()
    assert 2 ** 31 <= w.max() <= 2 ** 32 and total == int(w.sum()) < 2 ** 63
    _, face, _, _ = R.sample_surface(v, f, n, 0)
    counts = np.bincount(face, minlength=len(f))
    assert counts[list(R.SOUP_DEAD)].sum() == 0  # zero-area and repeated-index faces are never chosen
    share = area / area.sum()
    live = w > 0
    z = np.abs(counts - n * share)[live] / np.sqrt(n * share * (1 - share))[live]
    print(f"largest deviation: {z.max():.2f} binomial standard deviations")
    assert z.max() <= 5.0


def test_tiny_face_is_never_picked():
    v, f = R.tiny_face_mesh()
    area = R.face_areas(v, f)
    assert 0 < area[0] / area[1] < 2.0 ** -33
    w, _, _ = R.area_cdf(area)
    assert w.tolist() == [0, 2 ** 31]
    assert (R.sample_surface(v, f, 3000, 1)[1] == 1).all()


def test_vertex_normals_mix_is_unit_and_between_corners():
    v, f, vn = R.sample_meshes()["spheres"]
    _, face, nrm, _ = R.sampled("spheres", 4099, 0, "vertex")
    assert np.allclose(np.linalg.norm(nrm.astype(F64), axis=1), 1.0, atol=1e-6)
    corner = vn[f[face, 0]].astype(F64)
    assert ((nrm * corner).sum(1) > 0.5).all()  # a smooth closed surface: the mix stays near its corners' normals


def test_brute_force_ties_and_empty():
    q, ref, _ = R.nn_cases()["lattice"]
    d2, idx = R.nn_reference("lattice")
    centres = 125
    assert (d2[:centres] == 0.75).all() and (d2[centres:] == 0).all()
    assert idx[centres:].tolist() == list(range(216))
    lat = ref[idx[:centres]]
    assert (lat == q[:centres] - 0.5).all()  # of the 8 equidistant corners the smallest index is the low corner
    d2, idx = R.nn_reference("m0")
    assert np.isinf(d2).all() and (idx == -1).all()


def test_concentric_spheres():
    v, f = R.sphere()
    n = 4000
    inner, outer = (v, f), ((v * np.float32(1.5)).astype(np.float32), f)
    m = R.mesh_distance(inner, outer, n, seed=0, thresholds=(0.1, 0.4))
    spacing = np.sqrt(R.face_areas(*outer).sum() / n)
    gap = 0.5 * np.linalg.norm(v.astype(F64), axis=1).mean()  # the radius difference of the two meshes
    print(f"gap {gap:.4f}, a_to_b_mean {m['a_to_b_mean']:.4f}, b_to_a_mean {m['b_to_a_mean']:.4f}, spacing {spacing:.4f}")
    assert abs(m["a_to_b_mean"] - gap) <= spacing
    assert abs(m["b_to_a_mean"] - gap) <= spacing
    assert m["hausdorff"] >= gap - spacing and m["chamfer"] == (m["a_to_b_mean"] + m["b_to_a_mean"]) / 2
    assert m["precision@0.1"] == 0 and m["recall@0.1"] == 0 and m["fscore@0.1"] == 0  # 0 / 0 is defined as 0
    assert m["precision@0.4"] == 1 and m["recall@0.4"] == 1 and m["fscore@0.4"] == 1


def test_mesh_against_itself_is_exactly_zero():
    v, f = R.sphere()
    m = R.mesh_distance((v, f), (v, f), 3000, seed=4, thresholds=(0.0,), normals=True)
    for key in ("a_to_b_mean", "a_to_b_rms", "a_to_b_max", "b_to_a_mean", "b_to_a_rms", "b_to_a_max", "chamfer",
                "chamfer_sq", "hausdorff"):
        assert m[key] == 0.0, key
    assert m["precision@0.0"] == 1 and m["recall@0.0"] == 1 and m["fscore@0.0"] == 1
    assert abs(m["normal_consistency"] - 1) < 1e-6
    other = R.mesh_distance((v, f), (v, f), 3000, seed=4)
    assert other == {k: m[k] for k in other}
    # another seed on one side: the point-set distance of a surface to itself is small but not zero
    a, b = R.sample_surface(v, f, 3000, 4)[0], R.sample_surface(v, f, 3000, 5)[0]
    c = R.point_set_metrics(a, b)[0]["chamfer"]
    assert 0 < c <= np.sqrt(R.face_areas(v, f).sum() / 3000)
