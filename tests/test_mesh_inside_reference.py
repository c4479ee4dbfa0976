"""The reference of the crossing counts (tests/mesh_inside_reference.py), pinned to facts that do not
depend on it: the tables of the contract, the exact sign against rational arithmetic where floating point fails,
the column walk against brute force, and parity against the analytic sphere.  CPU only."""
import math

import numpy as np
import pytest

import mesh_distance_reference as D
import mesh_inside_reference as R
import mesh_metrics_reference as MR
import mesh_raycast_reference as RC

F32 = np.float32


# ------------------------------------------------------------------ orient


def _agree(P, Q, R_):
    want = R.orient_fraction(P, Q, R_)
    got, exact = R.orient_float(P, Q, R_)
    assert got == want, (P, Q, R_, got, want)
    return want, exact


def test_filter_and_expansion_agree_with_fractions_on_near_collinear_triples():
    rng = np.random.default_rng(0)
    signs, exact_path = {-1: 0, 0: 0, 1: 0}, 0
    for e in range(-20, 21, 4):
        scale = 2.0 ** e
        for _ in range(200):
            P, Q = (rng.uniform(-1, 1, 2) * scale).astype(F32), (rng.uniform(-1, 1, 2) * scale).astype(F32)
            t = rng.uniform(-1, 2)
            on = (P.astype(np.float64) + t * (Q.astype(np.float64) - P)).astype(F32)  # rounded onto the line
            for nudge in (on, np.nextafter(on, F32(np.inf)), np.nextafter(on, F32(-np.inf)),
                          np.array([np.nextafter(on[0], F32(np.inf)), on[1]], F32)):  # one-ulp nudges
                s, exact = _agree(P, Q, nudge)
                signs[s] += 1
                exact_path += exact
            # three points a few ulps apart, far from the origin: the six products agree in their leading 40 bits
            B = (rng.uniform(0.5, 1, 2) * scale * rng.choice([-1, 1], 2)).astype(F32)
            ulp = np.abs(np.nextafter(B, F32(np.inf)) - B)
            for _ in range(4):
                Q, R_ = (B + rng.integers(-2, 3, 2).astype(F32) * ulp for _ in range(2))
                assert Q.dtype == F32 and R_.dtype == F32
                s, exact = _agree(B, Q, R_)
                signs[s] += 1
                exact_path += exact
    print(signs, "exact path:", exact_path)
    assert min(signs.values()) > 50 and exact_path > 1000  # the hard cases are met, all three outcomes occur


def test_exactly_collinear_lattice_triples_give_zero():
    rng = np.random.default_rng(1)
    for e in (-20, -7, 0, 9, 20):
        for _ in range(100):
            P, d = rng.integers(-2 ** 11, 2 ** 11, 2), rng.integers(-2 ** 10, 2 ** 10, 2)
            j, k = rng.integers(-2 ** 10, 2 ** 10, 2)
            pts = [(P + m * d).astype(np.float64) * 2.0 ** e for m in (0, j, k)]
            assert all(float(F32(x)) == x for p in pts for x in p)  # representable: the triple is exactly collinear
            assert _agree(*pts) == (0, True)
            off = pts[2] + np.array([2.0 ** e, 0.0])  # one lattice step off the line
            s, _ = _agree(pts[0], pts[1], off)
            assert s == R.orient_fraction(pts[0], pts[1], off) and (s != 0 or d[1] == 0 or j == 0)


def test_expansion_survives_cancellation_across_the_whole_exponent_range():
    big, tiny = F32(2.0 ** 100), F32(2.0 ** -120)
    # orient = big * tiny-scale differences: the products differ by 2^220 in size and the sum cancels to one term
    for P, Q, R_ in (((0, 0), (big, big), (big, big)), ((tiny, 0), (big, big), (-big, -big)),
                     ((0, tiny), (big, big), (-big, -big)), ((tiny, tiny), (big, big), (-big, -big))):
        _agree(np.array(P, F32), np.array(Q, F32), np.array(R_, F32))
    assert R.expansion_sign([1e300, 1.0, -1e300, -1.0, 2.0 ** -1000, 0.0]) == 1
    assert R.expansion_sign([1e300, 1.0, -1e300, -1.0, -(2.0 ** -1000), 0.0]) == -1
    assert R.expansion_sign([1e300, 1.0, -1e300, -1.0, 0.0, 0.0]) == 0


# ------------------------------------------------------------------ the rule


def test_table_on_one_triangle():
    v, f = R.TRIANGLE
    for (x, y), want in R.TABLE:
        for tri, winding in ((f, 1), (f[:, ::-1], -1)):
            c, w = R.brute(v, tri, [[x, y, -1]])
            assert (int(c[0]), int(w[0])) == (want, winding * want), (x, y, winding)
        for qz in (0.0, 1.0):  # the ray is open at its origin: a query in the face's plane, or above it
            assert R.brute(v, f, [[x, y, qz]])[0][0] == 0
    assert sum(want for _, want in R.TABLE[1:4]) == 2 and sum(want for _, want in R.TABLE[4:]) == 1


def test_octahedron():
    v, f = RC.octahedron()
    assert R.volume(v, f) == pytest.approx(4.0)  # wound outwards
    for q, want in R.OCTAHEDRON:
        c, w = R.brute(v, f, [q])
        assert (int(c[0]), int(w[0])) == want, q


def test_every_edge_and_vertex_of_a_closed_projection_has_one_owner():
    """the perturbation argument on the octahedron: from below, every query on the projection of an edge or of a
    vertex that lies inside the outline crosses exactly one lower and one upper face"""
    v, f = RC.octahedron()
    q = [(0, 0), (.5, 0), (-.5, 0), (0, .75), (0, -.75), (.25, 0), (0, .375), (.5, .75 * .5), (-.25, 0)]
    c, w = R.brute(v, f, [[x, y, -3] for x, y in q])
    assert (c == 2).all() and (w == 0).all()
    rim = [(1, 0), (-1, 0), (0, 1.5), (0, -1.5), (.5, .75), (-.5, .75), (.5, -.75), (-.5, -.75)]
    c, w = R.brute(v, f, [[x, y, -3] for x, y in rim])
    assert ((c == 0) | (c == 2)).all() and (w == 0).all() and 0 < (c == 2).sum() < len(rim)


# ------------------------------------------------------------------ the walk


@pytest.mark.parametrize("which", ("one_cell", "default", "cap"))
@pytest.mark.parametrize("name", ("sphere12", "spheres", "soup60", "tiny_face"))
def test_column_walk_equals_brute_force(name, which):
    v, f = R.mesh(name)
    grid = D.face_grid(v, f, R.grid_cell(name, which))
    if which != "default":
        assert max(grid["dims"]) == (1 if which == "one_cell" else 1024 if name == "tiny_face" else 32)
    q = R.queries(name)
    want = R.brute_of(name)
    step = {"default": 1, "cap": 4, "one_cell": 16}[which]  # one cell tests every face for every query
    c, w, count = R.column_walk(v, f, q[::step], grid, counts=True)
    assert np.array_equal(c, want[0][::step]) and np.array_equal(w, want[1][::step])
    print(f"{name} {which}: dims={grid['dims']} keys scanned {count[:, 0].mean():.1f}, faces tested "
          f"{count[:, 1].mean():.1f} per query, crossings up to {want[0].max()}, windings {want[1].min()}..{want[1].max()}")
    if which == "one_cell":
        assert (count[:, 1] == len(f)).all()


def test_query_sets_reach_the_cases():
    c, w = R.brute_of("soup60")
    assert w.min() <= -2 and w.max() >= 2 and c.max() >= 4
    c, w = R.brute_of("tiny_face")
    assert (c == 1).sum() >= 100 and (c == 0).sum() >= 100
    q = R.queries("tiny_face")
    under_tiny = (q[:, 0] >= 2) & (q[:, 1] >= 2) & (q[:, 2] < 2)
    assert 0 < c[under_tiny].sum() < under_tiny.sum()  # both outcomes under the tiny face
    for name in ("sphere12", "spheres"):
        c, w = R.brute_of(name)
        assert set(np.unique(w)) <= {0, 1} and ((c & 1) == w).all()  # closed, outward: parity and winding agree
        assert 0.1 < (w == 1).mean() < 0.9


def test_parity_against_the_analytic_sphere():
    q = R.sphere_queries().astype(np.float64)
    c, w = R.brute_of("sphere12")
    r = np.linalg.norm(q, axis=1)
    far = np.abs(r - 0.6) > R.SPHERE_H
    left_out = int((~far).sum())
    print(f"left out {left_out} of {len(q)}")
    assert left_out <= len(q) / 4
    assert np.array_equal((c[far] & 1).astype(bool), r[far] < 0.6)
    assert np.array_equal(w[far], (r[far] < 0.6).astype(np.int32))
    assert R.volume(*R.sphere()) > 0 and R.volume(*D.spheres()) > 0


def test_float_orient_gives_the_same_counts_and_meets_the_exact_path():
    took = [0, 0]

    def orient(P, Q, R_):
        s, exact = R.orient_float(P, Q, R_)
        took[0] += 1
        took[1] += exact
        return s

    v, f = R.sphere()
    got = R.brute(v, f, R.sphere_queries(), orient)
    want = R.brute_of("sphere12")
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    print(f"{took[1]} of {took[0]} orientation tests took the exact path")
    assert took[1] > 0.05 * took[0]  # lattice-aligned queries: the degenerate case is the everyday case


# ------------------------------------------------------------------ the layers above


def test_box_points_follow_rand64():
    lo, hi = (-1.0, 0.5, 2.0), (1.0, 0.75, 2.0)
    for seed in (0, 0x9e3779b97f4a7c15):
        p = R.box_points(257, seed, lo, hi)
        for i in (0, 1, 256):
            for c in range(3):
                u = (int(MR.rand64(seed, R.BOX_STREAM + c, i)) >> 40) / 2.0 ** 24
                want = F32(lo[c]) + F32(u) * (F32(hi[c]) - F32(lo[c]))
                assert p[i, c] == want and F32(u) == u
        assert np.array_equal(p[:100], R.box_points(100, seed, lo, hi))  # a prefix of a longer run
        assert (p >= np.asarray(lo, F32)).all() and (p <= np.asarray(hi, F32)).all() and (p[:, 2] == 2.0).all()
    assert R.BOX_STREAM != MR.STREAM and not np.array_equal(R.box_points(8, 0, lo, hi), R.box_points(8, 1, lo, hi))
    u = R.box_points(4096, 3, (0, 0, 0), (1, 1, 1))
    assert abs(u.mean() - 0.5) < 0.02 and u.max() < 1.0


def test_iou_reference_and_the_chosen_sample_count():
    same = R.iou_reference("self")
    assert same["iou"] == 1.0 and same["count_a"] == same["count_b"] == same["count_intersection"] == same["count_union"]
    lo, hi = same["box"]
    vol_box = R.box_volume(lo, hi)
    p = same["count_a"] / R.IOU_N
    se = vol_box * math.sqrt(p * (1 - p) / R.IOU_N)
    true = R.volume(*R.sphere())
    print(f"volume {true:.5f} estimate {same['volume_a']:.5f} se {se:.5f}")
    assert abs(same["volume_a"] - true) <= 5 * se and 0.3 < p < 0.7
    assert abs(true - 4 / 3 * math.pi * 0.6 ** 3) < 0.05 * true
    other = R.iou_reference("shifted")
    assert 0 < other["count_intersection"] < other["count_a"] < other["count_union"] <= R.IOU_N
    assert other["iou"] == other["count_intersection"] / other["count_union"]
    assert other["count_a"] + other["count_b"] == other["count_intersection"] + other["count_union"]
