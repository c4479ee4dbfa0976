"""The numpy reference of the mesh smoothing (tests/mesh_smooth_reference.py) against first
principles, on the CPU: the GPU tests compare the kernels with this reference bitwise, so it is pinned here.

The quality checks compare quantities of the reference with each other; they hold no tuned number."""
import numpy as np
import pytest

import mesh_reference as R
import mesh_smooth_reference as M

NAMES = tuple(M.lists())


def _rows(row_off, col):
    return [col[row_off[v]:row_off[v + 1]].tolist() for v in range(len(row_off) - 1)]


@pytest.mark.parametrize("name", NAMES)
def test_adjacency_structure(name):
    v, f = M.lists()[name]
    V = len(v)
    row_off, col = M.adjacency(f, V)
    assert row_off.dtype == np.int32 and col.dtype == np.int32 and row_off.shape == (V + 1,)
    assert row_off[0] == 0 and row_off[V] == len(col) and (np.diff(row_off) >= 0).all()
    rows = _rows(row_off, col)
    sets = M.adjacency_sets(f, V)
    for u, row in enumerate(rows):
        assert u not in row
        assert all(a < b for a, b in zip(row, row[1:]))  # strictly ascending: once each
        assert set(row) == sets[u]
        assert all(u in sets[w] for w in row)  # symmetric
    edges = {(min(a, b), max(a, b)) for a, b in R.undirected_edge_counts(f) if a != b}
    assert len(col) == 2 * len(edges)
    used = np.zeros(V, bool)
    used[np.asarray(f).reshape(-1)] = True
    assert all(not rows[u] for u in np.nonzero(~used)[0])


@pytest.mark.parametrize("name", NAMES)
def test_boundary_is_a_pair_that_occurs_once(name):
    v, f = M.lists()[name]
    count = {}
    for a, b, c in np.asarray(f).tolist():
        for x, y in ((a, b), (b, c), (c, a)):
            if x != y:
                count[(x, y)] = count.get((x, y), 0) + 1
                count[(y, x)] = count.get((y, x), 0) + 1
    ref = np.zeros(len(v), np.uint8)
    for (x, _), k in count.items():
        if k == 1:
            ref[x] = 1
    got = M.boundary_vertices(f, len(v))
    assert got.dtype == np.uint8 and np.array_equal(got, ref)


@pytest.mark.parametrize("name", M.CLEAN_LISTS)
def test_boundary_matches_boundary_edges(name):
    v, f = M.lists()[name]
    assert max(R.undirected_edge_counts(f).values()) <= 2  # what makes the list "clean"
    ref = np.zeros(len(v), np.uint8)
    for a, b in R.boundary_edges(f):
        ref[a] = ref[b] = 1
    assert np.array_equal(M.boundary_vertices(f, len(v)), ref)


def test_closed_surfaces_have_no_boundary():
    v, f, _ = M.sphere_mesh()
    assert R.is_closed(f) and not M.boundary_vertices(f, len(v)).any()
    assert not M.boundary_vertices(M.TETRA, 4).any()
    assert np.array_equal(M.boundary_vertices(*[M.lists()["fan300"][1], 301]), np.r_[0, np.ones(300)].astype(np.uint8))
    dm = M.lists()["duplicated_mirrored"]
    assert M.boundary_vertices(dm[1], len(dm[0])).tolist() == [0, 0, 0, 0, 0]  # every pair at least twice


@pytest.mark.parametrize("name", NAMES)
def test_vertex_faces(name):
    v, f = M.lists()[name]
    row_off, col = M.vertex_faces(f, len(v))
    assert row_off[0] == 0 and row_off[-1] == len(col)
    ref = [[] for _ in range(len(v))]
    for j, face in enumerate(np.asarray(f).tolist()):
        for u in sorted(set(face)):
            ref[u].append(j)
    assert _rows(row_off, col) == ref


def test_all_degenerate_list_has_no_entry():
    v, f = M.lists()["only_degenerate"]
    row_off, col = M.adjacency(f, len(v))
    assert len(col) == 0 and not row_off.any()
    assert (M.pair_keys(f) == M.SENTINEL).all()
    assert np.array_equal(M.smooth(v, f, 3), v)


@pytest.mark.parametrize("name", NAMES)
def test_pass_keeps_bits(name):
    v, f = M.lists()[name]
    row_off, col = M.structure(name)[:2]
    assert M.passed(name, 0.0, False).tobytes() == v.tobytes()
    neg = (-np.abs(v)) * np.float32(0.0)  # every coordinate -0.0: q + 0 * x would give +0.0
    assert M.smooth_pass(neg, row_off, col, 0.0).tobytes() == neg.tobytes()
    fixed = M.fixed_mask(len(v)).astype(bool)
    still = fixed | (np.diff(row_off) == 0)
    for s in M.PASS_FACTORS:
        out = M.passed(name, s, True)
        assert out.dtype == np.float32 and out[still].tobytes() == v[still].tobytes()


@pytest.mark.parametrize("name", ["fan300", "soup65", "noise"])
def test_pass_is_the_sequential_double_sum(name):
    v, f = M.lists()[name]
    row_off, col = M.structure(name)[:2]
    for s in (0.5, -0.53):
        out = M.passed(name, s, False)
        for u in list(range(min(len(v), 40))) + [len(v) - 1]:
            nb = col[row_off[u]:row_off[u + 1]]
            for c in range(3):
                if len(nb) == 0:
                    assert out[u, c] == v[u, c]
                    continue
                acc = float(v[nb[0], c])
                for w in nb[1:]:
                    acc = acc + float(v[w, c])  # Python floats are doubles: one rounded addition each
                q = float(v[u, c])
                assert out[u, c] == np.float32(q + float(np.float32(s)) * (acc / float(len(nb)) - q))


def test_full_step_moves_a_fan_centre_to_the_neighbour_mean():
    v, f = M.fan(12)
    v = v.copy()
    v[0] = (0.3, -0.2, 0.5)
    row_off, col = M.adjacency(f, len(v))
    out = M.smooth_pass(v, row_off, col, 1.0)
    mean = v[1:].astype(np.float64).mean(0)
    assert np.abs(out[0] - mean).max() <= 2e-7  # the rim is regular: its mean is the origin, up to fp32 rounding
    assert np.abs(mean).max() <= 1e-7


def test_normals_point_outwards_on_the_extracted_sphere():
    v, f, grid = M.sphere_mesh()
    n = M.compute_normals(v, f)
    radial = v / np.linalg.norm(v, axis=1, keepdims=True)
    assert ((n * radial).sum(1) > 0).all()  # lower density is outside: the convention of Mesh.normals
    assert ((n * grid).sum(1) > 0).all()
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() < 1e-6


def test_normals_zero_without_faces_and_where_they_cancel():
    v, f = M.lists()["unused"]
    n = M.normals_of("unused")
    assert not n[[0, 2, 3, 6]].any() and (np.linalg.norm(n[[1, 4, 5, 7, 8]], axis=1) > 0.99).all()
    v, f = M.lists()["duplicated_mirrored"]
    n = M.normals_of("duplicated_mirrored")
    assert not n[4].any()  # vertex 4 is in (3,1,4) and in its mirror image only: the two cross products cancel exactly
    assert n[0].any()      # vertex 0 is in (0,1,2) twice and in its mirror image once
    both = np.concatenate([f[:3], f[:3][:, [0, 2, 1]]])
    assert not M.compute_normals(v, both).any()
    assert np.array_equal(M.compute_normals(M.TETRA_V[:1], M.TETRA[:0]), np.zeros((1, 3), np.float32))


def test_tetrahedron_normals_by_hand():
    n = M.compute_normals(M.TETRA_V, M.TETRA)
    assert np.allclose(n[0], -np.ones(3) / np.sqrt(3), atol=1e-7)  # the corner at the origin: three unit faces
    assert (n[1:] * (M.TETRA_V[1:] - 0.25)).sum(1).min() > 0


def test_taubin_smooths_the_noisy_sphere():
    v, f = M.noisy_sphere()
    before, after = M.radial_rms(v), M.radial_rms(M.smooth(v, f, 10))
    print(f"RMS radial deviation: {before:.6f} -> {after:.6f}")
    assert after < before


def test_taubin_keeps_the_volume_better_than_laplacian():
    v, f = M.noisy_sphere()
    vol = R.signed_volume(v, f)
    taubin = abs(R.signed_volume(M.smooth(v, f, 10), f) - vol)
    laplace = abs(R.signed_volume(M.smooth(v, f, 20, mu=None), f) - vol)  # the same 20 passes, all at lam
    print(f"volume {vol:.6f}: |change| Taubin {taubin:.6f}, Laplacian {laplace:.6f}")
    assert taubin < laplace


def test_smooth_options():
    v, f = M.lists()["fan_open"]
    b = M.boundary_vertices(f, len(v)).astype(bool)
    assert b.all()  # an open fan: the centre is on the boundary too
    assert M.smooth(v, f, 3).tobytes() == v.tobytes()
    free = M.smooth(v, f, 3, fix_boundary=False)
    assert (free != v).any()
    fixed = np.zeros(len(v), bool)
    fixed[2] = True
    out = M.smooth(v, f, 3, fix_boundary=False, fixed=fixed)
    assert out[2].tobytes() == v[2].tobytes() and (out[0] != v[0]).any()
    assert M.smooth(v, f, 0).tobytes() == v.tobytes()
    p, n = M.smooth(v, f, 2, fix_boundary=False, normals=True)
    assert n.tobytes() == M.compute_normals(p, f).tobytes()
