"""The quadric-placement reference (tests/mesh_quadric_reference.py) against first principles, on the CPU: its Jacobi
against numpy.linalg.eigh, a cube whose faces, edges and corners it must recover, and a sphere whose volume it must
keep better than the mean.  What the device tests compare with is checked here without a device."""
import numpy as np
import pytest

import mesh_quadric_reference as Q
import mesh_simplify_reference as S


@pytest.mark.parametrize("name,A", Q.matrix_cases(), ids=[n for n, _ in Q.matrix_cases()])
def test_jacobi_against_eigh(name, A):
    lam, E = Q.jacobi_matrix(A)
    scale = np.abs(A).max()
    w, _ = np.linalg.eigh(A)
    assert np.abs(np.sort(lam) - w).max() <= 1e-12 * scale
    assert np.abs(A @ E - E * lam).max() <= 1e-12 * scale  # A e = l e, column by column
    assert np.abs(E.T @ E - np.eye(3)).max() <= 1e-14
    if name in ("zero", "diagonal", "identity", "axis_plane"):
        assert np.array_equal(E, np.eye(3)) and np.array_equal(lam, np.diag(A))  # no rotation at all


def test_jacobi_runs_over_the_clusters():
    """Many matrices at once give what each gives alone, bit for bit (the arrays run over the clusters only)."""
    mats = [A for _, A in Q.matrix_cases()]
    A6 = np.array([[A[0, 0], A[0, 1], A[0, 2], A[1, 1], A[1, 2], A[2, 2]] for A in mats])
    lam, E = Q.jacobi(A6)
    for k, A in enumerate(mats):
        l1, e1 = Q.jacobi_matrix(A)
        assert lam[k].tobytes() == l1.tobytes() and E[k].tobytes() == e1.tobytes()


@pytest.fixture(scope="module")
def cube():
    v, f, cell, origin = Q.cube_case()
    return v, f, cell, Q.simplify(v, f, cell, origin=origin), Q.simplify(v, f, cell, origin=origin, placement="mean")


def test_cube_counts(cube):
    v, f, cell, quad, mean = cube
    assert v.shape == (866, 3) and f.shape == (1728, 3) and abs(Q.volume(v, f) - 1.0) < 1e-12
    ov, of, _, _, info = quad
    assert len(ov) == 152 and len(of) == 300
    fallbacks, used = Q.used_fallbacks(info)
    assert used == 152 and fallbacks == 0
    assert int((info["placed"][info["reps"]] == 0).sum()) == 0
    assert np.bincount(info["rank"], minlength=4).tolist() == [0, 96, 48, 8]  # faces, edges, corners


def test_cube_surface_corners_volume(cube):
    v, f, cell, quad, mean = cube
    ov, of = quad[0], quad[1]
    mv, mf = mean[0], mean[1]
    dist, dist_mean = Q.cube_surface_distance(ov), Q.cube_surface_distance(mv)
    print(f"cube: largest distance to the surface {dist.max():.3g} (quadric), {dist_mean.max():.4f} (mean), "
          f"cell {cell:.4f}; volume {Q.volume(ov, of):.9f} (quadric), {Q.volume(mv, mf):.4f} (mean)")
    assert dist.max() <= 1e-6
    assert dist_mean.max() > 0.1 * cell
    nearest = np.linalg.norm(ov.astype(np.float64)[None] - Q.CUBE_CORNERS[:, None], axis=2).min(1)
    assert nearest.max() <= 1e-6  # each of the 8 corners
    assert abs(Q.volume(ov, of) - 1.0) <= 1e-6
    assert Q.volume(mv, mf) < 0.98


def test_cube_connectivity_is_the_mean_placement_s(cube):
    _, _, _, quad, mean = cube
    assert np.array_equal(quad[1], mean[1])  # the compacted faces
    assert np.array_equal(quad[4]["faces"], mean[4]["faces"]) and np.array_equal(quad[4]["keep"], mean[4]["keep"])
    assert np.array_equal(quad[4]["labels"], mean[4]["labels"])
    assert quad[0].shape == mean[0].shape and quad[0].tobytes() != mean[0].tobytes()


def test_cube_stays_in_its_cells(cube):
    v, f, cell, quad, _ = cube
    info = quad[4]
    reps = info["reps"]
    i, _ = S.cell_indices(v[reps], info["lo"], cell, info["dims"])
    low = info["lo"].astype(np.float64) + i * np.float64(cell)
    p = info["position"][reps].astype(np.float64)
    slack = 1e-6  # the fp32 rounding of the output
    assert (p >= low - slack).all() and (p <= low + np.float64(cell) + slack).all()
    other = np.setdiff1d(np.arange(len(v)), reps)
    assert not info["position"][other].any() and not info["placed"][other].any()


@pytest.mark.parametrize("cell", Q.SPHERE_CELLS)
def test_sphere_volume(cell):
    v, f = Q.sphere_mesh()
    assert v.shape == (2 + 31 * 64, 3)
    qv, qf, _, _, info = Q.simplify(v, f, np.float32(cell))
    mv, mf, _, _, _ = Q.simplify(v, f, np.float32(cell), placement="mean")
    fallbacks, used = Q.used_fallbacks(info)
    vq, vm = Q.volume(qv, qf), Q.volume(mv, mf)
    print(f"sphere cell {cell}: {used} clusters, volume {vq:.4f} (quadric) {vm:.4f} (mean) of {Q.SPHERE_VOLUME:.4f}, "
          f"{fallbacks} fallbacks")
    assert np.array_equal(qf, mf)
    assert abs(vq - Q.SPHERE_VOLUME) < abs(vm - Q.SPHERE_VOLUME)
    assert fallbacks <= 0.05 * used


def test_tol_changes_the_rank():
    """A larger tol drops the weakly constrained directions: the rank of no cluster grows, and that of some falls."""
    v, f = Q.sphere_mesh()
    fine = Q.simplify(v, f, np.float32(0.2), tol=1e-3)[4]
    coarse = Q.simplify(v, f, np.float32(0.2), tol=0.3)[4]
    assert (coarse["rank"] <= fine["rank"]).all() and (coarse["rank"] < fine["rank"]).any()
    assert coarse["position"].tobytes() != fine["position"].tobytes()


def test_special_rows():
    """An empty row, a row of zero-area faces and a face with two corners in one cluster, by hand."""
    lo, cell, dims = S.LO, S.CELL, S.DIMS
    pts = S._points(np.array([[0.5, 0.5, 0.5], [0.6, 0.4, 0.5], [1.5, 0.5, 0.5], [2.5, 0.5, 0.5], [3.5, 0.5, 0.5],
                              [0.5, 1.5, 0.5]]))
    faces = np.array([[0, 1, 2], [3, 3, 3], [0, 0, 5]], np.int32)  # (0,1,2): two corners in cluster 0; (3,3,3); (a,a,b)
    labels = S.cluster_labels(pts, lo, cell, dims)
    assert labels.tolist() == [0, 0, 2, 3, 4, 5]
    row_off, col = Q.cluster_rows(faces, labels)
    assert col[row_off[0]:row_off[1]].tolist() == [0, 2]  # once each
    assert row_off[4] == row_off[5]  # vertex 4: no face
    mean, _, _ = S.cluster_reduce(pts, labels, lo, cell, dims)
    pos, placed, info = Q.cluster_quadric(pts, faces, labels, row_off, col, mean, lo, cell, dims, return_info=True)
    assert placed.tolist() == [1, 0, 1, 0, 0, 0]  # face 2 has no area: clusters 3, 4 and 5 keep the mean
    assert info["rank"].tolist() == [1, 1, 0, 0, 0]
    assert pos[[3, 4, 5]].tobytes() == mean[[3, 4, 5]].tobytes() and not pos[1].any()
    assert pos[0, 2] == mean[0, 2]  # the one plane is z = const: the mean is already on it
