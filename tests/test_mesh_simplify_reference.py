"""The vertex-clustering reference (tests/mesh_simplify_reference.py) against itself and against first principles, on
the CPU: the two extracted meshes of mesh_clean_reference and the synthetic sets.  What the device tests compare with
is checked here without a device."""
import numpy as np
import pytest

import mesh_simplify_reference as S


def _check_result(v, f, info, n_in):
    """The first-principle properties of a simplified mesh."""
    assert f.dtype == np.int32 and v.dtype == np.float32
    if len(f):
        assert f.min() >= 0 and f.max() < len(v)  # every index in range
    assert not ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).any()  # no repeated index
    canon = S.canonical(f)
    assert len(np.unique(canon, axis=0)) == len(f)  # no two faces share a canonical form
    assert len(np.unique(f)) == len(v)  # every vertex is used by a face
    # the vertex count is the number of clusters with a surviving face
    kept = info["faces"][info["keep"].astype(bool)]
    assert len(v) == len(np.unique(kept))
    assert (info["labels"][np.unique(kept)] == np.unique(kept)).all()  # and those are representatives


@pytest.mark.parametrize("attributes", [False, True])
@pytest.mark.parametrize("name,factor", S.MESH_CASES)
def test_extracted_meshes(name, factor, attributes):
    vin, fin, _ = S.extracted(name)
    v, f, n, c, info = S.simplified(name, factor, attributes)
    print(f"{name} x{factor}: V {len(vin)} -> {len(v)}, F {len(fin)} -> {len(f)}, "
          f"(degenerate, duplicate, opposite pairs) = {S.face_stats(fin, info['labels'])}")
    assert 0 < len(f) < len(fin) and 0 < len(v) < len(vin)
    _check_result(v, f, info, len(vin))
    assert (n is None) == (not attributes) and (c is None) == (not attributes)
    # every output vertex lies in the closed box of its cell
    lo, dims = info["lo"], info["dims"]
    cell = np.float32(factor * S.lattice_spacing(name))
    reps = np.unique(info["faces"][info["keep"].astype(bool)])
    i, _ = S.cell_indices(vin[reps], lo, cell, dims)
    low = lo.astype(np.float64) + i * np.float64(cell)
    assert (v >= low.astype(np.float32)).all() and (v <= (low + np.float64(cell)).astype(np.float32)).all()
    if attributes:
        assert np.isfinite(n).all() and np.isfinite(c).all()
        length = np.linalg.norm(n.astype(np.float64), axis=1)
        assert (np.abs(length[length > 0] - 1) < 1e-6).all()
        assert c.min() >= 0 and c.max() <= 1
    # kept faces keep their order: the kept rows, renumbered, are the output
    assert len(f) == int(info["keep"].sum())


def test_orientation_numbers():
    """The figures of the prototype this reference replaces (for orientation; the reference decides)."""
    got = {}
    for name, factor in S.MESH_CASES:
        v, f, _, _, info = S.simplified(name, factor, False)
        got[(name, factor)] = (len(v), len(f)) + S.face_stats(S.extracted(name)[1], info["labels"])
    print(got)
    assert got[("spheres", 2.0)][3] == 0  # the spheres never exercise the duplicate path
    assert got[("noise", 1.5)][3] > 0 and got[("noise", 2.0)][3] > 0  # the noise mesh does, with real data
    assert got[("noise", 1.5)][4] > 0  # opposite-orientation pairs exist and are kept


@pytest.mark.parametrize("kind", S.VERTEX_KINDS)
@pytest.mark.parametrize("V", S.SIZES)
def test_label_rules(kind, V):
    v, lo, cell, dims = S.vertex_case(kind, V)
    assert v.shape == (V, 3) and v.dtype == np.float32
    labels = S.cluster_labels(v, lo, cell, dims)
    assert np.array_equal(labels, S.cluster_labels_sorted(v, lo, cell, dims))  # a sort instead of a dictionary
    keys = S.cell_keys(v, lo, cell, dims)
    assert keys.min() >= 0 and keys.max() < int(np.prod(dims))
    assert (labels <= np.arange(V)).all() and (labels[labels] == labels).all()
    assert np.array_equal(keys[labels], keys)
    if kind == "one_cell":
        assert (labels == 0).all()
    if kind == "own_cell":
        assert np.array_equal(labels, np.arange(V))
    if kind == "flat_axis":
        i, _ = S.cell_indices(v, lo, cell, dims)
        assert (i[:, 1] == 0).all()
    if kind == "outside" and V >= 63:
        i, t = S.cell_indices(v, lo, cell, dims)
        assert (t < 0).any() and (t >= np.array(dims)).any()
        assert i.min() == 0 and (i.max(0) == np.array(dims) - 1).all()
    if kind == "boundaries" and V >= 63:
        i, t = S.cell_indices(v, lo, cell, dims)
        assert (t == np.floor(t)).all() and (t == np.array(dims)).any()  # exact, the upper face included
        assert (i.max(0) == np.array(dims) - 1).all()


def test_reduce_rules():
    V = 257
    v, lo, cell, dims = S.vertex_case("random", V)
    n, c = S.attribute_case(V)
    labels = S.cluster_labels(v, lo, cell, dims)
    ov, on, oc = S.cluster_reduce(v, labels, lo, cell, dims, n, c)
    rep = labels == np.arange(V)
    assert not ov[~rep].any() and not on[~rep].any() and not oc[~rep].any()  # zeros at the other rows
    assert np.isfinite(ov).all() and np.isfinite(on).all() and np.isfinite(oc).all()  # NaN attributes are clamped
    # against plain float64 means: the fixed point is 2^-24 of a cell, the output one fp32 rounding
    for r in np.flatnonzero(rep)[:20]:
        m = labels == r
        want = v[m].astype(np.float64).mean(0)
        assert np.abs(ov[r] - want).max() < 4e-7 * (1 + np.abs(want).max())
        cm = np.nan_to_num(np.clip(c[m].astype(np.float64), 0, 1), nan=0.0).mean(0)
        assert np.abs(oc[r] - cm).max() < 2e-7
    # positions alone give the same positions
    assert S.cluster_reduce(v, labels, lo, cell, dims)[0].tobytes() == ov.tobytes()
    v4, n4, lo, cell, dims = S.cancelling_normals()
    l4 = S.cluster_labels(v4, lo, cell, dims)
    assert l4.tolist() == [0, 0, 2, 2]
    _, on4, _ = S.cluster_reduce(v4, l4, lo, cell, dims, n4)
    assert on4.tolist() == [[0, 0, 0], [0, 0, 0], [0, 1, 0], [0, 0, 0]]


@pytest.mark.parametrize("kind", S.FACE_KINDS)
@pytest.mark.parametrize("F", S.SIZES)
def test_face_rules(kind, F):
    faces, labels = S.face_case(kind, F)
    assert faces.shape == (F, 3) and faces.min() >= 0 and faces.max() < len(labels)
    g, keep = S.cluster_faces(faces, labels)
    assert np.array_equal(g, labels[faces])
    ok = (g[:, 0] != g[:, 1]) & (g[:, 1] != g[:, 2]) & (g[:, 0] != g[:, 2])
    # a second way to the duplicates: the first occurrence of every canonical row, by numpy's unique
    _, first = np.unique(S.canonical(g[ok]), axis=0, return_index=True)
    want = np.zeros(F, np.uint8)
    want[np.flatnonzero(ok)[first]] = 1
    assert np.array_equal(keep, want)
    if kind == "rotations":
        assert keep.tolist() == [1] + [0] * (F - 1)
    if kind == "opposite":
        assert keep.tolist() == ([1, 1] + [0] * (F - 2))[:F]
    if kind == "strip_distinct":
        assert keep.all()
    if kind == "strip_partial" and F >= 63:
        assert 0 < keep.sum() < F and not ok[:F // 2 - 2].any() and ok[F // 2 + 2:].all()
    if kind == "degenerate" and F >= 63:
        before = (faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 0] == faces[:, 2])
        assert before.any() and (~before & ~ok).any() and ok.any()  # degenerate before, only after, and good faces


def test_origin_and_grid():
    v, f, _ = S.extracted("noise")
    cell = np.float32(1.5 * S.lattice_spacing("noise"))
    lo, dims = S.simplify_grid(v, cell)
    assert np.array_equal(lo, v.min(0)) and min(dims) >= 1
    i, _ = S.cell_indices(v, lo, cell, dims)
    assert (i.max(0) == np.array(dims) - 1).all()  # the grid is exactly as large as the vertices need
    origin = (v.min(0) - np.float32(0.37) * cell).astype(np.float32)
    a = S.simplify(v, f, cell)
    b = S.simplify(v, f, cell, origin=origin)
    assert len(a[1]) != len(b[1]) or a[0].tobytes() != b[0].tobytes()  # another origin, another clustering
    _check_result(b[0], b[1], b[4], len(v))
