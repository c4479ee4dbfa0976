"""kernels.mesh_cluster_labels / mesh_cluster_reduce / mesh_cluster_faces (csrc/mesh_simplify.hip), Mesh.simplify and
the ``simplify`` option of extract_mesh on the device (-m gpu), against the numpy restatement of the contract in
tests/mesh_simplify_reference.py.

Everything is exact: labels, faces and flags as integers; vertices, normals and colours bitwise (the reference does
the same fp32 / int64 / float64 operations in the same order, and the sums are integers).  The inputs are a few
thousand items at most and every reference is computed once per process."""
import numpy as np
import pytest
import torch

import mesh_clean_reference as C
import mesh_simplify_reference as S

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from nerf_amd import kernels
    return kernels


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.cpu().numpy().tobytes()


def _same_bits(got, ref):
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(ref.shape)
    assert _bits(got) == np.ascontiguousarray(ref, np.float32).tobytes()


def _minimal_log2(n):
    return int(n).bit_length()  # the smallest k with 2^k > n


# ------------------------------------------------------------------ labels


@pytest.mark.parametrize("kind", S.VERTEX_KINDS)
@pytest.mark.parametrize("V", S.SIZES)
def test_labels(K, kind, V):
    v, lo, cell, dims = S.vertex_case(kind, V)
    ref = S.cluster_labels(v, lo, cell, dims)
    tables = [None, _minimal_log2(V)] if kind in ("one_cell", "own_cell") else [None]
    if kind == "own_cell":
        tables = tables[::-1]  # the minimal table first: every vertex its own slot, the chains wrap around
    for table_log2 in tables:
        labels, probes = K.mesh_cluster_labels(_dev(v), lo, cell, dims, table_log2=table_log2, return_probes=True)
        print(f"{kind} V={V} table_log2={table_log2}: clusters={len(np.unique(ref))} longest probe chain={probes}")
        assert labels.dtype == torch.int32 and tuple(labels.shape) == (V,)
        assert np.array_equal(labels.cpu().numpy(), ref)  # status[0] == 0: the wrapper raises otherwise
        assert 1 <= probes <= 2 ** (table_log2 or 31)
    if kind == "one_cell":
        assert probes == 1
    assert np.array_equal(K.mesh_cluster_labels(_dev(v), lo, cell, dims).cpu().numpy(), ref)


def test_labels_arguments(K):
    v = _dev(S.vertex_case("random", 65)[0])
    ok = K.mesh_cluster_labels(v, S.LO, S.CELL, S.DIMS, table_log2=7)
    assert ok.shape[0] == 65
    wide = torch.zeros((65, 6), device=DEV)
    bad = [
        dict(vertices=v, lo=S.LO, cell=S.CELL, dims=S.DIMS, table_log2=6),       # 2^6 <= 65
        dict(vertices=v, lo=S.LO, cell=S.CELL, dims=S.DIMS, table_log2=32),
        dict(vertices=v, lo=S.LO, cell=0.0, dims=S.DIMS),
        dict(vertices=v, lo=S.LO, cell=-1.0, dims=S.DIMS),
        dict(vertices=v, lo=S.LO, cell=float("nan"), dims=S.DIMS),
        dict(vertices=v, lo=S.LO, cell=float("inf"), dims=S.DIMS),
        dict(vertices=v, lo=S.LO, cell=1e-46, dims=S.DIMS),                       # 0 as a float32
        dict(vertices=v, lo=S.LO, cell=S.CELL, dims=(5, 0, 3)),
        dict(vertices=v, lo=S.LO, cell=S.CELL, dims=(5, 4, 2 ** 20 + 1)),
        dict(vertices=v, lo=S.LO, cell=S.CELL, dims=(5, 4)),
        dict(vertices=v, lo=S.LO[:2], cell=S.CELL, dims=S.DIMS),
        dict(vertices=v.cpu(), lo=S.LO, cell=S.CELL, dims=S.DIMS),
        dict(vertices=v.double(), lo=S.LO, cell=S.CELL, dims=S.DIMS),
        dict(vertices=wide[:, ::2], lo=S.LO, cell=S.CELL, dims=S.DIMS),
        dict(vertices=v.reshape(-1), lo=S.LO, cell=S.CELL, dims=S.DIMS),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            K.mesh_cluster_labels(**kw)
    empty = K.mesh_cluster_labels(torch.empty((0, 3), device=DEV), S.LO, S.CELL, S.DIMS)
    assert tuple(empty.shape) == (0,) and empty.dtype == torch.int32
    assert K.mesh_cluster_labels(v, S.LO, S.CELL, (2 ** 20, 1, 1)).shape[0] == 65  # the largest axis allowed


# ------------------------------------------------------------------ reduce


def _check_reduce(K, v, lo, cell, dims, n=None, c=None):
    ref_l = S.cluster_labels(v, lo, cell, dims)
    labels = K.mesh_cluster_labels(_dev(v), lo, cell, dims)
    assert np.array_equal(labels.cpu().numpy(), ref_l)
    rv, rn, rc = S.cluster_reduce(v, ref_l, lo, cell, dims, n, c)
    ov, on, oc = K.mesh_cluster_reduce(_dev(v), labels, lo, cell, dims, normals=None if n is None else _dev(n),
                                       colors=None if c is None else _dev(c))
    _same_bits(ov, rv)
    for got, ref in ((on, rn), (oc, rc)):
        if ref is None:
            assert got is None
        else:
            _same_bits(got, ref)
    other = torch.from_numpy(ref_l != np.arange(len(v)))
    for got in (ov, on, oc):
        if got is not None and other.any():
            assert not got.cpu()[other].any()  # zeros at the rows that are no representative
    return ov, on, oc


@pytest.mark.parametrize("V", [65, 2049])
def test_reduce_random(K, V):
    v, lo, cell, dims = S.vertex_case("random", V)
    n, c = S.attribute_case(V)
    assert np.isnan(c).any() and np.isnan(n).any()  # a NaN colour and a NaN normal count as the lower bound
    ov, on, oc = _check_reduce(K, v, lo, cell, dims, n, c)
    assert bool(torch.isfinite(on).all()) and bool(torch.isfinite(oc).all())
    _check_reduce(K, v, lo, cell, dims)            # positions alone
    _check_reduce(K, v, lo, cell, dims, n, None)   # every combination of the two attributes
    _check_reduce(K, v, lo, cell, dims, None, c)


@pytest.mark.parametrize("kind", ["one_cell", "outside", "boundaries", "flat_axis"])
def test_reduce_edges(K, kind):
    """One cluster of 257 members (every add goes to one row), and members outside the grid or on its boundaries
    (u is clamped to [0,1])."""
    v, lo, cell, dims = S.vertex_case(kind, 257)
    n, c = S.attribute_case(257, seed=9)
    _check_reduce(K, v, lo, cell, dims, n, c)


def test_reduce_cancelling_normals(K):
    v, n, lo, cell, dims = S.cancelling_normals()
    _, on, _ = _check_reduce(K, v, lo, cell, dims, n)
    assert on.cpu().tolist() == [[0, 0, 0], [0, 0, 0], [0, 1, 0], [0, 0, 0]]


@pytest.mark.parametrize("name,factor", [("spheres", 1.0), ("spheres", 2.0), ("noise", 1.0), ("noise", 2.0)])
def test_reduce_extracted(K, name, factor):
    v, f, n = S.extracted(name)
    cell = np.float32(factor * S.lattice_spacing(name))
    lo, dims = S.simplify_grid(v, cell)
    _check_reduce(K, v, lo.tolist(), cell, dims, n, S.vertex_colors(len(v)))


def test_reduce_arguments(K):
    v, lo, cell, dims = S.vertex_case("random", 65)
    dv = _dev(v)
    labels = K.mesh_cluster_labels(dv, lo, cell, dims)
    bad_labels = labels.clone()
    bad_labels[3] = 65
    for kw in (dict(labels=labels[:64]), dict(labels=labels.long()), dict(labels=bad_labels), dict(labels=-labels - 1),
               dict(labels=labels, normals=dv[:64]), dict(labels=labels, colors=dv.double()),
               dict(labels=labels.cpu())):
        with pytest.raises(ValueError):
            K.mesh_cluster_reduce(dv, lo=lo, cell=cell, dims=dims, **kw)


# ------------------------------------------------------------------ faces


@pytest.mark.parametrize("kind", S.FACE_KINDS)
@pytest.mark.parametrize("F", S.SIZES)
def test_faces(K, kind, F):
    faces, labels = S.face_case(kind, F)
    ref_f, ref_keep = S.cluster_faces(faces, labels)
    for table_log2 in (_minimal_log2(F), None):  # the minimal table, then the default
        out, keep, probes = K.mesh_cluster_faces(_dev(faces), _dev(labels), table_log2=table_log2, return_probes=True)
        print(f"{kind} F={F} table_log2={table_log2}: kept={int(ref_keep.sum())} longest probe chain={probes}")
        assert out.dtype == torch.int32 and keep.dtype == torch.uint8
        assert np.array_equal(out.cpu().numpy(), ref_f)
        assert np.array_equal(keep.cpu().numpy(), ref_keep)
    if kind == "rotations":
        assert keep.cpu().tolist() == [1] + [0] * (F - 1)  # only face 0
    if kind == "opposite":
        assert keep.cpu().tolist() == ([1, 1] + [0] * (F - 2))[:F]  # the face and its mirror image
    if kind == "strip_distinct":
        assert bool(keep.all())


def test_faces_arguments(K):
    faces, labels = S.face_case("strip_partial", 65)
    f, l = _dev(faces), _dev(labels)
    assert K.mesh_cluster_faces(f, l, table_log2=7)[1].shape[0] == 65
    bad_f = f.clone()
    bad_f[5, 1] = len(labels)
    for args, kw in (((f, l), dict(table_log2=6)), ((bad_f, l), {}), ((f, l.long()), {}), ((f.long(), l), {}),
                     ((f, l.cpu()), {}), ((f, l + 70), {}), ((f.reshape(-1), l), {})):
        with pytest.raises(ValueError):
            K.mesh_cluster_faces(*args, **kw)
    out, keep = K.mesh_cluster_faces(torch.empty((0, 3), dtype=torch.int32, device=DEV), l)
    assert tuple(out.shape) == (0, 3) and tuple(keep.shape) == (0,)


# ------------------------------------------------------------------ Mesh.simplify


def _mesh(name, attributes):
    from nerf_amd import Mesh
    v, f, n = S.extracted(name)
    if not attributes:
        return Mesh(_dev(v), _dev(f))
    return Mesh(_dev(v), _dev(f), _dev(n), _dev(S.vertex_colors(len(v))))


def _assert_mesh(mesh, rv, rf, rn, rc):
    assert mesh.faces.dtype == torch.int32 and tuple(mesh.faces.shape) == (len(rf), 3)
    assert np.array_equal(mesh.faces.cpu().numpy(), rf)
    _same_bits(mesh.vertices, rv)
    for got, ref in ((mesh.normals, rn), (mesh.colors, rc)):
        if ref is None:
            assert got is None
        else:
            _same_bits(got, ref)


@pytest.mark.parametrize("attributes", [False, True])
@pytest.mark.parametrize("name,factor", S.MESH_CASES)
def test_simplify(K, name, factor, attributes):
    mesh = _mesh(name, attributes)
    cell = np.float32(factor * S.lattice_spacing(name))
    rv, rf, rn, rc, _ = S.simplified(name, factor, attributes)
    out = mesh.simplify(cell)
    print(f"{name} x{factor}: V {mesh.vertices.shape[0]} -> {len(rv)}, F {mesh.faces.shape[0]} -> {len(rf)}")
    _assert_mesh(out, rv, rf, rn, rc)
    again = mesh.simplify(float(cell))  # equal inputs, equal bits
    for a, b in ((out.vertices, again.vertices), (out.faces, again.faces), (out.normals, again.normals),
                 (out.colors, again.colors)):
        assert (a is None and b is None) or _bits(a) == _bits(b)


def test_simplify_origin(K):
    v, f, n = S.extracted("noise")
    cell = np.float32(1.5 * S.lattice_spacing("noise"))
    mesh = _mesh("noise", True)
    c = S.vertex_colors(len(v))
    default = mesh.simplify(cell)
    for origin in ((v.min(0) - np.float32(0.37) * cell).astype(np.float32), np.array(C.BOX_LO, np.float32),
                   v.mean(0).astype(np.float32)):  # below the vertices, the lattice's corner, inside the mesh
        rv, rf, rn, rc, _ = S.simplify(v, f, cell, origin=origin, normals=n, colors=c)
        for given in (origin.tolist(), _dev(origin)):
            _assert_mesh(mesh.simplify(cell, origin=given), rv, rf, rn, rc)
    assert default.faces.shape[0] != rf.shape[0] or _bits(default.vertices) != np.ascontiguousarray(rv).tobytes()


def test_simplify_welds(K):
    """A tiny cell welds coincident vertices and removes zero-area triangles: every vertex of the spheres doubled."""
    from nerf_amd import Mesh
    v, f, _ = S.extracted("spheres")
    V = len(v)
    v2 = np.concatenate([v, v], 0)
    f2 = np.where(np.arange(len(f))[:, None] % 2 == 0, f, f + V).astype(np.int32)  # every other face on the copies
    f2 = np.concatenate([f2, np.stack([f[:50, 0], f[:50, 0] + V, f[:50, 1]], 1).astype(np.int32)], 0)  # zero area
    cell = np.float32(1e-4)
    rv, rf, _, _, info = S.simplify(v2, f2, cell)
    assert len(rv) == V and len(rf) == len(f)
    out = Mesh(_dev(v2), _dev(f2)).simplify(cell)
    _assert_mesh(out, rv, rf, None, None)


def test_simplify_empty_and_errors(K):
    from nerf_amd import Mesh
    v, f, n = S.extracted("spheres")
    mesh = _mesh("spheres", True)
    no_faces = Mesh(_dev(v), torch.empty((0, 3), dtype=torch.int32, device=DEV), _dev(n)).simplify(0.1)
    assert tuple(no_faces.vertices.shape) == (0, 3) and tuple(no_faces.faces.shape) == (0, 3)
    assert tuple(no_faces.normals.shape) == (0, 3) and no_faces.colors is None
    nothing = Mesh(torch.empty((0, 3), device=DEV), torch.empty((0, 3), dtype=torch.int32, device=DEV)).simplify(0.1)
    assert tuple(nothing.vertices.shape) == (0, 3) and nothing.faces.dtype == torch.int32 and nothing.normals is None
    for cell in (0.0, -0.1, float("nan"), float("inf"), 1e-46, 1e39):
        with pytest.raises(ValueError):
            mesh.simplify(cell)
    with pytest.raises(ValueError):
        mesh.simplify(1e-7)  # more than 2^20 cells along an axis
    with pytest.raises(ValueError):
        mesh.simplify(0.1, origin=[0.0, 0.0])
    with pytest.raises(ValueError):
        mesh.simplify(0.1, origin=[0.0, float("nan"), 0.0])
    for bad in (float("nan"), float("inf"), -float("inf")):
        w = v.copy()
        w[17, 1] = bad
        with pytest.raises(ValueError):
            Mesh(_dev(w), _dev(f)).simplify(0.1)
    g = f.copy()
    g[3, 2] = len(v)
    with pytest.raises(ValueError):
        Mesh(_dev(v), _dev(g)).simplify(0.1)


# ------------------------------------------------------------------ end to end


@pytest.fixture(scope="module")
def model(K):
    import math
    import ngp_grad_cases as G
    from nerf_amd import ngp as N
    st = G.prod_state()
    st["sigma_head.bias"] = torch.full((1,), math.log(10.0))  # sigma = 10 exp(noise): crosses the threshold 10
    net = N.InstantNGP(occ_conf={}, scene_box=G.AABB, **G.PROD)
    net.load_reference_state(st)
    return net.to(DEV).eval()


RES, CELL = 20, 0.3  # the lattice spacing is 3 / 19


def test_model_simplified_extraction(K, model):
    full = model.extract_mesh(resolution=RES, normals="field", colors="linear")
    small = model.extract_mesh(resolution=RES, normals="field", colors="linear", simplify=CELL)
    print(f"model mesh: V {full.vertices.shape[0]} -> {small.vertices.shape[0]}, "
          f"F {full.faces.shape[0]} -> {small.faces.shape[0]}")
    assert 0 < small.faces.shape[0] < full.faces.shape[0]
    after = full.simplify(CELL)
    assert torch.equal(small.vertices, after.vertices) and torch.equal(small.faces, after.faces)
    # the networks ran after the clustering, on the surviving vertices
    assert torch.equal(small.normals, model.normals(small.vertices))
    assert torch.equal(small.colors, model.vertex_colors(small.vertices, model.normals(small.vertices)))
    # with the component filter in front: filter, then cluster
    both = model.extract_mesh(resolution=RES, normals=None, keep_largest=1, simplify=CELL)
    ref = model.extract_mesh(resolution=RES, normals=None, keep_largest=1).simplify(CELL)
    assert torch.equal(both.vertices, ref.vertices) and torch.equal(both.faces, ref.faces) and both.normals is None


def test_generic_simplified_extraction(K, model):
    from nerf_amd import extract_mesh
    lo, hi = [-1.5] * 3, [1.5] * 3
    plain = extract_mesh(model.density, lo, hi, RES, 10.0)
    again = extract_mesh(model.density, lo, hi, RES, 10.0, simplify=None)  # None: what was returned before
    assert torch.equal(plain.vertices, again.vertices) and torch.equal(plain.faces, again.faces)
    assert torch.equal(plain.normals, again.normals)
    small = extract_mesh(model.density, lo, hi, RES, 10.0, simplify=CELL)  # "grid" normals: averaged by the kernel
    ref = plain.simplify(CELL)
    assert torch.equal(small.vertices, ref.vertices) and torch.equal(small.faces, ref.faces)
    assert torch.equal(small.normals, ref.normals)
    called = extract_mesh(model.density, lo, hi, RES, 10.0, normals=model.normals, simplify=CELL)
    assert torch.equal(called.vertices, ref.vertices) and torch.equal(called.normals, model.normals(ref.vertices))
