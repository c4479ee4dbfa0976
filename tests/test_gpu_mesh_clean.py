"""kernels.mesh_components / mesh_compact (csrc/mesh_clean.hip), Mesh.components / filter_components / select_faces and
the colours and filters of InstantNGP.extract_mesh on the device (-m gpu), against the numpy restatement in
tests/mesh_clean_reference.py.

Everything is exact: labels, face counts and faces as integers, vertices and attributes bitwise (they are gathered,
never recomputed).  The extracted meshes stay below 2.5k lattice points so the looped reference takes seconds; every
reference is computed once per process (mesh_clean_reference caches them)."""
import numpy as np
import pytest
import torch

import mesh_clean_reference as C
import mesh_reference as R

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


def _components(K, faces, V):
    labels, counts, steps = K.mesh_components(_dev(faces.reshape(-1, 3)), V, return_steps=True)
    assert labels.dtype == torch.int32 and counts.dtype == torch.int32
    assert tuple(labels.shape) == (V,) and tuple(counts.shape) == (V,)
    return labels.cpu().numpy(), counts.cpu().numpy(), steps


def _check_components(K, name, faces, V):
    ref_l = C.component_labels(faces, V)
    ref_c = C.face_counts(faces, ref_l)
    labels, counts, steps = _components(K, faces, V)
    print(f"{name}: V={V} F={len(faces)} components={len(np.unique(ref_l))} most find steps of a face={steps}")
    assert np.array_equal(labels, ref_l)
    assert np.array_equal(counts, ref_c)
    return ref_l, ref_c


# ------------------------------------------------------------------ components


@pytest.mark.parametrize("numbering", ["identity", "reversed", "random"])
@pytest.mark.parametrize("n_faces", C.STRIP_F)
def test_strip(K, n_faces, numbering):
    faces, V = C.synthetic_lists()[f"strip{n_faces}-{numbering}"]
    labels, counts = _check_components(K, f"strip{n_faces}-{numbering}", faces, V)
    assert (labels == 0).all() and counts[0] == n_faces


@pytest.mark.parametrize("name", ["interleaved", "bridged", "duplicated", "degenerate"])
def test_strip_variants(K, name):
    faces, V = C.synthetic_lists()[name]
    labels, counts = _check_components(K, name, faces, V)
    with_faces = int((counts > 0).sum())
    if name == "interleaved":
        assert with_faces == 2 and len(np.unique(labels)) == 2 + 5
    if name == "bridged":
        assert with_faces == 1 and len(np.unique(labels)) == 1 + 5
    if name == "duplicated":
        assert with_faces == 1 and counts[0] == 2 * 257
    if name == "degenerate":
        assert (faces[:, 0] == faces[:, 1]).any() and ((faces[:, 0] == faces[:, 1]) & (faces[:, 1] == faces[:, 2])).any()


def test_two_spheres(K):
    v, f, _ = C.two_spheres_mesh()
    labels, counts = _check_components(K, "two spheres", f, len(v))
    sizes = sorted(counts[counts > 0].tolist())
    assert len(np.unique(labels)) == 2 and len(sizes) == 2 and sizes[0] != sizes[1]


def test_noise(K):
    v, f, _ = C.noise_mesh()
    ref_l = C.component_labels(f, len(v))
    sizes = C.face_counts(f, ref_l)
    sizes = sizes[sizes > 0]
    assert len(sizes) >= 50 and len(np.unique(sizes)) >= 10  # not a degenerate input
    _check_components(K, "noise", f, len(v))


def test_no_faces(K):
    empty = torch.empty((0, 3), dtype=torch.int32, device=DEV)
    labels, counts = K.mesh_components(empty, 0)
    assert tuple(labels.shape) == (0,) and tuple(counts.shape) == (0,)
    assert labels.dtype == torch.int32 and counts.dtype == torch.int32
    labels, counts = K.mesh_components(empty, 7)
    assert labels.cpu().tolist() == list(range(7)) and counts.cpu().tolist() == [0] * 7


# ------------------------------------------------------------------ filtering and compaction


def _mesh(mesh_np, colors=True):
    from nerf_amd import Mesh
    v, f, n = mesh_np
    c = np.random.default_rng(11).uniform(0, 1, v.shape).astype(np.float32) if colors else None
    return Mesh(_dev(v), _dev(f), _dev(n), None if c is None else _dev(c)), c


def _assert_mesh_equals(mesh, ref_v, ref_f, ref_n=None, ref_c=None):
    assert mesh.vertices.dtype == torch.float32 and mesh.faces.dtype == torch.int32
    assert tuple(mesh.vertices.shape) == (len(ref_v), 3) and tuple(mesh.faces.shape) == (len(ref_f), 3)
    assert np.array_equal(mesh.faces.cpu().numpy(), ref_f)
    assert mesh.vertices.cpu().numpy().tobytes() == np.ascontiguousarray(ref_v, np.float32).tobytes()
    for got, ref in ((mesh.normals, ref_n), (mesh.colors, ref_c)):
        if ref is None:
            assert got is None
        else:
            assert tuple(got.shape) == (len(ref_v), 3) and got.dtype == torch.float32
            assert got.cpu().numpy().tobytes() == np.ascontiguousarray(ref, np.float32).tobytes()


def _noise_sizes():
    v, f, _ = C.noise_mesh()
    labels = C.component_labels(f, len(v))
    counts = C.face_counts(f, labels)
    order = sorted(np.unique(labels).tolist(), key=lambda l: (-int(counts[l]), l))
    return labels, counts, order


def _filter_cases():
    _, counts, order = _noise_sizes()
    tie = next(i for i in range(1, len(order)) if counts[order[i - 1]] == counts[order[i]] > 0)
    existing = int(counts[order[len(order) // 3]])
    return {
        "min1": dict(min_faces=1),
        "min_existing_size": dict(min_faces=existing),
        "min_above_largest": dict(min_faces=int(counts.max()) + 1),
        "largest1": dict(keep_largest=1),
        "largest3": dict(keep_largest=3),
        "largest_across_tie": dict(keep_largest=tie),
        "largest_above_count": dict(keep_largest=len(order) + 10),
    }


@pytest.mark.parametrize("case", ["min1", "min_existing_size", "min_above_largest", "largest1", "largest3",
                                  "largest_across_tie", "largest_above_count"])
def test_filter_components_on_noise(K, case):
    kw = _filter_cases()[case]
    v, f, n = C.noise_mesh()
    mesh, c = _mesh(C.noise_mesh())
    keep = C.filter_components(f, len(v), **kw)
    rv, rf, (rn, rc) = C.compact(v, f, keep, [n, c])
    print(f"{case} {kw}: {int(keep.sum())} of {len(f)} faces, {len(rv)} of {len(v)} vertices")
    if case == "min_existing_size":  # the >= boundary: a component of exactly that size is kept, and something is dropped
        _, counts, _ = _noise_sizes()
        assert (counts == kw["min_faces"]).any() and 0 < keep.sum() < len(f)
    if case == "largest_across_tie":  # the cut falls between two components of equal size: the smaller label stays
        _, counts, order = _noise_sizes()
        k = kw["keep_largest"]
        assert counts[order[k - 1]] == counts[order[k]] and order[k - 1] < order[k]
    if case == "min_above_largest":
        assert len(rv) == 0 and len(rf) == 0
    if case in ("min1", "largest_above_count"):
        assert keep.all()
    out = mesh.filter_components(**kw)
    _assert_mesh_equals(out, rv, rf, rn, rc)
    again = mesh.filter_components(**kw)  # determinism: byte-equal
    for a, b in ((out.vertices, again.vertices), (out.faces, again.faces), (out.normals, again.normals),
                 (out.colors, again.colors)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_components_deterministic(K):
    v, f, _ = C.noise_mesh()
    a = _components(K, f, len(v))
    b = _components(K, f, len(v))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    faces, V = C.synthetic_lists()["strip2049-random"]
    a, b = _components(K, faces, V), _components(K, faces, V)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_keep_largest_of_two_spheres(K):
    mesh, _ = _mesh(C.two_spheres_mesh(), colors=False)
    labels, counts = mesh.components()
    assert int((counts > 0).sum()) == 2
    one = mesh.filter_components(keep_largest=1)
    v, f = one.vertices.cpu().numpy(), one.faces.cpu().numpy()
    assert len(f) == int(counts.max())
    assert R.is_closed(f) and R.euler_characteristic(len(v), f) == 2 and R.signed_volume(v, f) > 0
    assert one.colors is None and one.normals is not None


def test_select_faces(K):
    v, f, n = C.noise_mesh()
    mesh, c = _mesh(C.noise_mesh())
    F = len(f)
    same = mesh.select_faces(torch.ones(F, dtype=torch.bool, device=DEV))
    _assert_mesh_equals(same, v, f, n, c)
    for empty_mask in (torch.zeros(F, dtype=torch.bool, device=DEV), torch.zeros(F, dtype=torch.uint8, device=DEV)):
        none = mesh.select_faces(empty_mask)
        _assert_mesh_equals(none, v[:0], f[:0], n[:0], c[:0])
    keep = np.random.default_rng(2).uniform(size=F) < 0.3  # any subset, not whole components
    rv, rf, (rn, rc) = C.compact(v, f, keep, [n, c])
    assert 0 < len(rv) < len(v)
    _assert_mesh_equals(mesh.select_faces(_dev(keep)), rv, rf, rn, rc)
    _assert_mesh_equals(mesh.select_faces(_dev(keep.astype(np.uint8) * 3)), rv, rf, rn, rc)  # any non-zero byte keeps
    # the attributes equal a gather of the originals
    vv, ff, (aa,) = K.mesh_compact(_dev(v), _dev(f), _dev(keep), [_dev(np.concatenate([n, c, v], 1))])
    used = np.unique(f[keep])
    assert np.array_equal(aa.cpu().numpy(), np.concatenate([n, c, v], 1)[used]) and np.array_equal(vv.cpu().numpy(), v[used])


def test_bad_arguments(K):
    """Only inputs the wrappers reject before launching anything."""
    from nerf_amd import Mesh
    ok = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32, device=DEV)
    assert K.mesh_components(ok, 4)[0].cpu().tolist() == [0, 0, 0, 0]
    wide = torch.zeros((2, 6), dtype=torch.int32, device=DEV)
    bad = [
        (torch.tensor([[0, 1, -1]], dtype=torch.int32, device=DEV), 4),   # index -1
        (torch.tensor([[0, 1, 4]], dtype=torch.int32, device=DEV), 4),    # index V
        (ok.long(), 4),                                                   # int64 faces
        (ok.cpu(), 4),                                                    # CPU tensor
        (wide[:, ::2], 4),                                                # not contiguous
        (torch.zeros((2, 4), dtype=torch.int32, device=DEV), 4),          # not (F,3)
        (torch.zeros(6, dtype=torch.int32, device=DEV), 4),
        (ok, -1),
        (ok, 2 ** 31),
    ]
    for faces, V in bad:
        with pytest.raises(ValueError):
            K.mesh_components(faces, V)
    verts = torch.zeros((4, 3), device=DEV)
    keep = torch.ones(2, dtype=torch.bool, device=DEV)
    assert K.mesh_compact(verts, ok, keep)[1].shape[0] == 2
    bad_compact = [
        (verts, ok, torch.ones(3, dtype=torch.bool, device=DEV), ()),     # a mask of the wrong length
        (verts, ok, torch.ones(2, dtype=torch.int32, device=DEV), ()),    # a mask of the wrong dtype
        (verts, ok, keep.cpu(), ()),
        (verts[:3], ok, keep, ()),                                        # index 3 >= V = 3
        (verts.double(), ok, keep, ()),
        (verts, ok.long(), keep, ()),
        (verts, ok, keep, (torch.zeros((3, 2), device=DEV),)),            # attribute rows != V
        (verts, ok, keep, (torch.zeros(4, device=DEV),)),
    ]
    for v, f, k, attrs in bad_compact:
        with pytest.raises(ValueError):
            K.mesh_compact(v, f, k, attrs)
    mesh = Mesh(verts, ok)
    for kw in ({}, dict(min_faces=1, keep_largest=1)):
        with pytest.raises(ValueError):
            mesh.filter_components(**kw)
    with pytest.raises(ValueError):
        mesh.select_faces(torch.ones(3, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError):
        Mesh(verts, ok, colors=torch.zeros((3, 3), device=DEV))


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


RES = 20


@pytest.fixture(scope="module")
def plain(model):
    return model.extract_mesh(resolution=RES, normals="field")


@pytest.fixture(scope="module")
def coloured(model):
    return model.extract_mesh(resolution=RES, normals="field", colors="linear")


def test_model_colours(K, model, plain, coloured):
    from nerf_amd.losses import linear_to_srgb
    v = plain.vertices
    assert v.shape[0] > 0 and plain.colors is None
    c = coloured.colors
    assert tuple(c.shape) == (v.shape[0], 3) and c.dtype == torch.float32 and c.is_cuda
    assert float(c.min()) >= 0.0 and float(c.max()) <= 1.0
    with torch.no_grad():
        want = model(torch.cat([v, -model.normals(v)], -1))[:, :3]
    assert torch.equal(c, want)
    assert torch.equal(c, model.vertex_colors(v, model.normals(v)))
    small = model.extract_mesh(resolution=RES, normals="field", colors="linear", chunk=1000)
    assert torch.equal(small.colors, c)
    # the geometry and the normals are those of the call without colours
    for m in (coloured, small):
        assert torch.equal(m.vertices, v) and torch.equal(m.faces, plain.faces) and torch.equal(m.normals, plain.normals)
    srgb = model.extract_mesh(resolution=RES, normals=None, colors="srgb")
    assert srgb.normals is None and torch.equal(srgb.vertices, v) and torch.equal(srgb.faces, plain.faces)
    assert torch.equal(srgb.colors, linear_to_srgb(c))
    grid = model.extract_mesh(resolution=RES, normals="grid", colors="linear")
    assert torch.equal(grid.colors, c)  # the direction is the field normal whatever is stored
    assert torch.equal(grid.normals, model.extract_mesh(resolution=RES, normals="grid").normals)
    with pytest.raises(ValueError):
        model.extract_mesh(resolution=RES, colors="rgb")


def test_model_filtered_extraction(K, model, coloured):
    v, f = coloured.vertices.cpu().numpy(), coloured.faces.cpu().numpy()
    labels = C.component_labels(f, len(v))
    counts = C.face_counts(f, labels)
    sizes = np.sort(counts[counts > 0])
    print(f"model mesh: V={len(v)} F={len(f)} component sizes {sizes.tolist()}")
    assert len(sizes) >= 2 and sizes[0] < sizes[-1]
    m = int(sizes[-1])  # only the largest size survives: some but not all components
    keep = C.filter_components(f, len(v), min_faces=m)
    assert 0 < keep.sum() < len(f)
    direct = model.extract_mesh(resolution=RES, normals="field", colors="linear", min_faces=m)
    after = coloured.filter_components(min_faces=m)
    assert direct.faces.shape[0] == int(keep.sum())
    for a, b in ((direct.vertices, after.vertices), (direct.faces, after.faces), (direct.normals, after.normals),
                 (direct.colors, after.colors)):
        assert torch.equal(a, b)
    n_keep = int((sizes == m).sum())
    largest = model.extract_mesh(resolution=RES, normals="field", colors="linear", keep_largest=n_keep)
    assert torch.equal(largest.faces, direct.faces) and torch.equal(largest.colors, direct.colors)
    with pytest.raises(ValueError):
        model.extract_mesh(resolution=RES, min_faces=1, keep_largest=1)


def test_model_default_is_unchanged(K, model, plain):
    from nerf_amd import density_lattice, extract_mesh
    lo, hi = [-1.5] * 3, [1.5] * 3
    field = density_lattice(model.density, lo, hi, RES)
    v, f = K.mesh_extract(field, 10.0, lo, hi)
    assert torch.equal(plain.vertices, v) and torch.equal(plain.faces, f) and plain.colors is None
    assert torch.equal(plain.normals, model.normals(v))
    generic = extract_mesh(model.density, lo, hi, RES, 10.0)
    assert torch.equal(generic.vertices, v) and torch.equal(generic.faces, f) and generic.colors is None
    assert torch.equal(generic.normals, K.mesh_extract(field, 10.0, lo, hi, normals=True)[2])
    kept = extract_mesh(model.density, lo, hi, RES, 10.0, keep_largest=1)
    ref = generic.filter_components(keep_largest=1)
    assert torch.equal(kept.vertices, ref.vertices) and torch.equal(kept.faces, ref.faces)
    assert torch.equal(kept.normals, ref.normals)
