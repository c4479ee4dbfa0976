"""kernels.mesh_adjacency / mesh_vertex_faces / mesh_smooth_pass / mesh_vertex_normals (csrc/mesh_smooth.hip),
Mesh.adjacency / boundary_vertices / compute_normals / smooth and the ``smooth`` option of extract_mesh on the device
(-m gpu), against the numpy restatement of the contract in tests/mesh_smooth_reference.py.

Everything is exact: the CSR arrays and the boundary flags as integers, vertices and normals bitwise (the reference
does the same float64 operations in the same order).  The inputs are a few thousand items at most and every reference
is computed once per process."""
import numpy as np
import pytest
import torch

import mesh_smooth_reference as M

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAMES = tuple(M.lists())


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from nerf_amd import kernels
    return kernels


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same_bits(got, ref):
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(ref.shape)
    assert got.cpu().numpy().tobytes() == np.ascontiguousarray(ref, np.float32).tobytes()


def _same_ints(got, ref, dtype=torch.int32):
    assert got.dtype == dtype and tuple(got.shape) == tuple(ref.shape)
    assert np.array_equal(got.cpu().numpy(), ref)


# ------------------------------------------------------------------ the two adjacencies


@pytest.mark.parametrize("name", NAMES)
def test_adjacency_boundary_vertex_faces(K, name):
    v, f = M.lists()[name]
    V = len(v)
    row_off, col, boundary, frow, fcol = M.structure(name)
    got = K.mesh_adjacency(_dev(f), V, boundary=True)
    print(f"{name}: V={V} F={len(f)} E={len(col)} boundary vertices={int(boundary.sum())}")
    _same_ints(got[0], row_off)
    _same_ints(got[1], col)
    _same_ints(got[2], boundary, torch.uint8)
    plain = K.mesh_adjacency(_dev(f), V)
    assert len(plain) == 2 and torch.equal(plain[0], got[0]) and torch.equal(plain[1], got[1])
    vf = K.mesh_vertex_faces(_dev(f), V)
    _same_ints(vf[0], frow)
    _same_ints(vf[1], fcol)


def test_adjacency_arguments(K):
    v, f = M.lists()["soup65"]
    fd = _dev(f)
    wide = torch.zeros((len(f), 6), dtype=torch.int32, device=DEV)
    for fn in (K.mesh_adjacency, K.mesh_vertex_faces):
        for bad in (fd.cpu(), fd.long(), wide[:, ::2], fd.reshape(-1), fd[:, :2].contiguous()):
            with pytest.raises(ValueError):
                fn(bad, 65)
        with pytest.raises(ValueError):
            fn(fd, 64)  # an index out of range
        with pytest.raises(ValueError):
            fn(fd, 2 ** 31)
        with pytest.raises(ValueError):  # 6 F reaches 2^31: refused by the shape alone, before any launch
            fn(torch.zeros((1, 3), dtype=torch.int32, device=DEV).expand(2 ** 29, 3), 65)
        row_off, col = fn(torch.empty((0, 3), dtype=torch.int32, device=DEV), 5)[:2]
        assert row_off.tolist() == [0] * 6 and tuple(col.shape) == (0,) and col.dtype == torch.int32
        row_off, col = fn(torch.empty((0, 3), dtype=torch.int32, device=DEV), 0)[:2]
        assert row_off.tolist() == [0] and tuple(col.shape) == (0,)
    assert K.mesh_adjacency(torch.empty((0, 3), dtype=torch.int32, device=DEV), 5, boundary=True)[2].tolist() == [0] * 5


# ------------------------------------------------------------------ one pass


@pytest.mark.parametrize("name", NAMES)
def test_smooth_pass(K, name):
    v, f = M.lists()[name]
    V = len(v)
    row_off, col = (_dev(a) for a in M.structure(name)[:2])
    vd, fixed = _dev(v), _dev(M.fixed_mask(V))
    for s in M.PASS_FACTORS:
        _same_bits(K.mesh_smooth_pass(vd, row_off, col, s), M.passed(name, s, False))
        _same_bits(K.mesh_smooth_pass(vd, row_off, col, s, fixed=fixed), M.passed(name, s, True))
    _same_bits(K.mesh_smooth_pass(vd, row_off, col, 0.5, fixed=fixed.bool()), M.passed(name, 0.5, True))
    out = torch.full_like(vd, float("nan"))
    assert K.mesh_smooth_pass(vd, row_off, col, -0.53, out=out) is out
    _same_bits(out, M.passed(name, -0.53, False))
    _same_bits(vd, v)  # the input is only read


def test_smooth_pass_keeps_negative_zero(K):
    v, f = M.lists()["soup65"]
    row_off, col = (_dev(a) for a in M.structure("soup65")[:2])
    neg = (-np.abs(v)) * np.float32(0.0)
    _same_bits(K.mesh_smooth_pass(_dev(neg), row_off, col, 0.0), neg)


def test_smooth_pass_arguments(K):
    v, f = M.lists()["soup65"]
    ro, co = M.structure("soup65")[:2]
    vd, row_off, col = _dev(v), _dev(ro), _dev(co)
    wide = torch.zeros((65, 6), device=DEV)
    pool = torch.zeros(66 * 3, device=DEV)
    bad_rows = ro.copy()
    bad_rows[3] = bad_rows[4] + 1  # decreases afterwards
    bad_col = co.copy()
    bad_col[5] = 65
    bad = [
        dict(vertices=vd.cpu()), dict(vertices=vd.double()), dict(vertices=wide[:, ::2]), dict(vertices=vd.reshape(-1)),
        dict(row_off=row_off[:-1]), dict(row_off=row_off.long()), dict(row_off=row_off.cpu()),
        dict(row_off=_dev(bad_rows)), dict(row_off=row_off + 1),
        dict(col=col.long()), dict(col=col.cpu()), dict(col=col[:-1].contiguous()), dict(col=_dev(bad_col)),
        dict(col=-col - 1), dict(s=float("nan")), dict(s=float("inf")), dict(s=1e39),
        dict(fixed=torch.zeros(64, dtype=torch.uint8, device=DEV)), dict(fixed=torch.zeros(65, device=DEV)),
        dict(fixed=torch.zeros(65, dtype=torch.uint8)),
        dict(out=vd), dict(vertices=pool[:195].view(65, 3), out=pool[3:].view(65, 3)),  # one row apart: they overlap
        dict(out=torch.empty((64, 3), device=DEV)),
        dict(out=torch.empty((65, 3), dtype=torch.float64, device=DEV)),
    ]
    for kw in bad:
        args = dict(vertices=vd, row_off=row_off, col=col, s=0.5)
        args.update(kw)
        with pytest.raises(ValueError):
            K.mesh_smooth_pass(**args)
    empty = K.mesh_smooth_pass(torch.empty((0, 3), device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV),
                               torch.empty(0, dtype=torch.int32, device=DEV), 0.5)
    assert tuple(empty.shape) == (0, 3)


# ------------------------------------------------------------------ normals


@pytest.mark.parametrize("name", NAMES)
def test_vertex_normals(K, name):
    v, f = M.lists()[name]
    frow, fcol = (_dev(a) for a in M.structure(name)[3:])
    got = K.mesh_vertex_normals(_dev(v), _dev(f), frow, fcol)
    _same_bits(got, M.normals_of(name))
    unused = np.diff(M.structure(name)[3]) == 0
    assert not got.cpu().numpy()[unused].any()


def test_vertex_normals_cancel_and_arguments(K):
    from nerf_amd import Mesh
    v, f = M.lists()["duplicated_mirrored"]
    n = Mesh(_dev(v), _dev(f)).compute_normals().normals.cpu().numpy()
    assert not n[4].any() and n[0].any()  # vertex 4: a face and its mirror image only
    both = np.concatenate([f[:3], f[:3][:, [0, 2, 1]]])
    assert not Mesh(_dev(v), _dev(both)).compute_normals().normals.any()
    frow, fcol = K.mesh_vertex_faces(_dev(f), len(v))
    for kw in (dict(vertices=_dev(v).cpu()), dict(faces=_dev(f).long()), dict(row_off=frow[:-1]),
               dict(col=fcol + len(f)), dict(col=fcol.cpu()), dict(vertices=_dev(v)[:4].contiguous())):
        args = dict(vertices=_dev(v), faces=_dev(f), row_off=frow, col=fcol)
        args.update(kw)
        with pytest.raises(ValueError):
            K.mesh_vertex_normals(**args)


# ------------------------------------------------------------------ Mesh


def _colors(V):
    return np.random.default_rng(11).uniform(0, 1, (V, 3)).astype(np.float32)


@pytest.fixture(scope="module")
def meshes(K):
    """name -> (Mesh on the device with normals and colours, its arrays on the host): the closed two-sphere surface
    and the same surface cut open by select_faces."""
    from nerf_amd import Mesh
    import mesh_simplify_reference as S
    v, f, n = S.extracted("spheres")
    closed = Mesh(_dev(v), _dev(f), _dev(n), _dev(_colors(len(v))))
    centre_x = v[f].mean(1)[:, 0]
    opened = closed.select_faces(_dev((centre_x < -0.8) | (centre_x > 0.7)))  # both spheres lose a cap
    out = {}
    for name, m in (("closed", closed), ("open", opened)):
        out[name] = (m, tuple(t.cpu().numpy() for t in (m.vertices, m.faces, m.normals, m.colors)))
    return out


def test_mesh_adjacency_and_boundary(meshes):
    for name, (mesh, (v, f, n, c)) in meshes.items():
        row_off, col = mesh.adjacency()
        ref = M.adjacency(f, len(v))
        _same_ints(row_off, ref[0])
        _same_ints(col, ref[1])
        b = mesh.boundary_vertices()
        assert b.dtype == torch.bool and np.array_equal(b.cpu().numpy(), M.boundary_vertices(f, len(v)).astype(bool))
        assert bool(b.any()) == (name == "open")


def test_compute_normals(meshes):
    for name, (mesh, (v, f, n, c)) in meshes.items():
        out = mesh.compute_normals()
        _same_bits(out.normals, M.compute_normals(v, f))
        assert out.vertices is mesh.vertices and out.faces is mesh.faces and out.colors is mesh.colors
        assert (out.normals * mesh.normals).sum(1).min() > 0  # the side of the extractor's grid normals


@pytest.mark.parametrize("mu", [-0.53, None])
@pytest.mark.parametrize("fix_boundary", [True, False])
@pytest.mark.parametrize("name", ["open", "closed"])
def test_mesh_smooth(meshes, name, fix_boundary, mu):
    mesh, (v, f, n, c) = meshes[name]
    out = mesh.smooth(3, mu=mu, fix_boundary=fix_boundary)
    rv, rn = M.smooth(v, f, 3, mu=mu, fix_boundary=fix_boundary, normals=True)
    _same_bits(out.vertices, rv)
    _same_bits(out.normals, rn)
    assert torch.equal(out.faces, mesh.faces) and torch.equal(out.colors, mesh.colors)
    _same_bits(mesh.vertices, v)  # the input mesh is untouched
    b = M.boundary_vertices(f, len(v)).astype(bool)
    moved = (out.vertices.cpu().numpy() != v).any(1)
    assert moved.any()
    if fix_boundary:
        assert out.vertices.cpu().numpy()[b].tobytes() == v[b].tobytes()
    elif name == "open":
        assert moved[b].any()
    again = mesh.smooth(3, mu=mu, fix_boundary=fix_boundary)
    assert torch.equal(again.vertices, out.vertices) and torch.equal(again.normals, out.normals)  # equal bits


def test_mesh_smooth_fixed_mask_and_attributes(meshes):
    from nerf_amd import Mesh
    mesh, (v, f, n, c) = meshes["open"]
    fixed = M.fixed_mask(len(v))
    ref = M.smooth(v, f, 2, fixed=fixed)
    for mask in (_dev(fixed), _dev(fixed).bool()):
        _same_bits(mesh.smooth(2, fixed=mask).vertices, ref)
    _same_bits(mesh.smooth(2, fixed=_dev(fixed), fix_boundary=False).vertices,
               M.smooth(v, f, 2, fixed=fixed, fix_boundary=False))
    bare = Mesh(mesh.vertices, mesh.faces).smooth(2, lam=0.25, mu=-0.3)
    assert bare.normals is None and bare.colors is None
    _same_bits(bare.vertices, M.smooth(v, f, 2, lam=0.25, mu=-0.3))


def test_mesh_smooth_zero_iterations_and_empty(meshes):
    from nerf_amd import Mesh
    mesh, _ = meshes["closed"]
    same = mesh.smooth(0)
    for a, b in ((same.vertices, mesh.vertices), (same.faces, mesh.faces), (same.normals, mesh.normals),
                 (same.colors, mesh.colors)):
        assert torch.equal(a, b)
    no_faces = Mesh(mesh.vertices, torch.empty((0, 3), dtype=torch.int32, device=DEV), mesh.normals)
    out = no_faces.smooth(3)
    assert torch.equal(out.vertices, mesh.vertices) and torch.equal(out.normals, mesh.normals)
    assert tuple(out.faces.shape) == (0, 3)
    nothing = Mesh(torch.empty((0, 3), device=DEV), torch.empty((0, 3), dtype=torch.int32, device=DEV))
    out = nothing.smooth(3)
    assert tuple(out.vertices.shape) == (0, 3) and tuple(out.faces.shape) == (0, 3) and out.normals is None
    assert tuple(nothing.compute_normals().normals.shape) == (0, 3)
    assert not no_faces.compute_normals().normals.any()
    assert not no_faces.boundary_vertices().any() and tuple(no_faces.adjacency()[1].shape) == (0,)
    # a host mesh with nothing to launch on comes back too: nothing touches the device
    host = Mesh(torch.zeros((4, 3)), torch.zeros((0, 3), dtype=torch.int32)).smooth(3)
    assert tuple(host.vertices.shape) == (4, 3)


def test_mesh_smooth_arguments(meshes):
    from nerf_amd import Mesh
    mesh, (v, f, n, c) = meshes["closed"]
    V = len(v)
    bad = [dict(iterations=-1), dict(iterations=1.5), dict(iterations="3"), dict(iterations=True), dict(iterations=None),
           dict(lam=0.0), dict(lam=-0.5), dict(lam=1.5), dict(lam=float("nan")), dict(lam=float("inf")),
           dict(lam=1e-46), dict(lam="x"),
           dict(mu=-0.5), dict(mu=0.53), dict(mu=-0.4), dict(mu=float("nan")), dict(mu=float("-inf")), dict(mu=-1e39),
           dict(lam=0.6),  # the default mu = -0.53 is not below -0.6
           dict(fixed=torch.zeros(V - 1, dtype=torch.bool, device=DEV)),
           dict(fixed=torch.zeros((V, 1), dtype=torch.bool, device=DEV)),
           dict(fixed=torch.zeros(V, dtype=torch.int32, device=DEV)), dict(fixed=torch.zeros(V, device=DEV)),
           dict(fixed=[0] * V), dict(fixed=torch.zeros(V, dtype=torch.bool))]
    for kw in bad:
        with pytest.raises(ValueError):
            mesh.smooth(**kw)
    for kw in bad[:19]:  # what needs no look at the data is refused whatever the iteration count
        if "iterations" not in kw:
            with pytest.raises(ValueError):
                mesh.smooth(iterations=0, **kw)
    for value in (np.nan, np.inf, -np.inf):
        w = v.copy()
        w[V // 2, 1] = value
        with pytest.raises(ValueError):
            Mesh(_dev(w), _dev(f)).smooth(1)
    g = f.copy()
    g[3, 2] = V
    with pytest.raises(ValueError):
        Mesh(_dev(v), _dev(g)).smooth(1)
    with pytest.raises(ValueError):  # 6 F reaches 2^31: refused by the shape alone
        Mesh(_dev(v), torch.zeros((1, 3), dtype=torch.int32, device=DEV).expand(2 ** 29, 3)).smooth(1)
    with pytest.raises(ValueError):
        Mesh(torch.from_numpy(v), torch.from_numpy(f)).smooth(1)  # host tensors: no CPU fallback
    assert mesh.smooth(np.int64(1), lam=1.0, mu=-1.01).vertices.shape[0] == V  # the ends of the ranges


# ------------------------------------------------------------------ extract_mesh


def _sphere_density(x):
    return 0.6 - x.norm(dim=-1, keepdim=True)


def test_extract_mesh_smooth(K):
    from nerf_amd import Mesh, extract_mesh
    from nerf_amd.mesh import density_lattice
    lo, hi, res = [-1.0] * 3, [1.0] * 3, 16
    today = Mesh(*K.mesh_extract(density_lattice(_sphere_density, lo, hi, res, device=DEV), 0.0, lo, hi, normals=True))
    plain = extract_mesh(_sphere_density, lo, hi, res, 0.0, device=DEV)
    none = extract_mesh(_sphere_density, lo, hi, res, 0.0, device=DEV, smooth=None)
    for m in (plain, none):  # smooth=None: what is returned today, bit for bit
        assert torch.equal(m.vertices, today.vertices) and torch.equal(m.faces, today.faces)
        assert torch.equal(m.normals, today.normals) and m.colors is None
    ref = plain.smooth(2)
    got = extract_mesh(_sphere_density, lo, hi, res, 0.0, device=DEV, smooth=2)
    assert torch.equal(got.vertices, ref.vertices) and torch.equal(got.faces, ref.faces)
    assert torch.equal(got.normals, ref.normals)
    assert not torch.equal(got.vertices, plain.vertices)
    v, f = plain.vertices.cpu().numpy(), plain.faces.cpu().numpy()
    rv, rn = M.smooth(v, f, 2, normals=True)
    _same_bits(got.vertices, rv)
    _same_bits(got.normals, rn)  # "grid" normals became the face-derived normals of the smoothed mesh
    bare = extract_mesh(_sphere_density, lo, hi, res, 0.0, device=DEV, normals=None, smooth=2)
    assert bare.normals is None and torch.equal(bare.vertices, ref.vertices)
    seen = []

    def normals_fn(x):
        seen.append(x)
        return torch.nn.functional.normalize(x, dim=-1)

    called = extract_mesh(_sphere_density, lo, hi, res, 0.0, device=DEV, normals=normals_fn, smooth=2)
    assert len(seen) == 1 and torch.equal(seen[0], ref.vertices)  # the callable sees the final vertices
    assert torch.equal(called.normals, normals_fn(ref.vertices))
    both = extract_mesh(_sphere_density, lo, hi, res, 0.0, device=DEV, simplify=0.2, smooth=2)
    after = plain.simplify(0.2).smooth(2)
    assert torch.equal(both.vertices, after.vertices) and torch.equal(both.normals, after.normals)
    for bad in (-1, 1.5, "2", True):
        with pytest.raises(ValueError):
            extract_mesh(_sphere_density, lo, hi, res, 0.0, device=DEV, smooth=bad)


def test_model_extract_mesh_smooth(K):
    import math
    import ngp_grad_cases as G
    from nerf_amd import ngp as N
    st = G.prod_state()
    st["sigma_head.bias"] = torch.full((1,), math.log(10.0))  # sigma = 10 exp(noise): crosses the threshold 10
    net = N.InstantNGP(occ_conf={}, scene_box=G.AABB, **G.PROD)
    net.load_reference_state(st)
    net = net.to(DEV).eval()
    plain = net.extract_mesh(resolution=20, normals=None)
    assert plain.faces.shape[0] > 0
    ref = plain.smooth(2)
    got = net.extract_mesh(resolution=20, normals="field", colors="linear", smooth=2)
    assert torch.equal(got.vertices, ref.vertices) and torch.equal(got.faces, plain.faces)
    assert torch.equal(got.normals, net.normals(ref.vertices))  # the networks are queried at the final vertices
    assert torch.equal(got.colors, net.vertex_colors(ref.vertices, got.normals))
    grid = net.extract_mesh(resolution=20, normals="grid", smooth=2)
    assert torch.equal(grid.normals, ref.compute_normals().normals)
    none = net.extract_mesh(resolution=20, normals=None, smooth=None)
    assert torch.equal(none.vertices, plain.vertices) and torch.equal(none.faces, plain.faces)
