"""Texture baking on the device (-m gpu): kernels.mesh_atlas_texels / mesh_texture_lookup (csrc/mesh_texture.hip),
Mesh.atlas / atlas_uv / bake_texture / sample_texture / render / save_obj, InstantNGP.bake_texture and
extract_mesh(texture=), TSDFVolume.bake_texture, against the numpy restatement in tests/mesh_texture_reference.py
(DESIGN §3.11.12).

Parity is bit for bit (uint32 views): mesh_texture.o is built with -ffp-contract=off and both sides round every fp32
and double operation once, in the same order.  The one exception is the payload of a NaN, which IEEE 754 leaves to the
implementation: where both sides hold a NaN the bits are not compared.  Every reference is computed once per module;
the shapes are the smallest that reach the edges: an empty mesh, a lone face with L = 1, a half-owned last cell, a
full atlas, whole unowned cells with T = 21 (441 texels cross a 256-thread block and wave edges), and two larger ones.
"""
import functools
import os

import numpy as np
import pytest
import torch

import mesh_texture_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = np.float32
ATLAS_CASES = [(0, 5), (1, 5), (2, 6), (3, 7), (8, 7), (9, 7), (33, 16), (128, 9)]
ZERO_AREA_CASE, NAN_CASE = (8, 7), (9, 7)


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from nerf_amd import kernels
    return kernels


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same_bits(got, ref, nan_ok=False):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == ref.shape and got.dtype == ref.dtype, (got.shape, ref.shape, got.dtype, ref.dtype)
    if got.dtype != F32:
        assert np.array_equal(got, ref)
        return
    same = _bits(got) == _bits(ref)
    if nan_ok:
        same |= np.isnan(got) & np.isnan(ref)
    assert same.all(), f"{int((~same).sum())} of {same.size} elements differ"


@functools.lru_cache(maxsize=None)
def _soup(F, S):
    """A random triangle soup of F faces over 3 + F // 2 vertices, with vertex normals; one case holds a face without
    area, one a NaN vertex."""
    rng = np.random.default_rng(100 * F + S)
    V = 3 + F // 2
    v = rng.uniform(-1, 1, (V, 3)).astype(F32)
    n = rng.normal(size=(V, 3)).astype(F32)
    n[0] = 0  # a zero normal at a vertex: the mix can vanish at that corner
    f = np.stack([rng.permutation(V)[:3] for _ in range(F)]).astype(np.int32) if F else np.zeros((0, 3), np.int32)
    if (F, S) == ZERO_AREA_CASE:
        f[2] = [f[2, 0], f[2, 1], f[2, 1]]
        f[5] = f[5, 0]
    if (F, S) == NAN_CASE:
        v[f[4, 1], 2] = np.nan
    return v, f, n


@functools.lru_cache(maxsize=None)
def _atlas_reference(F, S, with_normals):
    v, f, n = _soup(F, S)
    return R.atlas_texels(v, f, S, n if with_normals else None)


@pytest.mark.parametrize("with_normals", [False, True], ids=["face_normals", "vertex_normals"])
@pytest.mark.parametrize("F,S", ATLAS_CASES)
def test_texel_kernel_parity(K, F, S, with_normals):
    v, f, n = _soup(F, S)
    ref = _atlas_reference(F, S, with_normals)
    got = K.mesh_atlas_texels(_dev(v), _dev(f, np.int32), S, vertex_normals=_dev(n) if with_normals else None)
    assert (got["T"], got["cols"], got["texels"]) == (ref["T"], ref["cols"], S)
    assert got["face"].dtype == torch.int32 and tuple(got["face"].shape) == (ref["T"], ref["T"])
    nan_ok = (F, S) == NAN_CASE
    for key in ("face", "bary", "position", "normal"):
        _same_bits(got[key], ref[key], nan_ok=nan_ok and key in ("position", "normal"))
    if nan_ok:  # the NaN did arrive, and only in the texels of faces that use the vertex
        bad = np.isnan(ref["position"]).any(-1)
        assert bad.any() and np.array_equal(np.isnan(got["position"].cpu().numpy()).any(-1), bad)
    if (F, S) == ZERO_AREA_CASE and not with_normals:
        nrm = got["normal"].cpu().numpy()
        assert (nrm[ref["face"] == 2] == 0).all() and (nrm[ref["face"] == 5] == 0).all()
    without = K.mesh_atlas_texels(_dev(v), _dev(f, np.int32), S, normals=False)
    assert "normal" not in without
    _same_bits(without["position"], ref["position"], nan_ok=nan_ok)
    if F == 0:
        assert bool((got["face"] == -1).all()) and got["T"] == S


def _on_hypotenuse(u):
    """(n,2) float32 pairs with u + v = 1 exactly: u is cut to a multiple of 2^-24, so that 1 - u is a float32 too."""
    u = (np.floor(np.asarray(u, np.float64) * 2.0 ** 24) / 2.0 ** 24).astype(F32)
    return np.stack([u, F32(1) - u], 1)


def _lookup_queries(F, N, seed):
    """(face (N,) int32, bary (N,2) float32): the corners, the edge midpoints, the centroid, u + v = 1 exactly, no
    face, and random interior points, over random faces."""
    rng = np.random.default_rng(seed)
    face = rng.integers(0, max(F, 1), N).astype(np.int32)
    _, bary = R.surface_samples(1, N, seed + 1)
    third = F32(1) / F32(3)
    special = np.array([[0, 0], [1, 0], [0, 1], [0.5, 0], [0, 0.5], [0.5, 0.5], [third, third]], F32)
    k = min(N, special.shape[0])
    bary[:k] = special[:k]
    edge = np.arange(N) % 5 == 3
    bary[edge] = _on_hypotenuse(bary[edge, 0])
    face[np.arange(N) % 7 == 5] = -1
    if F == 0:
        face[:] = -1
    return face, bary


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("F,S", [(3, 5), (9, 7), (128, 8)])
def test_lookup_kernel_parity(K, F, S, C):
    cols, T = R.layout(F, S)
    tex = np.random.default_rng(F + S + C).random((T, T, C)).astype(F32)
    d_tex = _dev(tex)
    for N in (0, 1, 63, 64, 65, 257):
        face, bary = _lookup_queries(F, N, seed=N + C)
        got = K.mesh_texture_lookup(d_tex, S, F, _dev(face, np.int32), _dev(bary))
        assert got.dtype == torch.float32 and tuple(got.shape) == (N, C)
        _same_bits(got, R.texture_lookup(tex, S, F, face, bary))
        assert bool((got[torch.from_numpy(face).to(DEV) < 0] == 0).all())


@pytest.mark.parametrize("F,S", [(3, 5), (9, 7), (128, 8)])
def test_no_bleeding_between_faces(K, F, S):
    own = R.owner(F, S)
    tex = np.where(own >= 0, own.astype(F32) * F32(0.125) + F32(0.0625), F32(-1000.0)).astype(F32)  # exact values
    tex = np.repeat(tex[:, :, None], 3, 2) + np.array([0, 1, 2], F32)
    per = 4096
    face = np.repeat(np.arange(F, dtype=np.int32), per)
    _, bary = R.surface_samples(1, F * per, seed=F)
    kind = np.arange(F * per) % 8
    bary[kind == 1, 0] = 0                                   # the edge u = 0
    bary[kind == 2, 1] = 0                                   # the edge v = 0
    bary[kind == 3] = _on_hypotenuse(bary[kind == 3, 0])     # the hypotenuse, u + v = 1 exactly
    bary[:F * per:per] = [0, 0]
    bary[1:F * per:per] = [1, 0]
    bary[2:F * per:per] = [0, 1]
    got = K.mesh_texture_lookup(_dev(tex), S, F, _dev(face, np.int32), _dev(bary)).cpu().numpy()
    want = (face.astype(F32) * F32(0.125) + F32(0.0625))[:, None] + np.array([0, 1, 2], F32)
    assert np.array_equal(got, want), f"{int((got != want).any(1).sum())} lookups blended another face's texel"


# ------------------------------------------------------------------ the Mesh methods, on the 128-face sphere


@pytest.fixture(scope="module")
def sphere(K):
    from nerf_amd import Mesh
    v, f = R.octasphere(2)
    mesh = Mesh(_dev(v), _dev(f, np.int32))
    before = mesh.cpu()  # a mesh built before any baking
    color = lambda p, n: _dev(R.analytic_color(p.cpu().numpy()))
    textured = Mesh(mesh.vertices, mesh.faces).bake_texture(color, 16)
    return dict(v=v, f=f, plain=mesh, before=before, textured=textured, color=color)


def test_bake_and_sample_round_trip(K, sphere):
    v, f, mesh = sphere["v"], sphere["f"], sphere["textured"]
    assert mesh.texels == 16 and tuple(mesh.texture.shape) == (128, 128, 3) and mesh.texture.dtype == torch.float32
    assert "texture=128" in repr(mesh) and "texture" not in repr(sphere["plain"])
    tex = R.bake(v, f, 16, R.analytic_color)
    _same_bits(mesh.texture, tex)
    face, bary = R.surface_samples(128, 20000, seed=7)
    got = mesh.sample_texture(_dev(face, np.int32), _dev(bary))
    ref = R.texture_lookup(tex, 16, 128, face, bary)
    _same_bits(got, ref)
    truth = R.analytic_color(R.surface_points(v, f, face, bary)).astype(np.float64)
    err_tex = np.abs(got.cpu().numpy().astype(np.float64) - truth)
    assert np.array_equal(err_tex, np.abs(ref.astype(np.float64) - truth))
    err_vert = np.abs(R.vertex_color_mix(R.analytic_color(v), f, face, bary) - truth).mean()
    print(f"mean abs error: vertex mix {err_vert:.3e}, S=16 texture {err_tex.mean():.3e}")
    assert err_tex.mean() < 0.1 * err_vert
    # the dict of the texel kernel, the corner coordinates, the host copy
    a = mesh.atlas(16)
    _same_bits(a["position"], R.atlas_texels(v, f, 16)["position"])
    _same_bits(mesh.atlas_uv(), R.atlas_uv(128, 16))
    _same_bits(sphere["plain"].atlas_uv(7), R.atlas_uv(128, 7))
    host = mesh.cpu()
    assert host.texels == 16 and not host.texture.is_cuda and torch.equal(host.texture, mesh.texture.cpu())
    # a new mesh with other vertices or faces is untextured; the same surface with new normals keeps its texture
    keep = torch.ones(128, dtype=torch.bool, device=DEV)
    keep[5] = False
    assert mesh.select_faces(keep).texture is None and mesh.smooth(1).texture is None
    assert mesh.simplify(0.5).texture is None
    assert mesh.compute_normals().texture is mesh.texture


def test_render_adds_the_texture_image(K, sphere):
    plain, mesh = sphere["plain"], sphere["textured"]
    c2w = torch.tensor([[1.0, 0, 0, 0.2], [0, 1, 0, -0.1], [0, 0, 1, 3.0]], device=DEV)
    cam = dict(H=37, W=41, fx=40.0, fy=40.0, cx=20.5, cy=18.5, c2w=c2w)
    a, b = plain.render(**cam), mesh.render(**cam)
    assert set(b) == set(a) | {"texture"} and "texture" not in a
    for key in a:
        assert np.array_equal(a[key].cpu().numpy().view(np.uint8), b[key].cpu().numpy().view(np.uint8)), key
    from nerf_amd.ray_sampling import rays_for_camera
    rays = rays_for_camera(37, 41, 40.0, 40.0, 20.5, 18.5, c2w, near=0.0, far=float("inf"))
    _, face, bary = mesh.ray_cast(rays)
    hit = (face >= 0).view(37, 41)
    assert bool(hit.any()) and not bool(hit.all())
    assert tuple(b["texture"].shape) == (37, 41, 3)
    assert torch.equal(b["texture"].view(-1, 3), mesh.sample_texture(face, bary))
    assert bool((b["texture"][~hit] == 0).all()) and bool((b["texture"][hit] > 0).any())


def _parse_obj(path):
    out = {"v": [], "vt": [], "vn": [], "f": [], "mtllib": [], "usemtl": []}
    with open(path) as fh:
        for line in fh:
            tag, *rest = line.split()
            out[tag].append(rest)
    return out


def test_save_obj_writes_obj_mtl_and_png(K, sphere, tmp_path):
    from PIL import Image
    plain, mesh = sphere["plain"], sphere["textured"].compute_normals()
    mesh.save_obj(tmp_path / "ball.obj")
    obj = _parse_obj(tmp_path / "ball.obj")
    F, T = 128, 128
    assert obj["mtllib"] == [["ball.mtl"]] and obj["usemtl"] == [["ball"]]
    assert len(obj["v"]) == mesh.vertices.shape[0] == len(obj["vn"]) and len(obj["vt"]) == 3 * F and len(obj["f"]) == F
    uv = R.atlas_uv(F, 16).reshape(-1, 2).astype(np.float64)
    vt = np.array(obj["vt"], np.float64)
    assert np.abs(vt[:, 0] - uv[:, 0] / T).max() < 1e-8 and np.abs(vt[:, 1] - (1 - uv[:, 1] / T)).max() < 1e-8
    faces = mesh.faces.cpu().numpy()
    for k, corners in enumerate(obj["f"]):
        idx = np.array([[int(x) for x in c.split("/")] for c in corners])
        assert idx.shape == (3, 3)
        assert np.array_equal(idx[:, 0] - 1, faces[k]) and np.array_equal(idx[:, 2] - 1, faces[k])
        assert np.array_equal(idx[:, 1] - 1, 3 * k + np.arange(3))
    mtl = (tmp_path / "ball.mtl").read_text()
    assert "newmtl ball" in mtl and "map_Kd ball.png" in mtl
    png = np.asarray(Image.open(tmp_path / "ball.png"))
    want = np.rint(np.clip(mesh.texture.cpu().numpy(), 0.0, 1.0) * 255.0).astype(np.uint8)
    assert png.shape == (T, T, 3) and np.array_equal(png, want)
    # without normals: f a/t
    sphere["textured"].save_obj(tmp_path / "flat.obj")
    flat = _parse_obj(tmp_path / "flat.obj")
    assert not flat["vn"] and all(len(c.split("/")) == 2 for corners in flat["f"] for c in corners)
    # an untextured mesh writes what it always has, and no other file
    plain.save_obj(tmp_path / "plain.obj")
    sphere["before"].save_obj(tmp_path / "before.obj")
    data = (tmp_path / "plain.obj").read_bytes()
    assert data == (tmp_path / "before.obj").read_bytes()
    lines = ["v %.9g %.9g %.9g\n" % tuple(x) for x in sphere["v"].tolist()]
    lines += ["f %d %d %d\n" % tuple(x) for x in (sphere["f"] + 1).tolist()]
    assert data == "".join(lines).encode()
    assert sorted(os.listdir(tmp_path)) == ["ball.mtl", "ball.obj", "ball.png", "before.obj", "flat.mtl", "flat.obj",
                                            "flat.png", "plain.obj"]


# ------------------------------------------------------------------ the models


@pytest.fixture(scope="module")
def model(K):
    import math

    import ngp_grad_cases as C
    from nerf_amd import ngp as N
    st = C.prod_state()
    st["sigma_head.bias"] = torch.full((1,), math.log(10.0))  # sigma = 10 exp(noise): crosses the threshold 10
    net = N.InstantNGP(occ_conf={}, scene_box=C.AABB, **C.PROD)
    net.load_reference_state(st)
    return net.to(DEV).eval()


def test_model_bake_texture(K, model, sphere):
    from nerf_amd import Mesh
    from nerf_amd.losses import linear_to_srgb
    mesh = Mesh(sphere["plain"].vertices, sphere["plain"].faces)
    assert model.bake_texture(mesh, texels=6, colors="linear") is mesh
    a = mesh.atlas(6)
    own = a["face"] >= 0
    pts = a["position"][own]
    want = model.vertex_colors(pts, model.normals(pts))
    assert mesh.texels == 6 and tuple(mesh.texture.shape) == (a["T"], a["T"], 3)
    assert torch.equal(mesh.texture[own], want) and bool((mesh.texture[~own] == 0).all())
    srgb = model.bake_texture(Mesh(mesh.vertices, mesh.faces), texels=6)
    assert torch.equal(srgb.texture[own], linear_to_srgb(want))
    with pytest.raises(ValueError):
        model.bake_texture(mesh, colors="fused")

    out = model.extract_mesh(resolution=12, normals=None, texture=6)
    F = out.faces.shape[0]
    assert F > 0 and out.texels == 6 and out.texture.shape[0] == K.atlas_layout(F, 6)[1]
    assert torch.equal(out.vertices, model.extract_mesh(resolution=12, normals=None).vertices)
    own = out.atlas(6)["face"] >= 0
    assert int(own.sum()) == 36 * (F // 2) + 21 * (F % 2) and bool((out.texture[~own] == 0).all())
    with pytest.raises(ValueError):
        model.extract_mesh(resolution=12, texture=4)


def test_model_extract_mesh_tsdf_textured(K, model):
    import math

    from nerf_amd.ray_rendering import fuse_depth_views
    from nerf_amd.scene import hemisphere_poses
    poses = hemisphere_poses(4, seed=0)
    n = 16
    focal = 0.5 * n / math.tan(0.5 * 0.6911112)
    cam = dict(H=n, W=n, fx=focal, fy=focal, cx=n / 2.0, cy=n / 2.0, near=2.0, far=6.0)
    kw = dict(resolution=16, ray_samples=32, batch=3)
    plain = model.extract_mesh_tsdf(poses, **cam, colors="fused", **kw)
    fused = model.extract_mesh_tsdf(poses, **cam, colors="fused", texture=5, **kw)
    F = fused.faces.shape[0]
    assert F > 0 and plain.texture is None and torch.equal(fused.vertices, plain.vertices)
    assert torch.equal(fused.colors, plain.colors) and fused.texels == 5
    # the fused route bakes from the volume, the other from the colour network along the field normals
    vol = fuse_depth_views(model, poses, lo=[-1.5] * 3, hi=[1.5] * 3, colors=True, **cam, **kw)
    a = fused.atlas(5)
    own = a["face"] >= 0
    assert torch.equal(fused.texture[own], vol.sample_colors(a["position"][own])[0])
    assert torch.equal(vol.extract_mesh(normals=None, texture=5).texture, fused.texture)
    net = model.extract_mesh_tsdf(poses, **cam, colors="linear", texture=5, **kw)
    pts = a["position"][own]
    assert torch.equal(net.vertices, plain.vertices)
    assert torch.equal(net.texture[own], model.vertex_colors(pts, model.normals(pts)))
    with pytest.raises(ValueError):
        fuse_depth_views(model, poses, lo=[-1.5] * 3, hi=[1.5] * 3, **cam, **kw).extract_mesh(texture=5)
    with pytest.raises(ValueError):
        model.extract_mesh_tsdf(poses, **cam, texture=3, **kw)


def test_tsdf_volume_bake_texture(K, sphere):
    from nerf_amd import Mesh, TSDFVolume
    vol = TSDFVolume([-1.25] * 3, [1.25] * 3, 12, color=True)
    g = torch.Generator().manual_seed(3)
    vol.color.copy_(torch.rand(vol.color.shape, generator=g))  # r, g, b and a positive colour weight everywhere
    mesh = Mesh(sphere["plain"].vertices, sphere["plain"].faces)
    assert vol.bake_texture(mesh, texels=5) is mesh
    a = mesh.atlas(5)
    own = a["face"] >= 0
    assert torch.equal(mesh.texture[own], vol.sample_colors(a["position"][own])[0])
    assert bool((mesh.texture[~own] == 0).all()) and mesh.texels == 5
    with pytest.raises(ValueError):
        TSDFVolume([-1.25] * 3, [1.25] * 3, 12).bake_texture(mesh)


# ------------------------------------------------------------------ argument errors


def test_argument_errors(K, sphere):
    from nerf_amd import Mesh
    v, f = sphere["plain"].vertices, sphere["plain"].faces
    with pytest.raises(ValueError):
        K.mesh_atlas_texels(v, f, 4)  # S < 5
    with pytest.raises(ValueError):
        K.atlas_layout(2 * 3276 ** 2 + 1, 5)  # T > 16384
    assert K.atlas_layout(2 * 3276 ** 2, 5) == (3276, 16380)
    assert K.atlas_layout(128, 2048) == (8, 16384)  # 128 faces: 8 columns of cells
    with pytest.raises(ValueError):
        K.atlas_layout(128, 2049)
    with pytest.raises(ValueError):
        K.mesh_atlas_texels(v.cpu(), f.cpu(), 8)  # no CPU fallback
    bad = f.clone()
    bad[3, 1] = v.shape[0]
    with pytest.raises(ValueError):
        K.mesh_atlas_texels(v, bad, 8)
    face = torch.zeros(4, dtype=torch.int32, device=DEV)
    bary = torch.zeros((4, 2), device=DEV)
    tex = torch.zeros((64, 64, 3), device=DEV)  # the atlas of 128 faces at S = 8
    assert tuple(K.mesh_texture_lookup(tex, 8, 128, face, bary).shape) == (4, 3)
    for texture, S in ((torch.zeros((64, 63, 3), device=DEV), 8), (torch.zeros((64, 64, 5), device=DEV), 8),
                       (torch.zeros((64, 64), device=DEV), 8), (torch.zeros((72, 72, 3), device=DEV), 8),
                       (tex, 7), (tex, 16), (tex, 4), (tex.double(), 8)):
        with pytest.raises(ValueError):
            K.mesh_texture_lookup(texture, S, 128, face, bary)
    with pytest.raises(ValueError):
        K.mesh_texture_lookup(tex, 8, 128, face.long(), bary)
    with pytest.raises(ValueError):
        K.mesh_texture_lookup(tex, 8, 128, face, bary[:3])
    with pytest.raises(ValueError):
        K.mesh_texture_lookup(tex, 8, 128, face + 128, bary)  # a face past the end
    with pytest.raises(ValueError):
        Mesh(v, f, texture=tex)  # texture and texels go together
    with pytest.raises(ValueError):
        Mesh(v, f, texture=tex, texels=7)
    with pytest.raises(ValueError):
        sphere["plain"].sample_texture(face, bary)  # no texture
    with pytest.raises(ValueError):
        sphere["plain"].bake_texture(lambda p, n: p[:5], 8)  # a colour function of the wrong shape
    assert sphere["plain"].texture is None
