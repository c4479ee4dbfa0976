"""kernels.mesh_ray_cast (csrc/mesh_raycast.hip), mesh_metrics.ray_cast_mesh, Mesh.ray_cast and Mesh.render on the
device (-m gpu), against the numpy restatement of the contract in tests/mesh_raycast_reference.py.

t (float64), face and bary (fp32) are exact: bitwise equal to the reference's brute force over all faces.  Every ray
set has a few hundred to a thousand rays, every mesh at most 1388 faces, and every reference is computed once per
process.

The grids are those of the distance tests: one cell, the default, and the cap, 1024 cells per axis for tiny_face
(2^18 + 1 keys; a ray that crosses the box walks up to 1024 layers of at most 9 cells) and 32 per axis for soup60 and
spheres (soup60 has 1.4e9 keys at 1024)."""
import numpy as np
import pytest
import torch

import mesh_raycast_reference as R
import mesh_smooth_reference as MS

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAMES = ("soup60", "tiny_face", "spheres")
GRIDS = ("one_cell", "default", "cap")
INF = float("inf")


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from nerf_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def MM(K):
    from nerf_amd import mesh_metrics
    return mesh_metrics


@pytest.fixture(scope="module")
def Mesh(K):
    from nerf_amd import Mesh
    return Mesh


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(got, ref):
    """(t, face, bary) of the device against the reference's, bit for bit"""
    assert len(got) == 3
    for g, r, dtype in zip(got, ref, (torch.float64, torch.int32, torch.float32)):
        assert g.dtype == dtype and tuple(g.shape) == tuple(r.shape)
        assert g.cpu().numpy().tobytes() == np.ascontiguousarray(r).tobytes()


def _share(ref):
    return float((ref[1] >= 0).mean())


# ------------------------------------------------------------------ the hit test


def test_table_on_one_triangle(Mesh, MM):
    v, f = R.TRIANGLE
    mesh = Mesh(_dev(v), _dev(f))
    rays = R.table_rays()
    for cull in (False, True):
        rows = [i for i, row in enumerate(R.TABLE) if row[1] == cull]
        got = mesh.ray_cast(_dev(rays[rows]), cull_backfaces=cull)
        _same(got, R.ray_cast(v, f, rays[rows], cull))
        for k, i in enumerate(rows):
            want = R.TABLE[i][2]
            row = (float(got[0][k]), int(got[1][k]), *got[2][k].tolist())
            assert row == ((INF, -1, 0.0, 0.0) if want is None else (want[0], 0, want[1], want[2])), (i, row)
        again = MM.ray_cast_mesh(_dev(rays[rows]), mesh, cull_backfaces=cull)
        assert all(torch.equal(a, b) for a, b in zip(again, got))
    import nerf_amd
    assert nerf_amd.ray_cast_mesh is MM.ray_cast_mesh and "ray_cast_mesh" in nerf_amd.__all__


def test_sliver_is_a_miss(Mesh):
    for scale in (1.0, 2.0 ** 10):
        v, f, ray = R.sliver(scale)
        assert R.ray_cast(v, f, ray, box_clause=False)[1][0] == 0  # without the clause: a hit 98 units from the face
        for cell_size in (None, 0.25 * scale):
            _same(Mesh(_dev(v), _dev(f)).ray_cast(_dev(ray), cell_size=cell_size), R.ray_cast(v, f, ray))


# ------------------------------------------------------------------ the walk


@pytest.mark.parametrize("which", GRIDS)
@pytest.mark.parametrize("name", NAMES)
def test_ray_sets_on_three_grids(K, name, which):
    v, f = R.mesh(name)
    vd, fd = _dev(v), _dev(f)
    grid = K.mesh_face_grid(vd, fd, R.grid_cell(name, which))
    print(f"{name} {which}: cell={grid['cell']:.4g} dims={grid['dims']} n_keys={grid['n_keys']}")
    if which != "default":
        assert max(grid["dims"]) == (1 if which == "one_cell" else 1024 if name == "tiny_face" else 32)
    shares = {kind: _share(R.brute(name, kind)) for kind in ("rays", "axis", "inside", "outside", "far")}
    print(" ".join(f"{kind} {100 * s:.1f}%" for kind, s in shares.items()))
    assert 0.25 <= shares["rays"] <= 0.75  # neither outcome can hide
    assert shares["axis"] >= 0.9
    assert shares["outside"] == 0.0
    for kind, rays in (("rays", R.rays(name)), ("axis", R.axis_rays(name)), ("inside", R.inside_rays(name)),
                       ("outside", R.outside_rays(name)), ("far", R.far_rays(name))):
        assert len(rays) == {"rays": 1000, "far": 100}.get(kind, len(rays))
        for cull in (False, True):
            _same(K.mesh_ray_cast(_dev(rays), vd, fd, grid, cull_backfaces=cull), R.brute(name, kind, cull))
    ref_grid = {"lo": np.asarray(grid["lo"], np.float32), "cell": np.float32(grid["cell"]), "dims": grid["dims"]}
    plane = R.plane_rays(name, ref_grid)
    exact = plane[:, :3] == np.float32(grid["lo"]) + np.round((plane[:, :3] - np.float32(grid["lo"])) / np.float32(
        grid["cell"])).astype(np.float32) * np.float32(grid["cell"])
    assert ((exact & (plane[:, 3:6] == 0)).sum(1) >= 1).all()  # on a plane lo + k cell, and running along it
    second = R.second_hit_rays(name)
    for rays in (plane, second):
        for cull in (False, True):
            _same(K.mesh_ray_cast(_dev(rays), vd, fd, grid, cull_backfaces=cull), R.ray_cast(v, f, rays, cull))


@pytest.mark.parametrize("name", ("soup60", "spheres"))
def test_near_past_the_first_hit_returns_the_second_face(Mesh, name):
    v, f = R.mesh(name)
    first, rays = R.brute(name), R.second_hit_rays(name)
    want = R.ray_cast(v, f, rays)
    was = first[1] >= 0
    assert (want[0][was] > first[0][was]).all() and (want[1][was] != first[1][was]).all()
    assert int((want[1][was] >= 0).sum()) >= 100
    _same(Mesh(_dev(v), _dev(f)).ray_cast(_dev(rays)), want)


def test_far_less_than_near_and_infinite_bounds(Mesh):
    v, f = R.mesh("spheres")
    rays = R.rays("spheres")[:300].copy()
    rays[:100, 6], rays[:100, 7] = 3.0, 1.0  # far < near: a miss
    rays[100:200, 6], rays[100:200, 7] = -INF, INF  # the whole line: hits behind the origin count
    rays[200:, 6], rays[200:, 7] = INF, INF
    want = R.ray_cast(v, f, rays)
    assert (want[1][:100] == -1).all() and (want[0][100:200] < 0).any() and (want[1][200:] == -1).all()
    _same(Mesh(_dev(v), _dev(f)).ray_cast(_dev(rays)), want)


def test_ties_take_the_smaller_face(Mesh):
    v, f = R.mesh("soup60")
    twice = np.concatenate([f, f[::-1]])  # face 60 + k is face 59 - k again: every hit is a tie
    rays = R.rays("soup60")[:400]
    for cull in (False, True):
        got = Mesh(_dev(v), _dev(twice)).ray_cast(_dev(rays), cull_backfaces=cull)
        _same(got, R.ray_cast(v, twice, rays, cull))
        assert int(got[1].max()) < 60 and torch.equal(got[0], _dev(R.brute("soup60", "rays", cull)[0][:400]))


# ------------------------------------------------------------------ sizes, reuse, empties


@pytest.mark.parametrize("n", (0, 1, 255, 256, 257))
def test_block_edges(Mesh, n):
    v, f = R.mesh("soup60")
    got = Mesh(_dev(v), _dev(f)).ray_cast(_dev(R.rays("soup60")[:n]))
    _same(got, tuple(r[:n] for r in R.brute("soup60")))
    assert tuple(got[2].shape) == (n, 2)


def test_no_faces(K, Mesh):
    v, _ = R.mesh("soup60")
    rays = _dev(R.rays("soup60")[:70])
    none = Mesh(_dev(v), torch.empty((0, 3), dtype=torch.int32, device=DEV))
    for got in (none.ray_cast(rays), K.mesh_ray_cast(rays, none.vertices, none.faces,
                                                     K.mesh_face_grid(none.vertices, none.faces))):
        _same(got, R.ray_cast(v, np.zeros((0, 3), np.int32), R.rays("soup60")[:70]))
        assert bool(torch.isinf(got[0]).all()) and bool((got[1] == -1).all()) and not bool(got[2].any())
    image = none.render(*R.camera("soup60")[:6], _dev(R.camera("soup60")[6]))
    assert not bool(image["mask"].any()) and bool(torch.isinf(image["depth"]).all()) and not bool(image["normal"].any())


def test_a_grid_built_once_gives_the_same_bits(K, MM, Mesh):
    v, f = R.mesh("spheres")
    mesh = Mesh(_dev(v), _dev(f))
    grid = K.mesh_face_grid(mesh.vertices, mesh.faces)
    keys = grid["keys"].clone()
    first = mesh.ray_cast(_dev(R.rays("spheres")))
    for kind, rays in (("rays", R.rays("spheres")), ("axis", R.axis_rays("spheres")), ("rays", R.rays("spheres"))):
        got = MM.ray_cast_mesh(_dev(rays), mesh, grid=grid)
        _same(got, R.brute("spheres", kind))
        assert all(torch.equal(a, b) for a, b in zip(got, mesh.ray_cast(_dev(rays), grid=grid)))
    assert all(torch.equal(a, b) for a, b in zip(first, got)) and torch.equal(grid["keys"], keys)


# ------------------------------------------------------------------ arguments


def test_arguments(K, MM, Mesh):
    v, f = R.mesh("soup60")
    vd, fd, rd = _dev(v), _dev(f), _dev(R.rays("soup60")[:65])
    mesh = Mesh(vd, fd)
    grid = K.mesh_face_grid(vd, fd)

    def changed(row, col, value):
        bad = rd.clone()
        bad[row, col] = value
        return bad

    zero_d = rd.clone()
    zero_d[7, 3:6] = 0.0
    wide = torch.zeros((65, 16), dtype=torch.float32, device=DEV)
    bad_rays = (rd.cpu(), rd.double(), wide[:, ::2], rd.reshape(-1), rd[:, :6].contiguous(), rd[:, :3].contiguous(),
                changed(5, 2, INF), changed(5, 1, float("nan")), changed(9, 4, -INF), changed(9, 3, float("nan")), zero_d,
                changed(11, 6, float("nan")), changed(11, 7, float("nan")))
    for bad in bad_rays:
        with pytest.raises(ValueError):
            MM.ray_cast_mesh(bad, mesh)
        with pytest.raises(ValueError):
            mesh.ray_cast(bad, grid=grid)
        with pytest.raises(ValueError):
            K.mesh_ray_cast(bad, vd, fd, grid)
    for good in (changed(3, 6, -INF), changed(3, 7, INF), changed(3, 7, -INF)):  # +-inf in near / far is allowed
        K.mesh_ray_cast(good, vd, fd, grid)
    nan_v = vd.clone()
    nan_v[3, 1] = float("nan")
    inf_v = vd.clone()
    inf_v[4, 0] = INF
    for bad in (Mesh(vd.cpu(), fd.cpu()), Mesh(vd.double(), fd), Mesh(vd, fd.long()), Mesh(nan_v, fd), Mesh(inf_v, fd),
                Mesh(vd[:20].contiguous(), fd)):  # the last: indices out of range
        with pytest.raises(ValueError):
            bad.ray_cast(rd)
        with pytest.raises(ValueError):
            K.mesh_ray_cast(rd, bad.vertices, bad.faces, grid)
    for bad_cell in (0.0, -1.0, float("nan"), INF, 1e-4, "x"):  # 1e-4: about 20000 cells along an axis
        with pytest.raises(ValueError):
            mesh.ray_cast(rd, cell_size=bad_cell)
    for bad_grid in ({"keys": None}, None, K.points_grid(vd), {**grid, "F": 59}, {**grid, "keys": grid["keys"][:-1]},
                     {**grid, "keys": grid["keys"].cpu()}, {**grid, "keys": grid["keys"].to(torch.int32)}):
        if bad_grid is not None:
            with pytest.raises(ValueError):
                mesh.ray_cast(rd, grid=bad_grid)
        with pytest.raises(ValueError):
            K.mesh_ray_cast(rd, vd, fd, bad_grid)
    # a cell below 2^-20 of the largest |coordinate|: two small faces far from the origin of the coordinates
    far_v = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 1]], np.float32) * np.float32(2.0 ** -8)
             + np.float32(2.0 ** 14)).astype(np.float32)
    far_f = np.array([[0, 1, 2], [1, 2, 3]], np.int32)
    fine = K.mesh_face_grid(_dev(far_v), _dev(far_f), 2.0 ** -8)  # 2^-22 of 2^14
    with pytest.raises(ValueError, match="2\\^-20"):
        K.mesh_ray_cast(rd, _dev(far_v), _dev(far_f), fine)
    coarse = K.mesh_face_grid(_dev(far_v), _dev(far_f), 2.0 ** -5)  # 2^-19 of it: allowed
    aimed = R.pack([[2.0 ** 14, 2.0 ** 14, 2.0 ** 14 + 1]], [[2.0 ** -10, 2.0 ** -10, -1]])
    _same(K.mesh_ray_cast(_dev(aimed), _dev(far_v), _dev(far_f), coarse), R.ray_cast(far_v, far_f, aimed))
    with pytest.raises(ValueError):
        mesh.render(12, 16, 14.0, 14.0, 8.0, 6.0, R.camera("soup60")[6])  # c2w: a tensor
    with pytest.raises(ValueError):
        mesh.render(0, 16, 14.0, 14.0, 8.0, 6.0, _dev(R.camera("soup60")[6]))


# ------------------------------------------------------------------ Mesh.render


@pytest.mark.parametrize("attributes", (True, False))
@pytest.mark.parametrize("name", ("octahedron", "spheres"))
def test_render(K, Mesh, name, attributes):
    from nerf_amd.ray_sampling import rays_for_camera
    v, f = R.mesh(name)
    H, W, fx, fy, cx, cy, c2w = R.camera(name)
    assert (H, W) == (12, 16)
    normals = np.ascontiguousarray(MS.compute_normals(v, f), np.float32) if attributes else None
    colors = np.random.default_rng(4).uniform(0, 1, v.shape).astype(np.float32) if attributes else None
    mesh = Mesh(_dev(v), _dev(f), None if normals is None else _dev(normals), None if colors is None else _dev(colors))
    out = mesh.render(H, W, fx, fy, cx, cy, _dev(c2w), cull_backfaces=True)
    assert set(out) == {"depth", "mask", "face", "normal"} | ({"color"} if attributes else set())
    rays = rays_for_camera(H, W, fx, fy, cx, cy, _dev(c2w), near=0.0, far=INF)
    assert tuple(rays.shape) == (H * W, 8)
    want = R.ray_cast(v, f, rays.cpu().numpy(), cull=True)
    share = _share(want)
    print(f"{name}: {100 * share:.1f}% of the pixels hit")
    assert 0.1 <= share <= 0.9
    t, face, bary = mesh.ray_cast(rays, cull_backfaces=True)
    _same((t, face, bary), want)
    assert out["depth"].dtype == torch.float32 and tuple(out["depth"].shape) == (H, W)
    assert torch.equal(out["depth"].reshape(-1), t.to(torch.float32))
    assert out["mask"].dtype == torch.bool and torch.equal(out["mask"].reshape(-1), face >= 0)
    assert out["face"].dtype == torch.int32 and torch.equal(out["face"].reshape(-1), face)
    hit = (face >= 0).cpu().numpy()
    depth = out["depth"].cpu().numpy().reshape(-1)
    assert np.isinf(depth[~hit]).all() and (depth[~hit] > 0).all() and np.isfinite(depth[hit]).all()
    normal = out["normal"].cpu().numpy().reshape(-1, 3).astype(np.float64)
    assert out["normal"].dtype == torch.float32 and tuple(out["normal"].shape) == (H, W, 3)
    assert (np.abs(np.linalg.norm(normal[hit], axis=1) - 1) <= 1e-6).all() and not normal[~hit].any()
    corners = f[want[1][hit]]
    if not attributes:
        flat = R.D.unit_face_normals(v, f)[want[1][hit]]
        assert np.abs(normal[hit] - flat).max() <= 1e-6
        d = rays[:, 3:6].cpu().numpy().astype(np.float64)
        assert ((normal[hit] * d[hit]).sum(1) < 0).all()  # culled to front hits: the winding normal faces the camera
    else:
        color = out["color"].cpu().numpy().reshape(-1, 3)
        assert out["color"].dtype == torch.float32 and tuple(out["color"].shape) == (H, W, 3)
        c = colors[corners]  # (hits, 3 corners, 3 channels)
        assert (color[hit] >= c.min(1)).all() and (color[hit] <= c.max(1)).all() and not color[~hit].any()
        w = np.stack([1 - want[2][hit, 0].astype(np.float64) - want[2][hit, 1], want[2][hit, 0], want[2][hit, 1]], 1)
        assert np.abs(color[hit] - np.einsum("nk,nkc->nc", w, c.astype(np.float64))).max() <= 1e-6
        mixed = np.einsum("nk,nkc->nc", w, normals[corners].astype(np.float64))
        mixed /= np.linalg.norm(mixed, axis=1, keepdims=True)
        assert np.abs(normal[hit] - mixed).max() <= 1e-6
    again = mesh.render(H, W, fx, fy, cx, cy, _dev(c2w), cull_backfaces=True, grid=K.mesh_face_grid(mesh.vertices, mesh.faces))
    assert all(torch.equal(out[k], again[k]) for k in out)
