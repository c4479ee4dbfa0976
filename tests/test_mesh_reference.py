"""The mesh extractor's yardsticks on the numpy reference alone (tests/mesh_reference.py), and the PLY / OBJ writers,
without a GPU: known answers as properties (closedness, Euler characteristic, radius, volume, plane), every
(tetrahedron, sign case) pair on a single cell, and a file round trip."""
import itertools

import numpy as np
import pytest
import torch

import mesh_reference as R

LO, HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)


@pytest.fixture(scope="module")
def sphere():
    shape = (14, 13, 12)
    v, f = R.marching_tets(R.sphere_field(shape, LO, HI), 0.0, LO, HI)
    return shape, v, f


def test_sphere_closed_oriented(sphere):
    _, v, f = sphere
    assert len(v) > 0 and len(f) > 0
    assert all(k == 2 for k in R.undirected_edge_counts(f).values())
    assert all(k == 1 for k in R.directed_edge_counts(f).values())
    assert R.euler_characteristic(len(v), f) == 2
    assert R.signed_volume(v, f) > 0


def test_sphere_radius_and_volume(sphere):
    """Linear interpolation of a distance field along an edge of length |h| misses the radius by at most
    |h|^2 / (8 (r0 - |h|)) (0.034 on this lattice; the reference measures 0.0151, and 0.961 of the ball's volume)."""
    shape, v, f = sphere
    h = R.spacing(shape, LO, HI).astype(np.float64)
    hh = float(np.sum(h * h))
    bound = hh / (8.0 * (0.6 - np.sqrt(hh)))
    err = np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - 0.6).max()
    assert err <= bound, (err, bound)
    ball = 4.0 / 3.0 * np.pi * 0.6 ** 3
    ratio = R.signed_volume(v, f) / ball
    # a point x = sum l_i v_i of a triangle has |x|^2 = sum l_i |v_i|^2 - sum_{i<j} l_i l_j |v_i - v_j|^2
    # >= r_min^2 - |h|^2 / 3 (vertices of one tetrahedron are at most |h| apart), and |x| <= r_max: the closed
    # surface lies between two spheres about the centre it encloses (0.73 .. 1.18 here)
    r_in = np.sqrt((0.6 - bound) ** 2 - hh / 3.0)
    assert (r_in / 0.6) ** 3 <= ratio <= ((0.6 + bound) / 0.6) ** 3, ratio


def test_torus_euler_zero():
    shape = (16, 16, 10)
    v, f = R.marching_tets(R.torus_field(shape, LO, HI), 0.0, LO, HI)
    assert R.is_closed(f)
    assert R.euler_characteristic(len(v), f) == 0


def test_noise_with_outside_border_is_closed():
    v, f = R.marching_tets(R.noise_field((8, 7, 6), 3, border_outside=True), 0.0, LO, HI)
    assert len(f) > 100
    assert R.is_closed(f)


def test_integer_field_iso_on_lattice_values():
    """Lattice values equal to iso are outside (t = 1 on their edges): zero-area triangles may appear, connectivity
    stays closed and positions finite."""
    v, f = R.marching_tets(R.integer_field((8, 7, 6), 4), 0.0, LO, HI)
    assert len(f) > 100
    assert np.isfinite(v).all()
    assert R.is_closed(f)


def test_plane():
    shape = (6, 5, 7)
    z0 = np.float32(0.13)
    field = (0.13 - R.lattice_points(shape, LO, HI)[..., 2]).astype(np.float32)
    v, f = R.marching_tets(field, 0.0, LO, HI)
    assert np.abs(v[:, 2] - z0).max() <= 2 * np.spacing(z0)
    assert abs(R.area(v, f) - 4.0) <= 1e-5 * 4.0
    n = R.face_normals(v, f)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    assert np.abs(n - np.array([0.0, 0.0, 1.0])).max() < 1e-6


@pytest.mark.parametrize("t,m", list(itertools.product(range(6), range(16))))
def test_every_case_points_outside(t, m):
    """One cell, tetrahedron t's corners set by case m (bit i = corner i inside), the cell's other four corners set
    either way: the triangles of tetrahedron t have their normals on the outside side (towards lower values)."""
    cm = R.tet_corners(t)
    others = [c for c in range(8) if c not in cm]
    for rest in range(16):
        field = np.zeros((2, 2, 2), np.float32)
        vals = {cm[i]: (1.0 if (m >> i) & 1 else -1.0) for i in range(4)}
        vals.update({c: (0.7 if (rest >> k) & 1 else -0.6) for k, c in enumerate(others)})
        for c, val in vals.items():
            field[c & 1, (c >> 1) & 1, (c >> 2) & 1] = val
        v, f = R.marching_tets(field, 0.0, (0, 0, 0), (1, 1, 1))
        # the faces of tetrahedron t: those of the tetrahedra before it come first
        inside = lambda tt: [vals[c] > 0 for c in R.tet_corners(tt)]  # noqa: E731
        first = sum(len(R.case_triangles(inside(tt))) for tt in range(t))
        tris = R.case_triangles(inside(t))
        assert len(tris) == (0 if m in (0, 15) else 2 if bin(m).count("1") == 2 else 1)
        pos = {c: np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], np.float64) for c in cm}
        if not tris:
            continue
        cin = np.mean([pos[cm[i]] for i in range(4) if (m >> i) & 1], axis=0)
        cout = np.mean([pos[cm[i]] for i in range(4) if not (m >> i) & 1], axis=0)
        for k in range(len(tris)):
            a, b, c = (v[j].astype(np.float64) for j in f[first + k])
            assert np.dot(np.cross(b - a, c - a), cout - cin) > 1e-6, (t, m, rest, k)


def _read_ply(path):
    raw = open(path, "rb").read()
    head, payload = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = nf = 0
    props = []
    for ln in lines[2:]:
        w = ln.split()
        if w[:2] == ["element", "vertex"]:
            nv = int(w[2])
        elif w[:2] == ["element", "face"]:
            nf = int(w[2])
        elif w[:2] == ["property", "float"]:
            props.append(w[2])
        elif w and w[0] == "property":
            assert ln == "property list uchar int vertex_indices"
    vb = nv * 4 * len(props)
    vert = np.frombuffer(payload[:vb], "<f4").reshape(nv, len(props))
    rec = np.frombuffer(payload[vb:], np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    assert len(payload) == vb + 13 * nf and len(rec) == nf
    assert (rec["n"] == 3).all()
    return props, vert, rec["v"]


@pytest.mark.parametrize("with_normals", [False, True])
def test_ply_obj_round_trip(tmp_path, sphere, with_normals):
    from nerf_amd.mesh import Mesh
    _, v, f = sphere
    n = (-v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32) if with_normals else None
    mesh = Mesh(torch.from_numpy(v), torch.from_numpy(f), None if n is None else torch.from_numpy(n))
    assert mesh.cpu().vertices.shape == (len(v), 3)

    mesh.save_ply(tmp_path / "m.ply")
    props, pv, pf = _read_ply(tmp_path / "m.ply")
    assert props == ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else [])
    assert np.array_equal(pv[:, :3], v) and np.array_equal(pf, f)
    if with_normals:
        assert np.array_equal(pv[:, 3:], n)

    mesh.save_obj(tmp_path / "m.obj")
    ov, on, of = [], [], []
    for ln in open(tmp_path / "m.obj"):
        w = ln.split()
        if w[0] == "v":
            ov.append([float(x) for x in w[1:]])
        elif w[0] == "vn":
            on.append([float(x) for x in w[1:]])
        elif w[0] == "f":
            idx = [x.split("//") for x in w[1:]]
            assert all(len(set(i)) == 1 and len(i) == (2 if with_normals else 1) for i in idx)
            of.append([int(i[0]) - 1 for i in idx])
    assert np.array_equal(np.array(ov, np.float32), v) and np.array_equal(np.array(of, np.int32), f)
    if with_normals:
        assert np.array_equal(np.array(on, np.float32), n)
    else:
        assert not on


def test_empty_mesh_files(tmp_path):
    from nerf_amd.mesh import Mesh
    mesh = Mesh(torch.empty((0, 3)), torch.empty((0, 3), dtype=torch.int32))
    mesh.save_ply(tmp_path / "e.ply")
    props, pv, pf = _read_ply(tmp_path / "e.ply")
    assert pv.shape == (0, 3) and pf.shape == (0, 3)
    mesh.save_obj(tmp_path / "e.obj")
    assert open(tmp_path / "e.obj").read() == ""
