"""The numpy restatement of the mesh clean-up (tests/mesh_clean_reference.py) against scipy's connected components and
the topology helpers of tests/mesh_reference.py, and the colour columns of the PLY / OBJ writers with host tensors.
No GPU."""
import numpy as np
import pytest
import torch
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import mesh_clean_reference as C
import mesh_reference as R


def _scipy_labels(faces, V):
    """scipy's component numbers canonicalised to the smallest vertex index of each component."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    i = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    j = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    g = coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(V, V))
    n, comp = connected_components(g, directed=False)
    smallest = np.full(n, V, np.int64)
    np.minimum.at(smallest, comp, np.arange(V))
    return n, smallest[comp].astype(np.int32)


def _inputs():
    out = dict(C.synthetic_lists())
    for name, mesh in (("two_spheres", C.two_spheres_mesh()), ("noise", C.noise_mesh())):
        out[name] = (mesh[1], len(mesh[0]))
    out["no_faces"] = (np.zeros((0, 3), np.int32), 7)
    out["nothing"] = (np.zeros((0, 3), np.int32), 0)
    return out


@pytest.mark.parametrize("name", sorted(_inputs()))
def test_labels_agree_with_scipy(name):
    faces, V = _inputs()[name]
    labels = C.component_labels(faces, V)
    n, ref = _scipy_labels(faces, V)
    assert labels.dtype == np.int32 and labels.shape == (V,)
    assert np.array_equal(labels, ref)
    counts = C.face_counts(faces, labels)
    assert counts.sum() == len(faces) and len(np.unique(labels)) == n
    assert (counts[labels != np.arange(V)] == 0).all()
    if name.startswith("strip") or name in ("duplicated", "bridged"):
        assert len(np.unique(labels[np.unique(faces)])) == 1
    if name == "interleaved":
        assert n == 2 + 5 and sorted(counts[counts > 0].tolist()) == [130, 130]
    if name == "no_faces":
        assert np.array_equal(labels, np.arange(7)) and not counts.any()


def test_two_spheres_components():
    v, f, _ = C.two_spheres_mesh()
    labels = C.component_labels(f, len(v))
    counts = C.face_counts(f, labels)
    sizes = sorted(counts[counts > 0].tolist())
    print("two spheres:", sizes)
    assert len(np.unique(labels)) == 2 and len(sizes) == 2 and sizes[0] != sizes[1]


def test_noise_components():
    v, f, _ = C.noise_mesh()
    labels = C.component_labels(f, len(v))
    counts = C.face_counts(f, labels)
    sizes = counts[counts > 0]
    print(f"noise: {len(sizes)} components, {len(np.unique(sizes))} distinct sizes, largest {sizes.max()}")
    assert len(sizes) >= 50 and len(np.unique(sizes)) >= 10


@pytest.mark.parametrize("keep_largest", [1, 2])
def test_compact_keeps_closed_components(keep_largest):
    v, f, n = C.two_spheres_mesh()
    keep = C.filter_components(f, len(v), keep_largest=keep_largest)
    cv, cf, (cn,) = C.compact(v, f, keep, [n])
    assert R.is_closed(cf) and R.euler_characteristic(len(cv), cf) == 2 * keep_largest
    assert R.signed_volume(cv, cf) > 0
    assert sorted(np.unique(cf).tolist()) == list(range(len(cv)))
    # geometry is carried, not recomputed: every kept face has the corners it had
    assert np.array_equal(cv[cf], v[f[keep]]) and np.array_equal(cn[cf], n[f[keep]])
    assert (np.diff(np.flatnonzero(np.isin(np.arange(len(v)), f[keep]))) > 0).all()
    if keep_largest == 1:
        assert keep.sum() == max(C.face_counts(f, C.component_labels(f, len(v))))
    else:
        assert keep.all() and np.array_equal(cv, v) and np.array_equal(cf, f)


def test_filter_ties_go_to_the_smaller_label():
    v, f, _ = C.noise_mesh()
    labels = C.component_labels(f, len(v))
    counts = C.face_counts(f, labels)
    labs = np.unique(labels)
    order = sorted(labs.tolist(), key=lambda l: (-int(counts[l]), l))
    k = next(i for i in range(1, len(order)) if counts[order[i - 1]] == counts[order[i]])  # cut inside a tie
    kept = C.kept_labels(labels, counts, keep_largest=k)
    assert kept.tolist() == sorted(order[:k]) and order[k] not in kept and order[k] > order[k - 1]
    m = int(counts[order[k]])
    assert C.kept_labels(labels, counts, min_faces=m).tolist() == sorted(l for l in order if counts[l] >= m)
    assert len(C.kept_labels(labels, counts, keep_largest=10 ** 6)) == len(labs)
    with pytest.raises(ValueError):
        C.kept_labels(labels, counts)
    with pytest.raises(ValueError):
        C.kept_labels(labels, counts, min_faces=1, keep_largest=1)


# ------------------------------------------------------------------ writers


def _old_ply_bytes(v, f, n):
    """The PLY of a mesh without colours, restated from the format: what the writer produced before it knew colours."""
    props = ["x", "y", "z"] + (["nx", "ny", "nz"] if n is not None else [])
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"] + [f"property float {p}" for p in props]
    head += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    body = (v if n is None else np.concatenate([v, n], 1)).astype("<f4").tobytes()
    faces = b"".join(b"\x03" + row.astype("<i4").tobytes() for row in f)
    return ("\n".join(head) + "\n").encode("ascii") + body + faces


def _old_obj_text(v, f, n):
    out = ["v %.9g %.9g %.9g\n" % tuple(x) for x in v.tolist()]
    if n is not None:
        out += ["vn %.9g %.9g %.9g\n" % tuple(x) for x in n.tolist()]
        out += ["f %d//%d %d//%d %d//%d\n" % (a, a, b, b, c, c) for a, b, c in (f + 1).tolist()]
    else:
        out += ["f %d %d %d\n" % (a, b, c) for a, b, c in (f + 1).tolist()]
    return "".join(out)


def _small_mesh():
    v, f, n = C.two_spheres_mesh()
    keep = C.filter_components(f, len(v), keep_largest=1)
    keep &= np.arange(len(f)) < 40
    v, f, (n,) = C.compact(v, f, keep, [n])
    return v.astype(np.float32), f.astype(np.int32), n.astype(np.float32)


def _read_ply(path):
    raw = open(path, "rb").read()
    head, payload = raw.split(b"end_header\n", 1)
    nv = nf = 0
    floats, uchars = [], []
    for ln in head.decode("ascii").split("\n"):
        w = ln.split()
        if w[:2] == ["element", "vertex"]:
            nv = int(w[2])
        elif w[:2] == ["element", "face"]:
            nf = int(w[2])
        elif w[:2] == ["property", "float"]:
            assert not uchars  # the colours come after every float column
            floats.append(w[2])
        elif w[:2] == ["property", "uchar"]:
            uchars.append(w[2])
    dt = np.dtype([("f", "<f4", (len(floats),)), ("c", "u1", (len(uchars),))])
    vert = np.frombuffer(payload[:nv * dt.itemsize], dt)
    rec = np.frombuffer(payload[nv * dt.itemsize:], np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    assert len(rec) == nf and len(payload) == nv * dt.itemsize + 13 * nf
    return floats, uchars, vert["f"], vert["c"], rec["v"]


@pytest.mark.parametrize("with_normals", [False, True])
def test_colour_round_trip(tmp_path, with_normals):
    from nerf_amd.mesh import Mesh
    v, f, n = _small_mesh()
    n = n if with_normals else None
    c = np.random.default_rng(7).uniform(0.0, 1.0, v.shape).astype(np.float32)
    mesh = Mesh(torch.from_numpy(v), torch.from_numpy(f), None if n is None else torch.from_numpy(n),
                colors=torch.from_numpy(c))
    assert "colors" in repr(mesh) and torch.equal(mesh.cpu().colors, mesh.colors)

    mesh.save_ply(tmp_path / "m.ply")
    floats, uchars, pf, pc, faces = _read_ply(tmp_path / "m.ply")
    assert floats == ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else [])
    assert uchars == ["red", "green", "blue"]
    assert np.array_equal(pf[:, :3], v) and np.array_equal(faces, f)
    if with_normals:
        assert np.array_equal(pf[:, 3:], n)
    assert np.array_equal(pc, np.rint(c.astype(np.float32) * np.float32(255.0)).astype(np.uint8))

    mesh.save_obj(tmp_path / "m.obj")
    ov, on, of = [], [], []
    for ln in open(tmp_path / "m.obj"):
        w = ln.split()
        if w[0] == "v":
            assert len(w) == 7
            ov.append([float(x) for x in w[1:]])
        elif w[0] == "vn":
            on.append([float(x) for x in w[1:]])
        elif w[0] == "f":
            of.append([int(x.split("//")[0]) - 1 for x in w[1:]])
    ov = np.array(ov, np.float32)
    assert np.array_equal(ov[:, :3], v) and np.array_equal(ov[:, 3:], c) and np.array_equal(np.array(of, np.int32), f)
    assert (np.array_equal(np.array(on, np.float32), n) if with_normals else not on)


def test_colour_bytes(tmp_path):
    """round(clamp(c, 0, 1) 255): 0 -> 0, 1 -> 255, 0.5 -> 128 (127.5 rounds to even), below 0 -> 0, above 1 -> 255."""
    from nerf_amd.mesh import Mesh
    vals = [0.0, 1.0, 0.5, -0.25, 1.75, 0.2, 1.0 / 255.0, 254.4 / 255.0]
    want = [0, 255, 128, 0, 255, 51, 1, 254]
    V = len(vals)
    v = torch.zeros((V, 3))
    c = torch.tensor(vals).view(V, 1).repeat(1, 3)
    Mesh(v, torch.zeros((0, 3), dtype=torch.int32), colors=c).save_ply(tmp_path / "c.ply")
    _, uchars, _, pc, _ = _read_ply(tmp_path / "c.ply")
    assert uchars == ["red", "green", "blue"]
    assert pc.tolist() == [[w] * 3 for w in want]


@pytest.mark.parametrize("with_normals", [False, True])
def test_no_colours_writes_the_old_bytes(tmp_path, with_normals):
    from nerf_amd.mesh import Mesh
    v, f, n = _small_mesh()
    n = n if with_normals else None
    old = Mesh(torch.from_numpy(v), torch.from_numpy(f), None if n is None else torch.from_numpy(n))
    new = Mesh(torch.from_numpy(v), torch.from_numpy(f), None if n is None else torch.from_numpy(n), colors=None)
    assert old.colors is None and repr(old) == repr(new) and "colors" not in repr(old)
    for m, stem in ((old, "old"), (new, "new")):
        m.save_ply(tmp_path / f"{stem}.ply")
        m.save_obj(tmp_path / f"{stem}.obj")
        assert open(tmp_path / f"{stem}.ply", "rb").read() == _old_ply_bytes(v, f, n)
        assert open(tmp_path / f"{stem}.obj").read() == _old_obj_text(v, f, n)


def test_colour_shape_is_validated():
    from nerf_amd.mesh import Mesh
    v, f = torch.zeros((4, 3)), torch.zeros((1, 3), dtype=torch.int32)
    with pytest.raises(ValueError):
        Mesh(v, f, colors=torch.zeros((3, 3)))
    with pytest.raises(ValueError):
        Mesh(v, f, colors=torch.zeros((4, 4)))
    with pytest.raises(ValueError):
        Mesh(v, f).filter_components()
    with pytest.raises(ValueError):
        Mesh(v, f).filter_components(min_faces=1, keep_largest=1)
