"""Reference for the mesh clean-up (a helper, not a test file): connected components of an indexed triangle list, face
counts, component filtering and order-preserving compaction, restated in numpy with a plain serial union-find
(DESIGN §3.11.1), plus the synthetic triangle lists the tests share.

The rules.  Two vertices are connected iff a chain of faces joins them.  labels[v] = the smallest vertex index of v's
component (an unused vertex is its own component); face_count[l] = the number of faces whose component has label l, 0
where l is no label.  filter_components: every component with face_count >= min_faces, or the keep_largest components
with the most faces, a tie going to the smaller label.  compact: the kept faces stay in their order, the vertices a kept
face uses stay in their order and are renumbered densely, the faces are rewritten to the new numbers, and every
per-vertex attribute is gathered like the vertices.
"""
import functools

import numpy as np

import mesh_reference as R


def component_labels(faces, n_vertices):
    """(V,) int32: the smallest vertex index of every vertex's component.  Serial union-find, smaller root wins."""
    parent = list(range(int(n_vertices)))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    for a, b, c in np.asarray(faces, np.int64).reshape(-1, 3).tolist():
        for x, y in ((a, b), (b, c)):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
    return np.array([find(v) for v in range(int(n_vertices))], np.int32).reshape(-1)


def face_counts(faces, labels):
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    out = np.zeros(len(labels), np.int32)
    if len(faces):
        np.add.at(out, np.asarray(labels)[faces[:, 0]], 1)
    return out


def kept_labels(labels, counts, min_faces=None, keep_largest=None):
    """The labels of the components that the filter keeps, ascending."""
    if (min_faces is None) == (keep_largest is None):
        raise ValueError("give exactly one of min_faces and keep_largest")
    labs = np.unique(np.asarray(labels))  # ascending
    if min_faces is not None:
        return labs[counts[labs] >= min_faces]
    order = np.argsort(-counts[labs].astype(np.int64), kind="stable")  # descending, a tie to the smaller label
    return np.sort(labs[order[:keep_largest]])


def filter_components(faces, n_vertices, min_faces=None, keep_largest=None):
    """(F,) bool: the faces of the kept components."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    labels = component_labels(faces, n_vertices)
    kept = kept_labels(labels, face_counts(faces, labels), min_faces, keep_largest)
    return np.isin(labels[faces[:, 0]], kept) if len(faces) else np.zeros(0, bool)


def compact(vertices, faces, keep_face, attrs=()):
    """(vertices, faces, [attrs...]) of the kept faces, by the order-preserving renumbering rule."""
    faces = np.asarray(faces).reshape(-1, 3)
    keep_face = np.asarray(keep_face).astype(bool)
    kf = faces[keep_face]
    used = np.zeros(len(vertices), bool)
    used[kf.reshape(-1)] = True
    new = np.cumsum(used) - 1
    return (np.asarray(vertices)[used], new[kf].astype(np.int32).reshape(-1, 3),
            [np.asarray(a)[used] for a in attrs])


# ------------------------------------------------------------------ extracted meshes (computed once per process)


BOX_LO, BOX_HI = (-1.0, -0.5, 0.25), (1.5, 0.75, 2.0)  # the box of tests/test_gpu_mesh.py
SPHERES_LO, SPHERES_HI, SPHERES_SHAPE = (-1.6, -0.8, -0.8), (1.6, 0.8, 0.8), (20, 11, 11)


@functools.lru_cache(maxsize=None)
def two_spheres_mesh():
    """(vertices, faces, normals) of two spheres, radii 0.5 and 0.3 at (-0.9,0,0) and (+0.9,0,0): two closed
    components of different size."""
    field = np.maximum(R.sphere_field(SPHERES_SHAPE, SPHERES_LO, SPHERES_HI, 0.5, (-0.9, 0.0, 0.0)),
                       R.sphere_field(SPHERES_SHAPE, SPHERES_LO, SPHERES_HI, 0.3, (0.9, 0.0, 0.0)))
    return R.marching_tets(field, 0.0, SPHERES_LO, SPHERES_HI, normals=True)


@functools.lru_cache(maxsize=None)
def noise_mesh():
    """(vertices, faces, normals) of a noise lattice at a high threshold: many small components, many open at the box,
    several of equal size."""
    return R.marching_tets(R.noise_field((17, 16, 9), seed=18), 0.7, BOX_LO, BOX_HI, normals=True)


# ------------------------------------------------------------------ synthetic triangle lists


STRIP_F = (1, 63, 64, 65, 255, 256, 257, 2049)  # across the wave (64), the workgroup (256) and the scan tile (2048)


def strip(n_faces, numbering="identity", seed=0):
    """Triangle i = (i, i+1, i+2) over n_faces + 2 vertices, renumbered: one component, and the deepest tree a
    union-find can meet (reversed indices hang every union on the far end).  Returns (faces int32, V)."""
    V = n_faces + 2
    i = np.arange(n_faces, dtype=np.int64)
    f = np.stack([i, i + 1, i + 2], 1)
    if numbering == "reversed":
        f = V - 1 - f
    elif numbering == "random":
        f = np.random.default_rng(seed).permutation(V)[f]
    elif numbering != "identity":
        raise ValueError(numbering)
    return np.ascontiguousarray(f, np.int32), V


def interleaved_strips(n_faces=130):
    """Two strips over the even and the odd vertices of one index range, with 5 unused vertices: two at the start, one
    in the middle, two at the end.  Returns (faces int32, V)."""
    i = np.arange(n_faces, dtype=np.int64)
    even = np.stack([2 * i, 2 * i + 2, 2 * i + 4], 1)
    both = np.concatenate([even, even + 1], 0)
    n_used = 2 * n_faces + 4
    mid = n_used // 2
    both = np.where(both >= mid, both + 1, both) + 2  # a hole at `mid`, two unused in front
    order = np.random.default_rng(3).permutation(len(both))  # the two strips' faces mixed
    return np.ascontiguousarray(both[order], np.int32), n_used + 5


def duplicated(faces):
    return np.ascontiguousarray(np.concatenate([faces, faces[::-1]], 0), np.int32)


def with_degenerate_faces(faces, n_vertices):
    """The list plus (a,a,b) faces (one joining two vertices that nothing else joins is left out: a and b are taken
    from one existing face) and (a,a,a) faces."""
    f = np.asarray(faces, np.int64)
    a, b = f[::7, 0], f[::7, 2]
    extra = np.concatenate([np.stack([a, a, b], 1), np.stack([b, b, b], 1),
                            np.array([[n_vertices - 1] * 3], np.int64)], 0)
    return np.ascontiguousarray(np.concatenate([f[: len(f) // 2], extra, f[len(f) // 2:]], 0), np.int32)


def bridged_strips(n_faces=130):
    """The interleaved strips plus one (a,a,b) face with a on the even and b on the odd strip: the repeated index
    still joins the two, so one component with faces remains."""
    f, V = interleaved_strips(n_faces)
    a, b = 2, 3  # the first even and the first odd vertex behind the two unused ones
    assert (f == a).any() and (f == b).any()
    return np.ascontiguousarray(np.concatenate([f, np.array([[a, a, b]], np.int32)], 0), np.int32), V


@functools.lru_cache(maxsize=None)
def synthetic_lists():
    """name -> (faces, V): every synthetic input of the tests."""
    out = {}
    for n in STRIP_F:
        for numbering in ("identity", "reversed", "random"):
            out[f"strip{n}-{numbering}"] = strip(n, numbering, seed=n)
    out["interleaved"] = interleaved_strips()
    out["bridged"] = bridged_strips()
    f, V = strip(257, "random", seed=5)
    out["duplicated"] = (duplicated(f), V)
    g, W = interleaved_strips(90)
    out["degenerate"] = (with_degenerate_faces(g, W), W)
    return out
