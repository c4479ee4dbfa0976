"""The texture atlas's contract on the CPU (-m "not gpu"): properties of tests/mesh_texture_reference.py, the numpy
restatement that the GPU tests compare the kernels with bit for bit.

  footprint   for points of a face's UV triangle (random, the corners, the edge midpoints) every texel of the bilinear
              footprint that carries weight lies in the face's own half cell, off the diagonal: i + j <= S - 2 for an
              even face, i + j >= S for an odd one, and inside the cell; S = 5..19
  partition   every texel of a cell with both faces present has exactly one owner, and the owners' half cells are what
              the footprint property names
  layout      cols and T for F in {0, 1, 2, 3, 8, 9, 10}; the limits
  winding     the UV corners of both parities turn the same way
  inverse     inside the UV triangle a texel's barycentric pair inverts the corner mix
  quality     the 128-face sphere with the colour 0.5 + 0.5 sin(6 p + (0,1,2)) at 20 000 seeded samples: the S = 16
              texture's mean absolute error is below a tenth of the vertex-colour mix's, the S = 8 texture's below it
"""
import numpy as np
import pytest

import mesh_texture_reference as R

F32 = np.float32


def _triangle_points(rng, n):
    """(n + 6, 2) float32 pairs (u, v): random interior points, the corners and the edge midpoints."""
    face, bary = R.surface_samples(1, n, int(rng.integers(1 << 30)))
    special = np.array([[0, 0], [1, 0], [0, 1], [0.5, 0], [0, 0.5], [0.5, 0.5]], F32)
    return np.concatenate([bary, special])


@pytest.mark.parametrize("S", range(5, 20))
def test_footprint_stays_in_the_faces_half_cell(S):
    rng = np.random.default_rng(S)
    bary = _triangle_points(rng, 20000)
    F = 6  # cols = 2: the cells 0..2, so that leaving a cell would show
    for f in range(F):
        face = np.full(bary.shape[0], f, np.int32)
        ix0, ix1, iy0, iy1, fx, fy = R.footprint(F, S, face, bary)
        cols, T = R.layout(F, S)
        ox, oy = S * ((f // 2) % cols), S * ((f // 2) // cols)
        for ix, iy, w in ((ix0, iy0, (1 - fx) * (1 - fy)), (ix1, iy0, fx * (1 - fy)), (ix0, iy1, (1 - fx) * fy),
                          (ix1, iy1, fx * fy)):
            used = w != 0
            i, j = ix[used] - ox, iy[used] - oy
            assert i.min() >= 0 and j.min() >= 0 and i.max() <= S - 1 and j.max() <= S - 1
            if f & 1:
                assert (i + j).min() >= S
            else:
                assert (i + j).max() <= S - 2
        assert (R.owner(F, S)[iy0, ix0] == f).all()  # the texel of full weight at fx = fy = 0 is the face's own


@pytest.mark.parametrize("S", [5, 6, 8, 13])
def test_every_texel_of_a_full_cell_has_one_owner(S):
    F = 8
    own = R.owner(F, S)
    cols, T = R.layout(F, S)
    assert own.shape == (T, T) and own.min() >= 0
    for c in range(F // 2):
        cell = own[S * (c // cols):S * (c // cols + 1), S * (c % cols):S * (c % cols + 1)]
        j, i = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
        assert np.array_equal(cell, np.where(i + j < S, 2 * c, 2 * c + 1))
    # an odd face count: the last cell's odd half and the unused cells belong to nobody
    own7 = R.owner(7, S)
    assert np.array_equal(own7 >= 0, own != 7)
    assert (R.owner(0, S) == -1).all() and R.owner(0, S).shape == (S, S)


@pytest.mark.parametrize("F,cols", [(0, 1), (1, 1), (2, 1), (3, 2), (8, 2), (9, 3), (10, 3)])
def test_layout(F, cols):
    for S in (5, 7, 16):
        assert R.layout(F, S) == (cols, cols * S)
    uv = R.atlas_uv(F, 7)
    assert uv.shape == (F, 3, 2) and (uv == np.rint(uv)).all()
    for f in range(F):
        c = f // 2
        assert np.array_equal(uv[f] - np.array([7 * (c % cols), 7 * (c // cols)], F32), R.local_corners(7, f & 1))


def test_layout_limits():
    with pytest.raises(ValueError):
        R.layout(4, 4)
    assert R.layout(2 * 3276 ** 2, 5) == (3276, 16380)
    with pytest.raises(ValueError):
        R.layout(2 * 3276 ** 2 + 1, 5)
    import math
    for cells in (10 ** 12, 10 ** 12 + 1, (10 ** 6 + 1) ** 2 - 1):
        cols = math.isqrt(cells - 1) + 1
        assert cols * cols >= cells and (cols - 1) * (cols - 1) < cells


def test_corner_winding_is_the_same_for_both_parities():
    for S in (5, 8, 19):
        signs = []
        for odd in (False, True):
            p = R.local_corners(S, odd).astype(np.float64)
            a, b = p[1] - p[0], p[2] - p[0]
            signs.append(np.sign(a[0] * b[1] - a[1] * b[0]))
        assert signs[0] == signs[1] != 0


@pytest.mark.parametrize("S", [5, 6, 9, 16])
def test_texel_bary_inverts_the_corner_mix_inside_the_triangle(S):
    j, i = (g.reshape(-1) for g in np.meshgrid(np.arange(S), np.arange(S), indexing="ij"))
    for odd in (False, True):
        sel = (i + j >= S) if odd else (i + j < S)
        b0, b1, b2 = R.texel_bary(S, i[sel], j[sel], np.full(int(sel.sum()), odd))
        assert (b0 >= 0).all() and (b1 >= 0).all() and (b2 >= 0).all()
        assert np.abs(b0 + b1 + b2 - 1).max() <= 2e-7
        x, y = R.face_uv(S, np.full(b1.shape, int(odd), np.int64), np.stack([b1, b2], 1))
        xc, yc = i[sel] + 0.5, j[sel] + 0.5
        rel = (S - xc, S - yc) if odd else (xc, yc)  # the texel's centre as the even face would see it
        inside = (rel[0] >= 1) & (rel[1] >= 1) & (rel[0] + rel[1] <= S - 2)
        assert inside.any() or S == 5
        assert np.abs(x[inside] - xc[inside]).max(initial=0) <= 1e-5 * S
        assert np.abs(y[inside] - yc[inside]).max(initial=0) <= 1e-5 * S


@pytest.fixture(scope="module")
def sphere_errors():
    v, f = R.octasphere(2)
    assert f.shape == (128, 3)
    face, bary = R.surface_samples(128, 20000, seed=7)
    truth = R.analytic_color(R.surface_points(v, f, face, bary)).astype(np.float64)
    err = {"vertex": np.abs(R.vertex_color_mix(R.analytic_color(v), f, face, bary) - truth).mean()}
    for S in (8, 16):
        tex = R.bake(v, f, S, R.analytic_color)
        err[S] = np.abs(R.texture_lookup(tex, S, 128, face, bary).astype(np.float64) - truth).mean()
    return err


def test_texture_beats_vertex_colours_on_the_sphere(sphere_errors):
    e = sphere_errors
    print(f"mean abs error: vertex mix {e['vertex']:.3e}, S=16 {e[16]:.3e}, S=8 {e[8]:.3e}")
    assert e[16] < 0.1 * e["vertex"]
    assert e[8] < e["vertex"]
