// Point-in-mesh by exact crossing counts: the faces crossed by the vertical ray q + t e_z, t > 0, from
// a query q, found through the face grid of mesh_grid_core.hpp, written once for the device and for a host
// compiler so that every loop can be run and checked under a host sanitizer without a GPU.
// Build with -ffp-contract=off: every fp64 operation below rounds on its own (two_sum depends on it).
//
// The rule.  q and the corners a, b, c are fp32 values; orient(P, Q, R) is the EXACT sign of
// (Qx - Px)(Ry - Py) - (Qy - Py)(Rx - Px) over the xy coordinates.  Face f is crossed iff
//   1. in fp32 compares, max(az, bz, cz) > qz, qx lies in [min, max] of the corners' x and qy in that of their y;
//   2. s = orient(a, b, c) != 0 (a vertical or degenerate face, one with a repeated index included, is never crossed);
//   3. for the three directed edges U -> V of the projection taken counter-clockwise (a b, b c, c a, with b and c
//      swapped when s < 0), e = orient(U, V, q) > 0, or e == 0 and (Vy < Uy, or Vy == Uy and Vx > Ux);
//   4. in rounded double, e1 = b - a, e2 = c - a, w = q - a, n = e1 x e2 (six products, three differences),
//      g = (nx wx + ny wy) + nz wz: g < 0 and s > 0, or g > 0 and s < 0 (the plane is met at t = -g / nz > 0; no
//      division is made).  b and c are NOT swapped here.
// crossings = the number of crossed faces, winding = the sum of s over them: +1 inside a closed mesh whose normals
// point outwards.
//
// The perturbation.  Rule 3 is the test of q' = q + (eps, eps^2) for an infinitesimal eps > 0 against the closed
// half-plane's boundary: orient(U, V, q') = e + eps (Uy - Vy) + eps^2 (Vx - Ux), whose sign for e == 0 is that of
// Uy - Vy and then of Vx - Ux; both vanish only for U == V, which rule 2 has excluded.  q' lies on no edge and on no
// vertex of any projection, and it is the same point for every face: in the projection of a closed mesh every edge
// is shared by faces whose projections lie on its two sides (or on the same side with opposite s), and q' is in
// exactly those that q + (eps, eps^2) geometrically is in.  Rules 1 to 3 are exact, so parity and winding are
// topologically right for every q that is not within the rounding of rule 4 of a face's plane.  Rule 1's closed
// intervals only pre-empt rule 3: a q outside the box of the projection fails an edge test.
//
// Rule 4 near a plane.  With L the largest |component| of e1 and e2 and W that of w, the computed g differs from
// the real n . w by at most 2^-46 L^2 W: each difference carries one rounding u = 2^-53, each product of n three,
// each n_k 8 u L^2 in all, each term n_k w_k 12 u L^2 W, the three terms and the two sums 48 u L^2 W < 2^-47 L^2 W to
// first order, doubled for the higher orders.  A query farther from the plane than 2^-46 L^2 W / |n| gets the
// geometric answer; a query closer gets the sign of the g computed here and nothing more: a point ON the surface
// is unspecified geometrically, but the answer is a function of the input alone.
//
// Exactness of orient.  Expanded, (Qx - Px)(Ry - Py) - (Qy - Py)(Rx - Px) =
//   Qx Ry - Qx Py - Px Ry - Qy Rx + Qy Px + Py Rx.
// Each term is a product of two fp32 values: 48 significant bits, an exponent within [-298, 256], so it is exact in
// double, and so is its negation.  The filter: sum = ((t0 + t1) + (t2 + t3)) + (t4 + t5) and S = the same sum of the
// |t_i|.  Five roundings give |sum - exact| <= ((1 + u)^3 - 1) S_exact < 4 u S_exact and S >= (1 - 3 u) S_exact, so
// |sum| > 2^-48 S = 32 u S implies |sum - exact| < |sum|: the sign of sum is the exact sign.  Otherwise the terms
// are added one at a time into a Shewchuk expansion (grow-expansion by two_sum; Shewchuk, Adaptive Precision
// Floating-Point Arithmetic and Fast Robust Geometric Predicates, Theorem 10): h0 .. h5 are non-overlapping,
// ascending in magnitude where non-zero, and their sum is the exact sum, whose sign is that of the last non-zero
// h.  |sum| <= 6 2^256 stays far from overflow, and double addition is exact where it would be subnormal, so
// two_sum's error term is exact throughout.  The expansion lives in six named doubles, no indexed array (§3.11.6
// records what indexing by a run-time value did to ray_cast_kernel).
//
// The walk.  (cx, cy, cz) = cell_index of q per axis.  nerf_grid::for_run over the cells (cx, cy, cz .. nz - 1): one
// lower bound at cell_id(cx, cy, cz) << 32, then the keys up to the end of the column (cx, cy): the ray runs along z
// because a column's cells are contiguous in the sorted keys.  A face registered in several cells of the column is
// tested at one key only: the one whose iz == max(cell_index(min corner z), cz).
// Why this finds every crossed face exactly once.  cell_index is monotone in the coordinate (a difference, a
// product, a floor and a clamp, each monotone).  For a crossed face rule 1 gives min x <= qx <= max x, hence
// cell_index(min x) <= cx <= cell_index(max x), and the same in y: the face is registered in the column (cx, cy), in
// the cells lz .. hz of its z index box.  Rule 1 also gives max z > qz, hence hz >= cz.  So m = max(lz, cz) lies in
// [lz, hz] and in [cz, nz - 1]: the key (cx, cy, m) exists, the scan meets it, and no other key of the face has
// iz == m.  A query outside the grid is clamped into a border column (or border cell in z); the faces met there are
// tested by the same rule 1 on their real coordinates, which rejects every one of them in x or y, and above the grid
// max z > qz fails.  Below the grid cz = 0 and the whole column is scanned, as it must be.  The test of a face is the
// same function for the walk and for brute force, so the result is brute force's, bit for bit, for any cell.
#pragma once
#include "mesh_distance_core.hpp"

namespace nerf_mi {

using nerf_grid::Corners;
using nerf_grid::Grid;
using nerf_grid::load_corners;

constexpr uint64_t BOX_STREAM = 0x626f78ULL;  // "box": the streams of a box point are BOX_STREAM + 0, 1, 2
constexpr double FILTER = 0x1p-48;

// ---------------------------------------------------------------- the exact orientation

// s + e == a + b exactly (Knuth)
NERF_MM_HD void two_sum(double a, double b, double& s, double& e) {
  const double x = a + b;
  const double bv = x - a;
  const double av = x - bv;
  const double br = b - bv;
  const double ar = a - av;
  s = x;
  e = ar + br;
}

NERF_MM_HD int sign_of(double x) { return x > 0.0 ? 1 : (x < 0.0 ? -1 : 0); }

// the exact sign of t0 + .. + t5 by the expansion alone
NERF_MM_HD int exact_sign6(double t0, double t1, double t2, double t3, double t4, double t5) {
  double h0 = t0, h1, h2, h3, h4, h5, q;
  two_sum(h0, t1, q, h0);
  h1 = q;
  two_sum(t2, h0, q, h0);
  two_sum(q, h1, q, h1);
  h2 = q;
  two_sum(t3, h0, q, h0);
  two_sum(q, h1, q, h1);
  two_sum(q, h2, q, h2);
  h3 = q;
  two_sum(t4, h0, q, h0);
  two_sum(q, h1, q, h1);
  two_sum(q, h2, q, h2);
  two_sum(q, h3, q, h3);
  h4 = q;
  two_sum(t5, h0, q, h0);
  two_sum(q, h1, q, h1);
  two_sum(q, h2, q, h2);
  two_sum(q, h3, q, h3);
  two_sum(q, h4, q, h4);
  h5 = q;
  if (h5 != 0.0) return sign_of(h5);
  if (h4 != 0.0) return sign_of(h4);
  if (h3 != 0.0) return sign_of(h3);
  if (h2 != 0.0) return sign_of(h2);
  if (h1 != 0.0) return sign_of(h1);
  return sign_of(h0);
}

// orient(P, Q, R) of the header comment; ``exact_path``, when given, is incremented when the filter did not decide
NERF_MM_HD int orient(float px, float py, float qx, float qy, float rx, float ry, int64_t* exact_path = nullptr) {
  const double Px = (double)px, Py = (double)py, Qx = (double)qx, Qy = (double)qy, Rx = (double)rx, Ry = (double)ry;
  const double t0 = Qx * Ry, t1 = -(Qx * Py), t2 = -(Px * Ry), t3 = -(Qy * Rx), t4 = Qy * Px, t5 = Py * Rx;
  const double sum = ((t0 + t1) + (t2 + t3)) + (t4 + t5);
  const double mag = ((fabs(t0) + fabs(t1)) + (fabs(t2) + fabs(t3))) + (fabs(t4) + fabs(t5));
  if (fabs(sum) > FILTER * mag) return sum > 0.0 ? 1 : -1;
  if (exact_path) ++*exact_path;
  return exact_sign6(t0, t1, t2, t3, t4, t5);
}

// rule 3 for one directed edge U -> V of a counter-clockwise projection
NERF_MM_HD bool edge_passes(float ux, float uy, float vx, float vy, float qx, float qy, int64_t* exact_path) {
  const int e = orient(ux, uy, vx, vy, qx, qy, exact_path);
  return e > 0 || (e == 0 && (vy < uy || (vy == uy && vx > ux)));
}

// ---------------------------------------------------------------- the test of a face

// Rules 1 to 4 for the corners a, b, c: 0 when the face is not crossed, else s = +1 or -1.
NERF_MM_HD int crossed_corners(const float a[3], const float b[3], const float c[3], const float q[3],
                               int64_t* exact_path = nullptr) {
  if (!(fmaxf(fmaxf(a[2], b[2]), c[2]) > q[2])) return 0;
  if (!(q[0] >= fminf(fminf(a[0], b[0]), c[0]) && q[0] <= fmaxf(fmaxf(a[0], b[0]), c[0]))) return 0;
  if (!(q[1] >= fminf(fminf(a[1], b[1]), c[1]) && q[1] <= fmaxf(fmaxf(a[1], b[1]), c[1]))) return 0;
  const int s = orient(a[0], a[1], b[0], b[1], c[0], c[1], exact_path);
  if (s == 0) return 0;
  // the counter-clockwise order a, B, C
  const float Bx = s > 0 ? b[0] : c[0], By = s > 0 ? b[1] : c[1];
  const float Cx = s > 0 ? c[0] : b[0], Cy = s > 0 ? c[1] : b[1];
  if (!edge_passes(a[0], a[1], Bx, By, q[0], q[1], exact_path)) return 0;
  if (!edge_passes(Bx, By, Cx, Cy, q[0], q[1], exact_path)) return 0;
  if (!edge_passes(Cx, Cy, a[0], a[1], q[0], q[1], exact_path)) return 0;
  double e1[3], e2[3], w[3], n[3];
  for (int k = 0; k < 3; ++k) {
    const double o = (double)a[k];
    e1[k] = (double)b[k] - o;
    e2[k] = (double)c[k] - o;
    w[k] = (double)q[k] - o;
  }
  nerf_grid::cross3(e1, e2, n);
  const double g = nerf_grid::dot3(n, w);
  return ((g < 0.0 && s > 0) || (g > 0.0 && s < 0)) ? s : 0;
}

struct Count {
  int32_t crossings, winding;
};

// every face in turn: the definition of the result
NERF_MM_HD Count brute(const float q[3], const float* verts, const int32_t* faces, int64_t F,
                       int64_t* exact_path = nullptr) {
  Count n = {0, 0};
  for (int64_t f = 0; f < F; ++f) {
    const Corners t = load_corners(verts, faces, f);
    const int s = crossed_corners(t.a, t.b, t.c, q, exact_path);
    n.crossings += s != 0;
    n.winding += s;
  }
  return n;
}

// ---------------------------------------------------------------- the walk

// The column of q from its own cell upwards.  n_keys == 0: (0, 0).  counts, when given, receives {keys scanned,
// faces tested after the once-only rule, orientation tests that took the exact path}.
NERF_MM_HD Count count_crossings(const Grid& g, const float q[3], const int64_t* keys, int64_t n_keys,
                                 const float* verts, const int32_t* faces, int64_t* counts = nullptr) {
  Count n = {0, 0};
  if (counts) counts[0] = counts[1] = counts[2] = 0;
  if (n_keys <= 0) return n;
  const int32_t cx = nerf_grid::cell_index(g, 0, q[0]), cy = nerf_grid::cell_index(g, 1, q[1]),
                cz = nerf_grid::cell_index(g, 2, q[2]);
  const int64_t base = nerf_grid::cell_id(g, cx, cy, 0);
  nerf_grid::for_run(g, keys, n_keys, cx, cy, cz, g.dims[2] - 1, [&](int64_t, int64_t cell, int32_t f) {
    if (counts) ++counts[0];
    const int32_t iz = (int32_t)(cell - base);
    const Corners t = load_corners(verts, faces, (int64_t)(uint32_t)f);
    const int32_t lz = nerf_grid::cell_index(g, 2, fminf(fminf(t.a[2], t.b[2]), t.c[2]));
    if (iz != (lz > cz ? lz : cz)) return;
    if (counts) ++counts[1];
    const int s = crossed_corners(t.a, t.b, t.c, q, counts ? counts + 2 : nullptr);
    n.crossings += s != 0;
    n.winding += s;
  });
  return n;
}

// ---------------------------------------------------------------- points of a box

// Coordinate c of point i: lo_c + u (hi_c - lo_c) in fp32, the difference, the product and the sum each rounded,
// u = (rand64(seed, BOX_STREAM + c, i) >> 40) 2^-24 (exact in fp32, in [0, 1)).
NERF_MM_HD void box_point(uint64_t seed, int64_t i, const float lo[3], const float hi[3], float* points) {
  for (int c = 0; c < 3; ++c) {
    const float u = (float)(nerf_mm::rand64(seed, BOX_STREAM + (uint64_t)c, (uint64_t)i) >> 40) * 0x1p-24f;
    const float d = hi[c] - lo[c];
    const float t = u * d;
    points[3 * i + c] = lo[c] + t;
  }
}

}  // namespace nerf_mi
