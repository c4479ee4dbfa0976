// The generalised winding number of a triangle mesh (Jacobson et al. 2013, with the one-level
// first-order far field of Barill et al. 2018): the solid angle of a face, the brick of a face, the moments of a brick
// and the sum of a query, written once for the device and for a host compiler so that every loop can be run and
// checked under a host sanitizer without a GPU.
// Build with -ffp-contract=off: every fp32 and fp64 operation below rounds on its own.  Everything but the centroid
// cell is double; dot3 is (x x' + y y') + z z' and cross3 six products and three differences (mesh_grid_core.hpp).
//
// The solid angle.  The corners are fp32 values widened to double; a, b, c = corner - q;
//   N = a . (b x c),  la = sqrt(a . a), lb, lc likewise,
//   D = (((la lb) lc + (a . b) lc) + (b . c) la) + (c . a) lb,
//   omega = 2 atan2(N, D)                                         (Van Oosterom and Strackee 1983).
// w(q) = (sum of omega over the faces) / 4 pi.  A closed mesh with positive Mesh.volume() (normals outwards, the
// extractor's convention) gives w = +1 inside and 0 outside: the same sign as the crossing-count winding of
// mesh_inside_core.hpp.  For q on the surface itself N is +0 or -0 and omega is what atan2 makes of it (0 or +-2 pi
// in the plane of a face): deterministic, not meaningful.
//
// The bricks.  A face belongs to ONE brick, the cell of its centroid in a coarse grid over the vertex box:
//   g_k = ((a_k + b_k) + c_k) * fp32(1/3) in fp32 (two sums and a product, each rounded; fp32(1/3) = 0x1.555556p-2),
//   brick = cell_id(cell_index(g_x), cell_index(g_y), cell_index(g_z)),  key = (brick << 32) | face.
// Sorted ascending, the faces of a brick are contiguous and ascending by index.  Occupied brick number b owns the run
// [start_b, end_b) of sorted positions, and its moments are sums over that run in sorted order by one owner:
//   x_f = (b - a) x (c - a) of the widened corners,  n = sum of 0.5 x_f (per component),
//   m_f = sqrt(x_f . x_f) (twice the area),  s_f = (a + b) + c (three times the centroid, per component),
//   P = sum of m_f s_f,  M = sum of m_f,  S = sum of s_f, each started from 0 and added to in sorted order;
//   p = P / (3 M) when M > 0, else S / (3 count), per component;
//   r2 = the largest (corner - p) . (corner - p) over the corners a, b, c of the run, started from 0.
//
// The sum of a query.  One double accumulator, the bricks in ascending order: d = p - q, d2 = d . d; the brick is far
// iff not ``exact`` and d2 > beta2 r2 (beta2 = beta beta, the product beta2 r2 rounded once; a strict compare, so a
// brick with r2 = 0 at the query itself is near, and d2 > 0 for every far brick); a far brick adds
// (d . n) / (d2 sqrt(d2)), a near brick adds the omega of its faces in sorted order.  w = acc / FOUR_PI.  With
// ``exact`` every brick is near: brute force in sorted-face order.
//
// What the far field is.  The solid angle of a small patch of area A and unit normal u at displacement d is
// A (u . d) / |d|^3 + O(A (r / |d|)^2 / |d|^2); summed over a brick around its area-weighted centroid the linear term
// of the expansion vanishes for a flat brick and is small for a gently curved one.  The error for a brick is bounded
// by a constant times its solid angle times 1 / beta^2, so the total falls as beta grows and does not depend on the
// brick size (DESIGN §3.11.10 has the measured table).
#pragma once
#include "mesh_grid_core.hpp"

namespace nerf_mw {

using nerf_grid::cross3;
using nerf_grid::dot3;
using nerf_grid::Grid;

constexpr float THIRD = 0x1.555556p-2f;              // fp32(1 / 3)
constexpr double FOUR_PI = 12.566370614359172;       // the double nearest to 4 pi
constexpr int RUN = 2, MOMENTS = 7, SOUP = 9;        // ints per run, doubles per record, floats per sorted face

// ---------------------------------------------------------------- the solid angle

// omega of the corners a, b, c (9 floats, in that order) seen from q
NERF_GRID_HD double solid_angle(const float* t, const double q[3]) {
  double a[3], b[3], c[3], x[3];
  for (int k = 0; k < 3; ++k) {
    a[k] = (double)t[k] - q[k];
    b[k] = (double)t[3 + k] - q[k];
    c[k] = (double)t[6 + k] - q[k];
  }
  cross3(b, c, x);
  const double N = dot3(a, x);
  const double la = sqrt(dot3(a, a)), lb = sqrt(dot3(b, b)), lc = sqrt(dot3(c, c));
  const double ab = dot3(a, b), bc = dot3(b, c), ca = dot3(c, a);
  const double t0 = (la * lb) * lc, t1 = ab * lc, t2 = bc * la, t3 = ca * lb;
  const double D = ((t0 + t1) + t2) + t3;
  return 2.0 * atan2(N, D);
}

// ---------------------------------------------------------------- the brick of a face

NERF_GRID_HD int64_t face_brick_key(const Grid& g, const float* verts, const int32_t* faces, int64_t f) {
  const nerf_grid::Corners t = nerf_grid::load_corners(verts, faces, f);
  int32_t i[3];
  for (int k = 0; k < 3; ++k) {
    const float s = t.a[k] + t.b[k];
    const float u = s + t.c[k];
    i[k] = nerf_grid::cell_index(g, k, u * THIRD);
  }
  return nerf_grid::make_key(nerf_grid::cell_id(g, i[0], i[1], i[2]), (uint32_t)f);
}

// the corners of the face at sorted position j, 9 floats
NERF_GRID_HD void write_soup(const float* verts, const int32_t* faces, const int64_t* sorted_keys, int64_t j,
                             float* soup) {
  const nerf_grid::Corners t = nerf_grid::load_corners(verts, faces, (int64_t)(uint32_t)nerf_grid::key_item(sorted_keys[j]));
  float* o = soup + SOUP * j;
  for (int k = 0; k < 3; ++k) o[k] = t.a[k], o[3 + k] = t.b[k], o[6 + k] = t.c[k];
}

// ---------------------------------------------------------------- the moments of a brick

// run[0 .. 1] = [start, end), rec[0 .. 6] = p, n, r2 of occupied brick b; starts (B,) ascending, starts[0] = 0
NERF_GRID_HD void brick_moments(const float* soup, int64_t F, const int64_t* starts, int64_t B, int64_t b, int32_t* run,
                                double* rec) {
  const int64_t s = starts[b], e = b + 1 < B ? starts[b + 1] : F;
  double n[3] = {0.0, 0.0, 0.0}, P[3] = {0.0, 0.0, 0.0}, S[3] = {0.0, 0.0, 0.0}, M = 0.0;
  for (int64_t j = s; j < e; ++j) {
    const float* t = soup + SOUP * j;
    double a[3], e1[3], e2[3], x[3];
    for (int k = 0; k < 3; ++k) {
      a[k] = (double)t[k];
      e1[k] = (double)t[3 + k] - a[k];
      e2[k] = (double)t[6 + k] - a[k];
    }
    cross3(e1, e2, x);
    const double m = sqrt(dot3(x, x));
    for (int k = 0; k < 3; ++k) {
      const double half = 0.5 * x[k];
      const double sk = (a[k] + (double)t[3 + k]) + (double)t[6 + k];
      const double w = m * sk;
      n[k] = n[k] + half;
      P[k] = P[k] + w;
      S[k] = S[k] + sk;
    }
    M = M + m;
  }
  double p[3];
  const double den = M > 0.0 ? 3.0 * M : 3.0 * (double)(e - s);
  for (int k = 0; k < 3; ++k) p[k] = (M > 0.0 ? P[k] : S[k]) / den;
  double r2 = 0.0;
  for (int64_t j = s; j < e; ++j) {
    const float* t = soup + SOUP * j;
    for (int v = 0; v < 3; ++v) {
      const double d[3] = {(double)t[3 * v] - p[0], (double)t[3 * v + 1] - p[1], (double)t[3 * v + 2] - p[2]};
      const double d2 = dot3(d, d);
      r2 = d2 > r2 ? d2 : r2;
    }
  }
  run[0] = (int32_t)s, run[1] = (int32_t)e;
  for (int k = 0; k < 3; ++k) rec[k] = p[k], rec[3 + k] = n[k];
  rec[6] = r2;
}

// ---------------------------------------------------------------- the sum of a query

// w(q).  counts, when given, receives {far bricks, faces summed exactly}.
NERF_GRID_HD double winding(const float q32[3], const int32_t* runs, const double* moments, int64_t B, const float* soup,
                            double beta2, bool exact, int64_t* counts = nullptr) {
  const double q[3] = {(double)q32[0], (double)q32[1], (double)q32[2]};
  double acc = 0.0;
  if (counts) counts[0] = counts[1] = 0;
  for (int64_t b = 0; b < B; ++b) {
    const double* rec = moments + MOMENTS * b;
    const double d[3] = {rec[0] - q[0], rec[1] - q[1], rec[2] - q[2]};
    const double d2 = dot3(d, d);
    if (!exact && d2 > beta2 * rec[6]) {
      const double num = dot3(d, rec + 3);
      const double den = d2 * sqrt(d2);
      acc = acc + num / den;
      if (counts) ++counts[0];
    } else {
      const int64_t s = runs[RUN * b], e = runs[RUN * b + 1];
      for (int64_t j = s; j < e; ++j) acc = acc + solid_angle(soup + SOUP * j, q);
      if (counts) counts[1] += e - s;
    }
  }
  return acc / FOUR_PI;
}

}  // namespace nerf_mw
