// Nearest-hit ray casting against a mesh: the ray / triangle test and the walk of a ray through the
// face grid of mesh_grid_core.hpp, written once for the device and for a host compiler so that every loop can be
// run and checked under a host sanitizer without a GPU.
// Build with -ffp-contract=off: every fp64 operation below rounds on its own.
//
// The hit test.  A ray is a row [o, d, near, far] of fp32 values converted to double, its points o + t d; d is not
// normalised and t is the ray's own parameter.  The corners a, b, c are fp32 values converted to double; everything
// after that is double.  Dot products are (x x' + y y') + z z', cross products six products and three differences.
//   e1 = b - a, e2 = c - a, p = d x e2, det = e1 . p, s = o - a,
//   u = (s . p) / det, q = s x e1, v = (d . q) / det, t = (e2 . q) / det          (three divisions, no reciprocal).
// A face is never hit when it has a repeated index, when nerf_mm::face_cross is exactly (0, 0, 0), when det == 0, or,
// with cull, when det <= 0 (det > 0: the ray runs against the face's winding normal).  Otherwise it is hit when
// u >= 0, u <= 1, v >= 0, u + v <= 1, near <= t, t <= far and, on every axis k, P_k = o_k + t d_k (the product and the
// sum each rounded) lies in [min_k - m, max_k + m] of the face's three corners, m = margin = 2^-30 of the largest
// |coordinate| of the mesh.  Every comparison is written so that a NaN fails it.  The box clause never bites on a
// well-conditioned face; on a sliver, where a tiny non-zero det makes u, v, t garbage, it keeps "what brute force
// accepts" inside "what lies near the face", and that is what lets a grid walk find the same hits.  The result of a
// ray is the smallest accepted t and, on equal t, the smaller face.
//
// The walk.  rel = o - lo and c_k(t) = (rel_k + t d_k) / cell is the ray in cell coordinates, as computed.  [near, far]
// is clipped to the grid's box widened by S = 2^-6 of a cell on every side (a slab test; an axis with d_k == 0 is an
// inside test on rel_k, never a division); an empty interval is a miss.  M is the axis of the largest |d_k|, the
// first on a tie.  The layers i of cells along M are walked in the ray's direction from the layer of c_M(t0), one
// back.  Layer i, widened by S on both sides, is crossed between tin and tout, (plane - rel_M) / d_M for its two
// planes; over [max(tin, t0), min(tout, t1)] the two other coordinates run between their values at the two ends, and
// the cells floor(min - S) .. floor(max + S), clamped to the grid, are searched: one nerf_grid::lower_bound per run
// of cells contiguous in z, every face of a run tested (a face met again changes nothing: the comparison is strict).
// The minor slopes are at most 1, a widened layer is 1 + 2 S thick, so that is at most 3 x 3 cells.  The walk stops
// before a layer with tin > best t, or tin > t1.  Every loop is bounded by a dim or by n_keys.
//
// Why the walk misses nothing.  Take a hit (t, f) that the test accepts.
// (1) P_k(t) lies in the box of f widened by m on every axis.  The caller refuses a grid with m > 2^-10 cell (that is
//     cell < 2^-20 of the largest |coordinate|: sixteen fp32 ulps, no real restriction).  By mesh_grid_core.hpp
//     every real point of f's box lies in its registered cells widened by delta = 2^-12, so P(t) lies in the
//     registered cells of f widened by delta + 2^-10: there is a registered cell (jx, jy, jz) with
//     j_k - delta - 2^-10 <= (P_k - lo_k) / cell <= j_k + 1 + delta + 2^-10 on every axis.
// (2) The arithmetic.  The walk runs only when |rel_k| <= 2^32 cell on every axis; a ray from farther away tests
//     every face, which is brute force itself.  lo is a vertex coordinate, so |lo_k| <= 2^20 cell, and for a t inside
//     the clipped interval |t d_k| <= |t d_M| <= |rel_M| + 1025 cell.  Hence P_k(t), rel_k + t d_k, c_k(t) and the real
//     line agree within 2^-52 (2^33 + 2^33) cell < 2^-17 of a cell, and the real position at a computed plane
//     parameter (plane - rel_k) / d_k is within 2^-52 2^33 cell = 2^-19 of a cell of the plane, whatever |d_k| is.
// (3) The clip keeps t.  (P_k - lo_k) / cell lies in [-delta - 2^-10, dims_k + delta + 2^-10] by (1), the real line
//     within 2^-17 of it, the clip's planes are S = 2^-6 outside the box and met within 2^-19: the real position at t
//     lies strictly between those at the two clip parameters, and the real line is strictly monotone in t where
//     d_k != 0, so t is inside; where d_k == 0, P_k(t) = o_k exactly and the inside test holds with the same room.
// (4) The layer is reached and its interval holds t.  The same comparison on the axis M with the planes of layer
//     j_M gives tin < t < tout, and with t0 <= t the start layer, floor(c_M(t0)) one back, is not beyond j_M.
// (5) The cell is searched.  For t in [max(tin, t0), min(tout, t1)] the real minor coordinates lie between their
//     values at the two ends; the computed ones are within 2^-17 of them and P within 2^-17 of the line, so
//     [j_k, j_k + 1] is within delta + 2^-10 + 2^-16 < S of the interval searched and j_k, which lies in the grid,
//     survives the clamp.
// (6) The stop.  tin is monotone along the walk (a difference and a division by the same d_M).  A hit whose cell lies
//     in a layer that was not walked has t > tin of its layer >= tin of the first layer left out > best t: it can
//     neither win nor tie.
// Kept in hand: S = 2^-6 = 0.0156 of a cell against delta + 2^-10 + 2^-16 < 0.0013.  The result is brute force's,
// bit for bit.  Tighten the slack only with an argument.
#pragma once
#include "mesh_distance_core.hpp"

namespace nerf_mr {

using nerf_grid::cross3;
using nerf_grid::Grid;

constexpr double SLACK = 0.015625;           // S = 2^-6 of a cell
constexpr double FAR_ORIGIN = 4294967296.0;  // 2^32 cells: beyond it every face is tested

struct Ray {
  double o[3], d[3], near, far;
};

struct Hit {
  double t;
  int32_t face;
  float u, v;
};

NERF_MM_HD Ray load_ray(const float* rays, int64_t i) {
  Ray r;
  for (int k = 0; k < 3; ++k) {
    r.o[k] = (double)rays[8 * i + k];
    r.d[k] = (double)rays[8 * i + 3 + k];
  }
  r.near = (double)rays[8 * i + 6];
  r.far = (double)rays[8 * i + 7];
  return r;
}

// ---------------------------------------------------------------- the hit test

// The rule of the header comment for face f: true and (t, u, v) on a hit.
NERF_MM_HD bool hit_face(const float* verts, const int32_t* faces, int64_t f, const Ray& r, double margin, bool cull,
                         double& t, double& u, double& v) {
  const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  if (i0 == i1 || i1 == i2 || i0 == i2) return false;
  double x[3];
  nerf_mm::face_cross(verts, faces, f, x);
  if (x[0] == 0.0 && x[1] == 0.0 && x[2] == 0.0) return false;
  const nerf_grid::Corners c = nerf_grid::load_corners(verts, faces, f);
  double a[3], e1[3], e2[3], s[3], p[3], q[3];
  for (int k = 0; k < 3; ++k) {
    a[k] = (double)c.a[k];
    e1[k] = (double)c.b[k] - a[k];
    e2[k] = (double)c.c[k] - a[k];
    s[k] = r.o[k] - a[k];
  }
  cross3(r.d, e2, p);
  const double det = nerf_grid::dot3(e1, p);
  if (det == 0.0) return false;
  if (cull && det <= 0.0) return false;
  u = nerf_grid::dot3(s, p) / det;
  cross3(s, e1, q);
  v = nerf_grid::dot3(r.d, q) / det;
  t = nerf_grid::dot3(e2, q) / det;
  if (!(u >= 0.0 && u <= 1.0 && v >= 0.0 && u + v <= 1.0)) return false;
  if (!(r.near <= t && t <= r.far)) return false;
  for (int k = 0; k < 3; ++k) {
    const double mn = (double)fminf(fminf(c.a[k], c.b[k]), c.c[k]) - margin,
                 mx = (double)fmaxf(fmaxf(c.a[k], c.b[k]), c.c[k]) + margin;
    const double td = t * r.d[k];
    const double P = r.o[k] + td;
    if (!(P >= mn && P <= mx)) return false;
  }
  return true;
}

// Smaller t wins, on equal t the smaller face; face == -1 compares as the largest index.
NERF_MM_HD void consider(const float* verts, const int32_t* faces, int32_t f, const Ray& r, double margin, bool cull,
                         Hit& best) {
  double t, u, v;
  if (!hit_face(verts, faces, f, r, margin, cull, t, u, v)) return;
  if (t < best.t || (t == best.t && (uint32_t)f < (uint32_t)best.face)) {
    best.t = t;
    best.face = f;
    best.u = (float)u;
    best.v = (float)v;
  }
}

NERF_MM_HD Hit miss() {
  Hit h = {(double)INFINITY, -1, 0.0f, 0.0f};
  return h;
}

// every face in turn: the definition of the result
NERF_MM_HD Hit brute(const Ray& r, const float* verts, const int32_t* faces, int64_t F, double margin, bool cull) {
  Hit best = miss();
  for (int64_t f = 0; f < F; ++f) consider(verts, faces, (int32_t)f, r, margin, cull, best);
  return best;
}

// ---------------------------------------------------------------- the walk

// floor(x) clamped to [0, dim - 1] as a double, then converted: a NaN counts as 0
NERF_MM_HD int32_t floor_cell(double x, int32_t dim) {
  const double f = floor(x), top = (double)(dim - 1);
  return (int32_t)(f >= 0.0 ? (f <= top ? f : top) : 0.0);
}

// The cells c0 .. c1 of a minor axis that the ray, widened by S, crosses over the parameters [a, b]; false when they
// all lie outside the grid.
NERF_MM_HD bool minor_cells(double rel, double d, int32_t dim, double a, double b, double inv, int32_t& c0,
                            int32_t& c1) {
  const double sa = a * d, sb = b * d;
  const double ca = (rel + sa) * inv, cb = (rel + sb) * inv;
  const double pl = (ca < cb ? ca : cb) - SLACK, ph = (ca < cb ? cb : ca) + SLACK;
  c0 = floor_cell(pl, dim);
  c1 = floor_cell(ph, dim);
  return ph >= 0.0 && pl <= (double)dim;
}

// The nearest hit of ray r.  n_keys == 0: a miss.  counts, when given, receives {layers walked, faces tested} (the
// host tools report them; the kernel drops them).
NERF_MM_HD Hit cast(const Grid& g, const Ray& r, const int64_t* keys, int64_t n_keys, const float* verts,
                    const int32_t* faces, int64_t F, double margin, bool cull, int64_t* counts = nullptr) {
  Hit best = miss();
  int64_t layers = 0, tested = 0;
  if (counts) counts[0] = counts[1] = 0;
  if (n_keys <= 0) return best;
  const double cell = (double)g.cell;
  const double inv = 1.0 / cell;
  double rel[3];
  bool far_origin = false;
  for (int k = 0; k < 3; ++k) {
    rel[k] = r.o[k] - (double)g.lo[k];
    if (!(fabs(rel[k]) <= FAR_ORIGIN * cell)) far_origin = true;
  }
  if (far_origin) {
    if (counts) counts[1] = F;
    return brute(r, verts, faces, F, margin, cull);
  }
  // the clip: [near, far] against the box widened by S
  double t0 = r.near, t1 = r.far;
  for (int k = 0; k < 3; ++k) {
    const double a = -SLACK * cell, b = ((double)g.dims[k] + SLACK) * cell;
    if (r.d[k] == 0.0) {
      if (!(rel[k] >= a && rel[k] <= b)) return best;
      continue;
    }
    const double ta = (a - rel[k]) / r.d[k], tb = (b - rel[k]) / r.d[k];
    const double tin = ta < tb ? ta : tb, tout = ta < tb ? tb : ta;
    if (tin > t0) t0 = tin;
    if (tout < t1) t1 = tout;
  }
  if (!(t0 <= t1)) return best;
  // the major axis; its values are picked by comparisons, not by an index, so that the arrays stay in registers
  int M = 0;
  double dm = r.d[0];
  if (fabs(r.d[1]) > fabs(dm)) M = 1, dm = r.d[1];
  if (fabs(r.d[2]) > fabs(dm)) M = 2, dm = r.d[2];
  if (dm == 0.0) return best;  // d = 0: no face has det != 0
  const double relm = M == 0 ? rel[0] : (M == 1 ? rel[1] : rel[2]);
  const int32_t sg = dm > 0.0 ? 1 : -1, nM = M == 0 ? g.dims[0] : (M == 1 ? g.dims[1] : g.dims[2]);
  const double s0 = t0 * dm;
  int32_t i = floor_cell((relm + s0) * inv - (double)sg, nM);
  for (int32_t step = 0; step < nM && i >= 0 && i < nM; ++step, i += sg) {
    const double A = ((double)i - SLACK) * cell, B = ((double)(i + 1) + SLACK) * cell;
    const double ta = (A - relm) / dm, tb = (B - relm) / dm;
    const double tin = sg > 0 ? ta : tb, tout = sg > 0 ? tb : ta;
    if (tin > best.t || tin > t1) break;
    const double a = tin > t0 ? tin : t0, b = tout < t1 ? tout : t1;
    if (!(a <= b)) continue;
    ++layers;
    int32_t x0 = i, x1 = i, y0 = i, y1 = i, z0 = i, z1 = i;
    bool inside = true;
    if (M != 0) inside = minor_cells(rel[0], r.d[0], g.dims[0], a, b, inv, x0, x1) && inside;
    if (M != 1) inside = minor_cells(rel[1], r.d[1], g.dims[1], a, b, inv, y0, y1) && inside;
    if (M != 2) inside = minor_cells(rel[2], r.d[2], g.dims[2], a, b, inv, z0, z1) && inside;
    if (!inside) continue;
    for (int32_t ix = x0; ix <= x1; ++ix)
      for (int32_t iy = y0; iy <= y1; ++iy)
        nerf_grid::for_run(g, keys, n_keys, ix, iy, z0, z1, [&](int64_t, int64_t, int32_t f) {
          consider(verts, faces, f, r, margin, cull, best);
          ++tested;
        });
  }
  if (counts) counts[0] = layers, counts[1] = tested;
  return best;
}

}  // namespace nerf_mr
