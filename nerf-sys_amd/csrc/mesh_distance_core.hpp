// Exact point-to-surface distance: the closest point of a triangle, the cell keys of a face and the
// exact nearest-face search through the uniform grid of mesh_grid_core.hpp, written once for the device and for a
// host compiler so that every loop can be run and checked under a host sanitizer without a GPU.
// Build with -ffp-contract=off: every fp64 operation below rounds on its own.
//
// The closest point.  The corners a, b, c and the query q are fp32 values converted to double; everything after that
// is double.  Dot products are (x x' + y y') + z z'.  The regions of Ericson, Real-Time Collision Detection §5.1.5,
// are tested in the order vertex a, vertex b, edge ab, vertex c, edge ac, edge bc, interior.  Every edge parameter and
// both interior weights pass through clamp01 (a NaN counts as 0) and the interior pair is cut back to v + w <= 1, so
// the returned point is always a combination of the corners with weights in [0, 1], evaluated with a handful of
// roundings of 2^-53: its distance to q never undercuts the true distance of the triangle by more than that rounding.
// d2 = (dx dx + dy dy) + dz dz of d = q - point (the double point, before it is rounded to fp32 for the caller).
// A face without area is treated as its three edges ab, ac, bc taken as segments, t = clamp01(((q - p0) . e) / (e . e)),
// t = 0 when e . e == 0, the smallest d2 winning and the earlier edge on a tie.  A face is in that class when it has a
// repeated index, when nerf_mm::face_cross is exactly (0, 0, 0), or when the walk reaches the interior with
// va + vb + vc <= 0: no division by zero and no NaN leaves this file for finite input.
//
// The search.  The faces are registered in the grid of mesh_grid_core.hpp, key = (cell_id << 32) | face, in every cell
// of the index box of their bounding box, so the search is that of nerf_mm::nearest (nerf_grid::walk_shells and
// nerf_grid::for_run) with a face evaluation in place of a point distance.  A face met in several cells is evaluated
// again: min is idempotent.  The search stops before shell r >= 2 when nerf_grid::shell_can_stop holds for best_d2
// rounded UP to fp32.
//
// Why that is safe.  mesh_grid_core.hpp shows that before shell r the real distance from the query to any point of
// an unevaluated face is at least (r - 1 - 2^-11) cell.  The part that is this search's own: the d2 computed for such
// a face is the squared distance to a combination of its corners with weights in [0, 1] up to a few roundings of
// 2^-53, so it is at least ((r - 1 - 2^-11) cell)^2 (1 - 2^-48); rounding best_d2 up to fp32 only makes the test
// harder to pass.  The rule keeps 2^-8 - 2^-11 of a cell and 2^-10 relative in hand: when it fires, every unevaluated
// face is strictly farther than the best, so neither the distance nor the smallest-index tie-break can change.  The
// result is brute force's, bit for bit.  Tighten the slack only with an argument.
#pragma once
#include "mesh_metrics_core.hpp"

namespace nerf_md {

using nerf_grid::dot3;
using nerf_grid::face_box;
using nerf_grid::face_cell_count;
using nerf_grid::face_keys;
using nerf_grid::Grid;

// ---------------------------------------------------------------- the closest point of a triangle

// t >= 0 ? (t <= 1 ? t : 1) : 0: a NaN counts as 0
NERF_MM_HD double clamp01(double t) { return t >= 0.0 ? (t <= 1.0 ? t : 1.0) : 0.0; }

NERF_MM_HD double dist2(const double q[3], const double r[3]) {
  const double d[3] = {q[0] - r[0], q[1] - r[1], q[2] - r[2]};
  return dot3(d, d);
}

// The region walk.  false when the interior is reached with va + vb + vc <= 0 (the caller then takes the edges).
NERF_MM_HD bool walk(const double a[3], const double b[3], const double c[3], const double q[3], double r[3]) {
  double ab[3], ac[3], ap[3], bp[3], cp[3];
  for (int k = 0; k < 3; ++k) {
    ab[k] = b[k] - a[k];
    ac[k] = c[k] - a[k];
    ap[k] = q[k] - a[k];
    bp[k] = q[k] - b[k];
    cp[k] = q[k] - c[k];
  }
  const double d1 = dot3(ab, ap), d2 = dot3(ac, ap);
  if (d1 <= 0.0 && d2 <= 0.0) {  // vertex a
    for (int k = 0; k < 3; ++k) r[k] = a[k];
    return true;
  }
  const double d3 = dot3(ab, bp), d4 = dot3(ac, bp);
  if (d3 >= 0.0 && d4 <= d3) {  // vertex b
    for (int k = 0; k < 3; ++k) r[k] = b[k];
    return true;
  }
  const double vc0 = d1 * d4, vc1 = d3 * d2;
  const double vc = vc0 - vc1;
  if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {  // edge ab
    const double v = clamp01(d1 / (d1 - d3));
    for (int k = 0; k < 3; ++k) {
      const double t = v * ab[k];
      r[k] = a[k] + t;
    }
    return true;
  }
  const double d5 = dot3(ab, cp), d6 = dot3(ac, cp);
  if (d6 >= 0.0 && d5 <= d6) {  // vertex c
    for (int k = 0; k < 3; ++k) r[k] = c[k];
    return true;
  }
  const double vb0 = d5 * d2, vb1 = d1 * d6;
  const double vb = vb0 - vb1;
  if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {  // edge ac
    const double w = clamp01(d2 / (d2 - d6));
    for (int k = 0; k < 3; ++k) {
      const double t = w * ac[k];
      r[k] = a[k] + t;
    }
    return true;
  }
  const double va0 = d3 * d6, va1 = d5 * d4;
  const double va = va0 - va1;
  const double u1 = d4 - d3, u2 = d5 - d6;
  if (va <= 0.0 && u1 >= 0.0 && u2 >= 0.0) {  // edge bc
    const double w = clamp01(u1 / (u1 + u2));
    for (int k = 0; k < 3; ++k) {
      const double e = c[k] - b[k];
      const double t = w * e;
      r[k] = b[k] + t;
    }
    return true;
  }
  const double s = (va + vb) + vc;
  if (!(s > 0.0)) return false;
  const double v = clamp01(vb / s);
  double w = clamp01(vc / s);
  if (v + w > 1.0) w = 1.0 - v;
  for (int k = 0; k < 3; ++k) {
    const double t1 = v * ab[k], t2 = w * ac[k];
    const double o = a[k] + t1;
    r[k] = o + t2;
  }
  return true;
}

// The closest point of the segment p0 p1; taken when ``first`` or when strictly nearer than best_d2.
NERF_MM_HD void segment(const double p0[3], const double p1[3], const double q[3], bool first, double& best_d2,
                        double best[3]) {
  double e[3], w[3], r[3];
  for (int k = 0; k < 3; ++k) {
    e[k] = p1[k] - p0[k];
    w[k] = q[k] - p0[k];
  }
  const double ee = dot3(e, e);
  const double t = ee == 0.0 ? 0.0 : clamp01(dot3(w, e) / ee);
  for (int k = 0; k < 3; ++k) {
    const double s = t * e[k];
    r[k] = p0[k] + s;
  }
  const double d2 = dist2(q, r);
  if (first || d2 < best_d2) {
    best_d2 = d2;
    for (int k = 0; k < 3; ++k) best[k] = r[k];
  }
}

// The squared distance from q to face f, in double, and the closest point rounded to fp32.
NERF_MM_HD double closest_on_face(const float* p, const int32_t* faces, int64_t f, const float qf[3], float closest[3]) {
  const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  const nerf_grid::Corners t = nerf_grid::load_corners(p, faces, f);
  double a[3], b[3], c[3], q[3], r[3];
  for (int k = 0; k < 3; ++k) {
    a[k] = (double)t.a[k];
    b[k] = (double)t.b[k];
    c[k] = (double)t.c[k];
    q[k] = (double)qf[k];
  }
  bool flat = i0 == i1 || i1 == i2 || i0 == i2;
  if (!flat) {
    double x[3];
    nerf_mm::face_cross(p, faces, f, x);
    flat = x[0] == 0.0 && x[1] == 0.0 && x[2] == 0.0;
  }
  double d2 = 0.0;
  if (!flat) flat = !walk(a, b, c, q, r);
  if (flat) {
    segment(a, b, q, true, d2, r);
    segment(a, c, q, false, d2, r);
    segment(b, c, q, false, d2, r);
  } else {
    d2 = dist2(q, r);
  }
  for (int k = 0; k < 3; ++k) closest[k] = (float)r[k];
  return d2;
}

// ---------------------------------------------------------------- the search

struct BestFace {
  double d2;
  int32_t face;
  float p[3];
};

// Smaller d2 wins, on equal d2 the smaller face; face == -1 compares as the largest index.
NERF_MM_HD void consider(const float* vertices, const int32_t* faces, int32_t f, const float q[3], BestFace& best) {
  float r[3];
  const double d2 = closest_on_face(vertices, faces, f, q, r);
  if (d2 < best.d2 || (d2 == best.d2 && (uint32_t)f < (uint32_t)best.face)) {
    best.d2 = d2;
    best.face = f;
    best.p[0] = r[0], best.p[1] = r[1], best.p[2] = r[2];
  }
}

// best_d2 rounded up to fp32 (+inf beyond the fp32 range), so that shell_can_stop errs towards searching on
NERF_MM_HD float round_up(double d2) {
  float f = (float)d2;
  if ((double)f < d2) f = nextafterf(f, INFINITY);
  return f;
}

// The nearest face of q.  The walk of a run is bounded by n_keys.  n_keys == 0: d2 = +inf, face = -1, the point = q.
NERF_MM_HD BestFace nearest_face(const Grid& g, const float q[3], const int64_t* keys, int64_t n_keys,
                                 const float* vertices, const int32_t* faces) {
  BestFace best = {(double)INFINITY, -1, {q[0], q[1], q[2]}};
  if (n_keys <= 0) return best;
  nerf_grid::walk_shells(
      g, q, [&](int32_t r) { return nerf_grid::shell_can_stop(round_up(best.d2), r, g.cell); },
      [&](int32_t ix, int32_t iy, int32_t z0, int32_t z1) {
        nerf_grid::for_run(g, keys, n_keys, ix, iy, z0, z1,
                           [&](int64_t, int64_t, int32_t f) { consider(vertices, faces, f, q, best); });
      });
  return best;
}

}  // namespace nerf_md
