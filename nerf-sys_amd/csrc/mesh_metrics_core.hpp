// Mesh metrics: the counter random numbers, the face area, the area-weighted surface sampler, the
// cell keys of a point set and the exact nearest-neighbour search through a uniform grid, written once for the device
// and for a host compiler so that every loop can be run and checked under a host sanitizer without a GPU.
// Build with -ffp-contract=off: every fp32 and fp64 operation below rounds on its own.
//
// The search.  The reference points P are binned into the grid of mesh_grid_core.hpp, key = (cell_id << 32) | j, and a
// query walks the Chebyshev shells around its own clamped cell (nerf_grid::walk_shells), measuring every point of
// every run (nerf_grid::for_run), until nerf_grid::shell_can_stop holds for the best fp32 d2.
//
// Why that is safe.  mesh_grid_core.hpp shows that before shell r every unsearched point lies at least
// (r - 1 - 2^-11) cell from the query.  The part that is this search's own: the fp32 distance
// d2 = (dx dx + dy dy) + dz dz carries at most five roundings of 2^-24 each against the real squared distance (one
// per difference, squared, one per product, two sums), and every fp32 operation is monotone, so the d2 of an
// unsearched point is at least ((r - 1 - 2^-11) cell)^2 (1 - 2^-21).  The rule leaves 2^-8 - 2^-11 of a cell and
// 2^-10 - 2^-21 relative in hand (it is evaluated in double, whose own rounding is 2^-53): when it fires, every
// unsearched point is strictly farther than the best, so neither the distance nor the smallest-index tie-break can
// change.  The result is brute force's, bit for bit.  Tighten the slack only with an argument.
#pragma once
#include "mesh_grid_core.hpp"

#define NERF_MM_HD NERF_GRID_HD

namespace nerf_mm {

using nerf_grid::cell_index;
using nerf_grid::Grid;
using nerf_grid::MAX_DIM;
using nerf_grid::point_key;
using nerf_grid::shell_can_stop;

// ---------------------------------------------------------------- counter random numbers

// splitmix64 finaliser
NERF_MM_HD uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}

// the 64-bit value of (seed, stream a, index b) that nerf_uniform (common.hpp) shifts down to 24 bits
NERF_MM_HD uint64_t rand64(uint64_t seed, uint64_t a, uint64_t b) {
  return mix64(seed * 0x9e3779b97f4a7c15ULL + mix64(a * 0xd1b54a32d192ed03ULL + b));
}

// the high 64 bits of a * b: for a uniform a, an integer in [0, b)
NERF_MM_HD uint64_t umulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * (unsigned __int128)b) >> 64);
#endif
}

constexpr uint64_t SAMPLE_STREAM = 0x6d657368ULL;  // "mesh": the streams of a sample are SAMPLE_STREAM + 0, 1, 2

// ---------------------------------------------------------------- faces

// (p1 - p0) x (p2 - p0) of face f in double: the differences, the six products and the three differences of
// products each rounded once.  A face with a repeated index gives exactly (0, 0, 0): an edge is 0, or both are equal
// and the paired products are the same number.
NERF_MM_HD void face_cross(const float* p, const int32_t* faces, int64_t f, double c[3]) {
  const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  double a[3], b[3];
  for (int k = 0; k < 3; ++k) {
    const double o = (double)p[3 * i0 + k];
    a[k] = (double)p[3 * i1 + k] - o;
    b[k] = (double)p[3 * i2 + k] - o;
  }
  nerf_grid::cross3(a, b, c);
}

NERF_MM_HD double norm3(const double c[3]) {
  const double xx = c[0] * c[0], yy = c[1] * c[1], zz = c[2] * c[2];
  return sqrt((xx + yy) + zz);
}

NERF_MM_HD double face_area(const float* p, const int32_t* faces, int64_t f) {
  double c[3];
  face_cross(p, faces, f, c);
  return 0.5 * norm3(c);
}

// The first index in [0, n] with cdf[index] > target (n when there is none).  n < 2^31: at most 31 halvings, the trip
// count is bounded by 32 whatever the data.  A face of weight 0 has cdf[f] == cdf[f - 1] (or 0 for f == 0), so it is
// never the first index above a target.
NERF_MM_HD int64_t upper_bound(const int64_t* cdf, int64_t n, int64_t target) {
  int64_t lo = 0, hi = n;
  for (int step = 0; step < 32 && lo < hi; ++step) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (cdf[mid] > target) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// Sample i of the surface: the face by the integer CDF (cdf[F - 1] == total, 0 < total < 2^63), the barycentric
// pair by an integer fold of two 24-bit numbers onto the triangle, the point in double.  normals_out may be NULL;
// vertex_normals NULL selects the face's own unit normal.  The face is clamped to F - 1, which the caller's own
// cdf / total never need.
NERF_MM_HD void sample(const float* p, const int32_t* faces, int64_t F, const int64_t* cdf, uint64_t total,
                       const float* vertex_normals, uint64_t seed, int64_t i, float* points, int32_t* face_idx,
                       float* normals_out) {
  const uint64_t z0 = rand64(seed, SAMPLE_STREAM, (uint64_t)i);
  const uint64_t z1 = rand64(seed, SAMPLE_STREAM + 1, (uint64_t)i);
  const uint64_t z2 = rand64(seed, SAMPLE_STREAM + 2, (uint64_t)i);
  int64_t f = upper_bound(cdf, F, (int64_t)umulhi64(z0, total));
  if (f > F - 1) f = F - 1;
  int64_t k1 = (int64_t)(z1 >> 40), k2 = (int64_t)(z2 >> 40);
  if (k1 + k2 > 16777216) k1 = 16777216 - k1, k2 = 16777216 - k2;
  const double u1 = (double)k1 * (1.0 / 16777216.0), u2 = (double)k2 * (1.0 / 16777216.0);  // exact
  const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  for (int c = 0; c < 3; ++c) {
    const double o = (double)p[3 * i0 + c];
    const double e1 = (double)p[3 * i1 + c] - o, e2 = (double)p[3 * i2 + c] - o;
    const double t1 = u1 * e1, t2 = u2 * e2;
    const double s = o + t1;
    points[3 * i + c] = (float)(s + t2);
  }
  face_idx[i] = (int32_t)f;
  if (!normals_out) return;
  double g[3], d;
  if (vertex_normals) {
    const double w0 = (1.0 - u1) - u2;  // exact: multiples of 2^-24 in [0, 1]
    for (int c = 0; c < 3; ++c) {
      const double t0 = w0 * (double)vertex_normals[3 * i0 + c];
      const double t1 = u1 * (double)vertex_normals[3 * i1 + c];
      const double t2 = u2 * (double)vertex_normals[3 * i2 + c];
      g[c] = (t0 + t1) + t2;
    }
    const double len = norm3(g);
    d = len > 1e-12 ? len : 1e-12;
  } else {
    face_cross(p, faces, f, g);
    d = norm3(g);  // > 0 for a face of positive weight; a zero cross product (possible only at the clamp) gives zeros
    if (!(d > 0.0)) d = 1.0;
  }
  for (int c = 0; c < 3; ++c) normals_out[3 * i + c] = (float)(g[c] / d);
}

// ---------------------------------------------------------------- the search

struct Best {
  float d2;
  int32_t idx;
};

// The nearest reference point of q.  Smaller d2 wins, and on equal d2 the smaller original index; idx == -1 compares
// as the largest index, so a first candidate with d2 == +inf is still taken, as brute force's argmin would.  The
// walk of a run is bounded by m.  m == 0: d2 = +inf, idx = -1.
NERF_MM_HD Best nearest(const Grid& g, const float q[3], const int64_t* keys, const float* sorted_points, int64_t m) {
  Best best = {INFINITY, -1};
  if (m <= 0) return best;
  nerf_grid::walk_shells(
      g, q, [&](int32_t r) { return shell_can_stop(best.d2, r, g.cell); },
      [&](int32_t ix, int32_t iy, int32_t z0, int32_t z1) {
        nerf_grid::for_run(g, keys, m, ix, iy, z0, z1, [&](int64_t j, int64_t, int32_t o) {
          const float dx = q[0] - sorted_points[3 * j], dy = q[1] - sorted_points[3 * j + 1],
                      dz = q[2] - sorted_points[3 * j + 2];
          const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
          const float d2 = (xx + yy) + zz;
          if (d2 < best.d2 || (d2 == best.d2 && (uint32_t)o < (uint32_t)best.idx)) best.d2 = d2, best.idx = o;
        });
      });
  return best;
}

}  // namespace nerf_mm
