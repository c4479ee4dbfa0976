// Mesh metrics: the counter random numbers, the face area, the area-weighted surface sampler, the
// cell keys of a point set and the exact nearest-neighbour search through a uniform grid, written once for the device
// and for a host compiler so that every loop can be run and checked under a host sanitizer without a GPU.
// Build with -ffp-contract=off: every fp32 and fp64 operation below rounds on its own.
//
// The grid and the search.  The reference points P are binned by the fp32 cell index of the vertex clustering,
// t = (p - lo) * inv, i = clamp(floorf(t), 0, dim - 1), every dim in [1, 1024]; key = (cell_id << 32) | j with
// cell_id = (ix ny + iy) nz + iz < 2^30.  Sorted ascending, the points of a cell are contiguous and ascending by j and
// the cells of one (ix, iy) column are contiguous in iz, so a run of cells of one column starts at the lower bound of
// its first cell_id << 32: no cell table.  A query walks the Chebyshev shells r = 0, 1, 2, ... around its own clamped
// cell and stops before shell r >= 2 when
//
//     best_d2 <= ((r - 1 - 2^-8) cell)^2 (1 - 2^-10).
//
// Why that is safe.  Every reference point must lie in the box [lo, lo + dims cell] up to rounding (the caller builds
// the grid from the points' own minimum and maximum).  Let s = (x - lo) / cell be the real cell coordinate and t its
// fp32 value.  t carries three relative errors of at most 2^-24 each: the subtraction, the product, and inv against
// 1 / cell (inv = fl(1 / cell), the caller's one division).  With s <= 1024 (+ the same error) that is
// |t - s| < 3 2^-24 1025 < 2^-12 =: delta of a cell, which is where the cap of 1024 cells per axis comes from.  So a
// point whose computed cell is i has s in [i - delta, i + 1 + delta]; the upper clamp only moves a point at s = dim
// into cell dim - 1, which that interval already covers.  A point of a shell >= r differs from the query's cell by at
// least r cells on some axis, so on that axis the real gap is at least (r - 1 - 2 delta) cell > (r - 1 - 2^-11) cell.
// A query outside the box is clamped into a border cell; its real gap to every cell is then larger than that of a
// query inside the border cell, so the bound holds a fortiori.  The fp32 distance d2 = (dx dx + dy dy) + dz dz
// carries at most five roundings of 2^-24 each against the real squared distance (one per difference, squared, one
// per product, two sums), and every fp32 operation is monotone, so the d2 of an unsearched point is at least
// ((r - 1 - 2^-11) cell)^2 (1 - 2^-21).  The rule leaves 2^-8 - 2^-11 of a cell and 2^-10 - 2^-21 relative in hand
// (it is evaluated in double, whose own rounding is 2^-53): when it fires, every unsearched point is strictly
// farther than the best, so neither the distance nor the smallest-index tie-break can change.  The result is brute
// force's, bit for bit.  Tighten the slack only with an argument.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NERF_MM_HD __host__ __device__ __forceinline__
#else
#define NERF_MM_HD inline
#endif

namespace nerf_mm {

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
  const double x0 = a[1] * b[2], x1 = a[2] * b[1];
  const double y0 = a[2] * b[0], y1 = a[0] * b[2];
  const double z0 = a[0] * b[1], z1 = a[1] * b[0];
  c[0] = x0 - x1;
  c[1] = y0 - y1;
  c[2] = z0 - z1;
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

// ---------------------------------------------------------------- the grid

constexpr int32_t MAX_DIM = 1024;

struct Grid {
  float lo[3];
  float cell, inv;
  int32_t dims[3];
};

// x >= a ? (x <= b ? x : b) : a: a NaN counts as the lower bound
NERF_MM_HD float clampf(float x, float a, float b) { return x >= a ? (x <= b ? x : b) : a; }

// the fp32 cell index of nerf_mesh_cluster_labels (mesh_simplify_core.hpp): clamped as a float, then converted
NERF_MM_HD int32_t cell_index(const Grid& g, int c, float x) {
  const float t = (x - g.lo[c]) * g.inv;
  return (int32_t)clampf(floorf(t), 0.0f, (float)(g.dims[c] - 1));
}

NERF_MM_HD int64_t cell_id(const Grid& g, int32_t ix, int32_t iy, int32_t iz) {
  return ((int64_t)ix * g.dims[1] + iy) * g.dims[2] + iz;
}

NERF_MM_HD int64_t point_key(const Grid& g, const float* points, int64_t j) {
  const int32_t ix = cell_index(g, 0, points[3 * j]), iy = cell_index(g, 1, points[3 * j + 1]),
                iz = cell_index(g, 2, points[3 * j + 2]);
  return (int64_t)(((uint64_t)cell_id(g, ix, iy, iz) << 32) | (uint64_t)(uint32_t)j);
}

// The first index in [0, n] whose key is >= target (n when there is none); n < 2^31, at most 32 trips.
NERF_MM_HD int64_t lower_bound(const int64_t* keys, int64_t n, int64_t target) {
  int64_t lo = 0, hi = n;
  for (int step = 0; step < 32 && lo < hi; ++step) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < target) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

struct Best {
  float d2;
  int32_t idx;
};

// The points of the cells (ix, iy, z0 .. z1) of one column: one lower bound, then a walk over the run (at most m
// points).  Smaller d2 wins, and on equal d2 the smaller original index; idx == -1 compares as the largest index, so
// a first candidate with d2 == +inf is still taken, as brute force's argmin would.
NERF_MM_HD void scan_run(const Grid& g, const float q[3], const int64_t* keys, const float* sorted_points, int64_t m,
                         int32_t ix, int32_t iy, int32_t z0, int32_t z1, Best& best) {
  const int64_t first = (int64_t)((uint64_t)cell_id(g, ix, iy, z0) << 32);
  const int64_t end = (int64_t)((uint64_t)(cell_id(g, ix, iy, z1) + 1) << 32);
  for (int64_t j = lower_bound(keys, m, first); j < m; ++j) {
    const int64_t key = keys[j];
    if (key >= end) break;
    const float dx = q[0] - sorted_points[3 * j], dy = q[1] - sorted_points[3 * j + 1],
                dz = q[2] - sorted_points[3 * j + 2];
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const float d2 = (xx + yy) + zz;
    const int32_t o = (int32_t)(uint32_t)((uint64_t)key & 0xffffffffu);
    if (d2 < best.d2 || (d2 == best.d2 && (uint32_t)o < (uint32_t)best.idx)) best.d2 = d2, best.idx = o;
  }
}

// the rule of the header comment, in double
NERF_MM_HD bool shell_can_stop(float best_d2, int32_t r, float cell) {
  const double b = ((double)(r - 1) - 0.00390625) * (double)cell;
  return (double)best_d2 <= (b * b) * (1.0 - 0.0009765625);
}

// The nearest reference point of q.  Shell r: the columns on the rim of the (2r+1)^2 square are searched over their
// whole clipped iz range with one lower bound; an inner column contributes only its two cap cells cz - r and cz + r,
// two runs and so two lower bounds.  The shell loop is bounded by max(dims), the column loops by the dims, the walk
// by m.  m == 0: d2 = +inf, idx = -1.
NERF_MM_HD Best nearest(const Grid& g, const float q[3], const int64_t* keys, const float* sorted_points, int64_t m) {
  Best best = {INFINITY, -1};
  if (m <= 0) return best;
  const int32_t nx = g.dims[0], ny = g.dims[1], nz = g.dims[2];
  const int32_t cx = cell_index(g, 0, q[0]), cy = cell_index(g, 1, q[1]), cz = cell_index(g, 2, q[2]);
  const int32_t shells = nx > ny ? (nx > nz ? nx : nz) : (ny > nz ? ny : nz);
  for (int32_t r = 0; r < shells; ++r) {
    if (r >= 2 && shell_can_stop(best.d2, r, g.cell)) break;
    if (cx - r < 0 && cx + r > nx - 1 && cy - r < 0 && cy + r > ny - 1 && cz - r < 0 && cz + r > nz - 1)
      break;  // this shell and every later one lie outside the grid: every cell has been searched
    const int32_t x0 = cx - r > 0 ? cx - r : 0, x1 = cx + r < nx - 1 ? cx + r : nx - 1;
    const int32_t y0 = cy - r > 0 ? cy - r : 0, y1 = cy + r < ny - 1 ? cy + r : ny - 1;
    const int32_t z0 = cz - r > 0 ? cz - r : 0, z1 = cz + r < nz - 1 ? cz + r : nz - 1;
    for (int32_t ix = x0; ix <= x1; ++ix) {
      const bool rim_x = ix == cx - r || ix == cx + r;
      for (int32_t iy = y0; iy <= y1; ++iy) {
        if (rim_x || iy == cy - r || iy == cy + r) {
          scan_run(g, q, keys, sorted_points, m, ix, iy, z0, z1, best);
        } else {
          if (cz - r >= 0) scan_run(g, q, keys, sorted_points, m, ix, iy, cz - r, cz - r, best);
          if (cz + r <= nz - 1) scan_run(g, q, keys, sorted_points, m, ix, iy, cz + r, cz + r, best);
        }
      }
    }
  }
  return best;
}

}  // namespace nerf_mm
