// Mesh smoothing: the int64 keys of the two adjacencies, the run flags and the row build of their
// CSR form, one Jacobi smoothing pass and the area-weighted vertex normal, written once for the device and for a host
// compiler so that every loop can be run and checked under a host sanitizer without a GPU.
//
// A key is (row << 32) | entry with row, entry in [0, 2^31): non-negative, and ordered by (row, entry).  Sorted
// ascending, the first key of every run of equal keys is one CSR entry, the rows are contiguous, and row v starts at
// the lower bound of v << 32.  SENTINEL (INT64_MAX) marks a dropped pair; it sorts behind every key and is never an
// entry.  Build with -ffp-contract=off: every double operation below rounds on its own.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NERF_MS_HD __host__ __device__ __forceinline__
#else
#define NERF_MS_HD inline
#endif

namespace nerf_ms {

constexpr int64_t SENTINEL = INT64_MAX;

NERF_MS_HD int64_t pack(int32_t row, int32_t entry) {
  return (int64_t)(((uint64_t)(uint32_t)row << 32) | (uint64_t)(uint32_t)entry);
}
NERF_MS_HD int32_t key_row(int64_t key) { return (int32_t)((uint64_t)key >> 32); }
NERF_MS_HD int32_t key_entry(int64_t key) { return (int32_t)(uint32_t)((uint64_t)key & 0xffffffffu); }

// Key i of the 6 F directed pairs: face i / 6, edge (i % 6) / 2 from corner e to corner (e + 1) % 3, forwards for an
// even i and backwards for an odd one.  A pair (a, a) is the sentinel.
NERF_MS_HD int64_t pair_key(const int32_t* faces, int64_t i) {
  const int64_t f = i / 6;
  const int j = (int)(i - 6 * f), e = j >> 1;
  const int32_t a = faces[3 * f + e], b = faces[3 * f + (e == 2 ? 0 : e + 1)];
  if (a == b) return SENTINEL;
  return (j & 1) ? pack(b, a) : pack(a, b);
}

// Key i of the 3 F (vertex, face) pairs: corner i % 3 of face i / 3.
NERF_MS_HD int64_t vertex_face_key(const int32_t* faces, int64_t i) { return pack(faces[i], (int32_t)(i / 3)); }

// The first index in [0, n] whose key is >= target (n when there is none).  n < 2^31, so the interval is empty after
// at most 31 halvings; the trip count is bounded by 32 whatever the data.
NERF_MS_HD int64_t lower_bound(const int64_t* keys, int64_t n, int64_t target) {
  int64_t lo = 0, hi = n;
  for (int step = 0; step < 32 && lo < hi; ++step) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < target) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// 1 at the first key of every run of equal keys that is no sentinel
NERF_MS_HD int32_t run_flag(const int64_t* keys, int64_t i) {
  const int64_t k = keys[i];
  return k != SENTINEL && (i == 0 || k != keys[i - 1]);
}

// the run that starts at i (run_flag(keys, i) != 0) has exactly one key: a directed pair that one face emitted once
NERF_MS_HD bool run_is_single(const int64_t* keys, int64_t n, int64_t i) { return i + 1 >= n || keys[i + 1] != keys[i]; }

// row_off[v] for v in [0, V]: the position of the first entry whose row is >= v
NERF_MS_HD int32_t row_start(const int64_t* keys, int64_t n, const int32_t* pos, int64_t v) {
  return pos[lower_bound(keys, n, (int64_t)((uint64_t)v << 32))];
}

// One Jacobi step of vertex v: out = p[v] + s (mean of the row's vertices - p[v]) per axis, the sum taken in the
// row's order in double.  An empty row, a fixed vertex and s == 0 copy p[v] bit for bit (s == 0 is a case of its own
// because q + 0 * x turns q = -0 into +0).
NERF_MS_HD void smooth_vertex(const float* p, const int32_t* row_off, const int32_t* col, const uint8_t* fixed,
                              int64_t v, float s, float* out) {
  const int32_t b = row_off[v], e = row_off[v + 1];
  if (e <= b || s == 0.0f || (fixed && fixed[v])) {
    for (int c = 0; c < 3; ++c) out[3 * v + c] = p[3 * v + c];
    return;
  }
  const int64_t u0 = col[b];
  double acc[3] = {(double)p[3 * u0], (double)p[3 * u0 + 1], (double)p[3 * u0 + 2]};
  for (int32_t k = b + 1; k < e; ++k) {
    const int64_t u = col[k];
    for (int c = 0; c < 3; ++c) acc[c] = acc[c] + (double)p[3 * u + c];
  }
  const double d = (double)(e - b);
  for (int c = 0; c < 3; ++c) {
    const double m = acc[c] / d;
    const double q = (double)p[3 * v + c];
    const double diff = m - q;
    const double step = (double)s * diff;
    out[3 * v + c] = (float)(q + step);
  }
}

// The unit normal of vertex v: the sum, in the row's order, of the cross products (p[i1] - p[i0]) x (p[i2] - p[i0])
// of its faces (twice the area each, by the face's winding), normalised; a zero sum gives zeros.
NERF_MS_HD void vertex_normal(const float* p, const int32_t* faces, const int32_t* row_off, const int32_t* col,
                              int64_t v, float* out) {
  double g[3] = {0.0, 0.0, 0.0};
  for (int32_t k = row_off[v], e = row_off[v + 1]; k < e; ++k) {
    const int64_t f = col[k];
    const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    double a[3], b[3];
    for (int c = 0; c < 3; ++c) {
      const double o = (double)p[3 * i0 + c];
      a[c] = (double)p[3 * i1 + c] - o;
      b[c] = (double)p[3 * i2 + c] - o;
    }
    const double x0 = a[1] * b[2], x1 = a[2] * b[1];
    const double y0 = a[2] * b[0], y1 = a[0] * b[2];
    const double z0 = a[0] * b[1], z1 = a[1] * b[0];
    const double cx = x0 - x1, cy = y0 - y1, cz = z0 - z1;
    g[0] = g[0] + cx;
    g[1] = g[1] + cy;
    g[2] = g[2] + cz;
  }
  const double xx = g[0] * g[0], yy = g[1] * g[1], zz = g[2] * g[2];
  const double len = sqrt((xx + yy) + zz);
  const double d = len > 1e-12 ? len : 1e-12;
  for (int c = 0; c < 3; ++c) out[3 * v + c] = (float)(g[c] / d);
}

}  // namespace nerf_ms
