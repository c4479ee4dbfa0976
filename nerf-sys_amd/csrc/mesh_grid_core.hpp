// The sorted-key uniform grid of the mesh queries: the cell of a coordinate, the
// keys of a point and of a face, the walk over the keys of a run of cells, the walk over the Chebyshev shells around a
// query and the rule that ends it, and the small vector helpers the queries share, written once for the device and
// for a host compiler so that every loop can be run and checked under a host sanitizer without a GPU.
// Build with -ffp-contract=off: every fp32 and fp64 operation below rounds on its own.
//
// The grid.  An item (a reference point j, or a face f) is binned by the fp32 cell index of the vertex clustering,
// t = (p - lo) * inv, i = clamp(floorf(t), 0, dim - 1), every dim in [1, 1024]; key = (cell_id << 32) | item with
// cell_id = (ix ny + iy) nz + iz < 2^30.  A point has the one key of its cell.  A face is registered in every cell of
// the index box [cell_index(min corner), cell_index(max corner)] of its bounding box (fminf / fmaxf over its three
// corners, per axis).  Sorted ascending, the items of a cell are contiguous and ascending by index and the cells of
// one (ix, iy) column are contiguous in iz, so a run of cells of one column starts at the lower bound of its first
// cell_id << 32: no cell table (for_run).
//
// The search.  A query walks the Chebyshev shells r = 0, 1, 2, ... around its own clamped cell (walk_shells) and stops
// before shell r >= 2 when shell_can_stop holds for the best squared distance found so far (a face search rounds it UP
// to fp32 first), that is when
//
//     best_d2 <= ((r - 1 - 2^-8) cell)^2 (1 - 2^-10).
//
// Why that is safe, as far as both searches share it.  Every reference point or vertex must lie in the box
// [lo, lo + dims cell] up to rounding (the caller builds the grid from the points' or vertices' own minimum and
// maximum).  Let s = (x - lo) / cell be the real cell coordinate and t its fp32 value.  t carries three relative errors
// of at most 2^-24 each: the subtraction, the product, and inv against 1 / cell (inv = fl(1 / cell), the caller's one
// division).  With s <= 1024 (+ the same error) that is |t - s| < 3 2^-24 1025 < 2^-12 =: delta of a cell, which is
// where the cap of 1024 cells per axis comes from.  So a point whose computed cell is i has s in
// [i - delta, i + 1 + delta]; the upper clamp only moves a point at s = dim into cell dim - 1, which that interval
// already covers.  The fp32 cell_index is monotone in the coordinate (a difference, a product, a floor and a clamp,
// each monotone), and every real point of a face has each coordinate between the smallest and the largest of its
// corners, so it computes a cell index between the two ends of the face's index box: every real point of the face
// lies in its registered cells widened by delta.
// The box-separation step.  Before shell r the cells of the cube of Chebyshev radius r - 1 around the query's clamped
// cell, clipped to the grid, have all been searched.  An item that has not been evaluated is registered in none of
// them; its registered cells form a box (one cell for a point), the cube is a box, and two disjoint boxes of cells are
// separated along one axis: on that axis every registered cell of the item differs from the query's cell by at least
// r (a point of a shell >= r differs from the query's cell by at least r cells on some axis).  The query lies in its
// own cell widened by delta, so on that axis the real gap is at least (r - 1 - 2 delta) cell > (r - 1 - 2^-11) cell.
// A query outside the box is clamped into a border cell; its real gap to every cell is then larger than that of a
// query inside the border cell, so the bound holds a fortiori.  Hence the real distance from the query to any point
// of an unevaluated item is at least (r - 1 - 2^-11) cell.
// The slack kept in hand.  The rule leaves 2^-8 - 2^-11 of a cell, and 2^-10 relative less what the evaluated d2 can
// fall short of the real squared distance by; that last bound is each search's own (mesh_metrics_core.hpp for the
// fp32 point distance, mesh_distance_core.hpp for the double face distance).  The rule is evaluated in double, whose
// own rounding is 2^-53.  When it fires, every unsearched item is strictly farther than the best, so neither the
// distance nor the smallest-index tie-break can change.  The result is brute force's, bit for bit.  Tighten the
// slack only with an argument.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NERF_GRID_HD __host__ __device__ __forceinline__
#else
#define NERF_GRID_HD inline
#endif

namespace nerf_grid {

// ---------------------------------------------------------------- vectors and corners

NERF_GRID_HD double dot3(const double a[3], const double b[3]) {
  const double x = a[0] * b[0], y = a[1] * b[1], z = a[2] * b[2];
  return (x + y) + z;
}

// a x b: the six products and the three differences of products each rounded once
NERF_GRID_HD void cross3(const double a[3], const double b[3], double c[3]) {
  const double x0 = a[1] * b[2], x1 = a[2] * b[1];
  const double y0 = a[2] * b[0], y1 = a[0] * b[2];
  const double z0 = a[0] * b[1], z1 = a[1] * b[0];
  c[0] = x0 - x1;
  c[1] = y0 - y1;
  c[2] = z0 - z1;
}

struct Corners {
  float a[3], b[3], c[3];
};

NERF_GRID_HD Corners load_corners(const float* verts, const int32_t* faces, int64_t f) {
  const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  Corners t;
  for (int k = 0; k < 3; ++k) {
    t.a[k] = verts[3 * i0 + k];
    t.b[k] = verts[3 * i1 + k];
    t.c[k] = verts[3 * i2 + k];
  }
  return t;
}

// ---------------------------------------------------------------- cells and keys

constexpr int32_t MAX_DIM = 1024;

struct Grid {
  float lo[3];
  float cell, inv;
  int32_t dims[3];
};

// x >= a ? (x <= b ? x : b) : a: a NaN counts as the lower bound
NERF_GRID_HD float clampf(float x, float a, float b) { return x >= a ? (x <= b ? x : b) : a; }

// t = (x - lo) * inv: the coordinate x on axis c in cells, as computed
NERF_GRID_HD float cell_coord(const Grid& g, int c, float x) { return (x - g.lo[c]) * g.inv; }

// the fp32 cell index of coordinate x on axis c: clamped as a float, then converted
NERF_GRID_HD int32_t cell_index(const Grid& g, int c, float x) {
  return (int32_t)clampf(floorf(cell_coord(g, c, x)), 0.0f, (float)(g.dims[c] - 1));
}

NERF_GRID_HD int64_t cell_id(const Grid& g, int32_t ix, int32_t iy, int32_t iz) {
  return ((int64_t)ix * g.dims[1] + iy) * g.dims[2] + iz;
}

// key = (cell_id << 32) | item, and its two halves
NERF_GRID_HD int64_t make_key(int64_t cell, uint32_t item) {
  return (int64_t)(((uint64_t)cell << 32) | (uint64_t)item);
}
NERF_GRID_HD int64_t key_cell(int64_t key) { return key >> 32; }
NERF_GRID_HD int32_t key_item(int64_t key) { return (int32_t)(uint32_t)((uint64_t)key & 0xffffffffu); }

NERF_GRID_HD int64_t point_key(const Grid& g, const float* points, int64_t j) {
  const int32_t ix = cell_index(g, 0, points[3 * j]), iy = cell_index(g, 1, points[3 * j + 1]),
                iz = cell_index(g, 2, points[3 * j + 2]);
  return make_key(cell_id(g, ix, iy, iz), (uint32_t)j);
}

// the index box of face f: lo[c] <= hi[c] because cell_index is monotone
NERF_GRID_HD void face_box(const Grid& g, const float* p, const int32_t* faces, int64_t f, int32_t lo[3],
                           int32_t hi[3]) {
  const Corners t = load_corners(p, faces, f);
  for (int c = 0; c < 3; ++c) {
    lo[c] = cell_index(g, c, fminf(fminf(t.a[c], t.b[c]), t.c[c]));
    hi[c] = cell_index(g, c, fmaxf(fmaxf(t.a[c], t.b[c]), t.c[c]));
  }
}

// the number of cells face f is registered in: at most 1024^3 = 2^30
NERF_GRID_HD int64_t face_cell_count(const Grid& g, const float* p, const int32_t* faces, int64_t f) {
  int32_t lo[3], hi[3];
  face_box(g, p, faces, f, lo, hi);
  return ((int64_t)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1)) * (hi[2] - lo[2] + 1);
}

// the keys of face f, face_cell_count of them, in ascending cell_id order; every loop is bounded by a dim
NERF_GRID_HD void face_keys(const Grid& g, const float* p, const int32_t* faces, int64_t f, int64_t* out) {
  int32_t lo[3], hi[3];
  face_box(g, p, faces, f, lo, hi);
  int64_t at = 0;
  for (int32_t ix = lo[0]; ix <= hi[0]; ++ix)
    for (int32_t iy = lo[1]; iy <= hi[1]; ++iy)
      for (int32_t iz = lo[2]; iz <= hi[2]; ++iz) out[at++] = make_key(cell_id(g, ix, iy, iz), (uint32_t)f);
}

// ---------------------------------------------------------------- the walks

// The first index in [0, n] whose key is >= target (n when there is none); n < 2^31, at most 32 trips.
NERF_GRID_HD int64_t lower_bound(const int64_t* keys, int64_t n, int64_t target) {
  int64_t lo = 0, hi = n;
  for (int step = 0; step < 32 && lo < hi; ++step) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < target) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// The keys of the cells (ix, iy, z0 .. z1) of one column, in order: one lower bound, then a walk over the run (at most
// n keys), visit(j, cell_id, item) for the key at sorted position j.
template <class Visit>
NERF_GRID_HD void for_run(const Grid& g, const int64_t* keys, int64_t n, int32_t ix, int32_t iy, int32_t z0, int32_t z1,
                          Visit visit) {
  const int64_t first = make_key(cell_id(g, ix, iy, z0), 0);
  const int64_t end = make_key(cell_id(g, ix, iy, z1) + 1, 0);
  for (int64_t j = lower_bound(keys, n, first); j < n; ++j) {
    const int64_t key = keys[j];
    if (key >= end) break;
    visit(j, key_cell(key), key_item(key));
  }
}

// the rule of the header comment, in double
NERF_GRID_HD bool shell_can_stop(float best_d2, int32_t r, float cell) {
  const double b = ((double)(r - 1) - 0.00390625) * (double)cell;
  return (double)best_d2 <= (b * b) * (1.0 - 0.0009765625);
}

// The cells around q, shell by shell, until stop(r) holds before a shell r >= 2 or the grid is exhausted:
// scan(ix, iy, z0, z1) for every run of cells.  Shell r: the columns on the rim of the (2r+1)^2 square are searched
// over their whole clipped iz range with one run; an inner column contributes only its two cap cells cz - r and
// cz + r, two runs and so two lower bounds.  The shell loop is bounded by max(dims), the column loops by the dims.
template <class Stop, class Scan>
NERF_GRID_HD void walk_shells(const Grid& g, const float q[3], Stop stop, Scan scan) {
  const int32_t nx = g.dims[0], ny = g.dims[1], nz = g.dims[2];
  const int32_t cx = cell_index(g, 0, q[0]), cy = cell_index(g, 1, q[1]), cz = cell_index(g, 2, q[2]);
  const int32_t shells = nx > ny ? (nx > nz ? nx : nz) : (ny > nz ? ny : nz);
  for (int32_t r = 0; r < shells; ++r) {
    if (r >= 2 && stop(r)) break;
    if (cx - r < 0 && cx + r > nx - 1 && cy - r < 0 && cy + r > ny - 1 && cz - r < 0 && cz + r > nz - 1)
      break;  // this shell and every later one lie outside the grid: every cell has been searched
    const int32_t x0 = cx - r > 0 ? cx - r : 0, x1 = cx + r < nx - 1 ? cx + r : nx - 1;
    const int32_t y0 = cy - r > 0 ? cy - r : 0, y1 = cy + r < ny - 1 ? cy + r : ny - 1;
    const int32_t z0 = cz - r > 0 ? cz - r : 0, z1 = cz + r < nz - 1 ? cz + r : nz - 1;
    for (int32_t ix = x0; ix <= x1; ++ix) {
      const bool rim_x = ix == cx - r || ix == cx + r;
      for (int32_t iy = y0; iy <= y1; ++iy) {
        if (rim_x || iy == cy - r || iy == cy + r) {
          scan(ix, iy, z0, z1);
        } else {
          if (cz - r >= 0) scan(ix, iy, cz - r, cz - r);
          if (cz + r <= nz - 1) scan(ix, iy, cz + r, cz + r);
        }
      }
    }
  }
}

}  // namespace nerf_grid
