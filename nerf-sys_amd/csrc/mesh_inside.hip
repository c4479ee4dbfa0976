// Point-in-mesh crossing counts and box points on the device (the shared core is
// mesh_inside_core.hpp).
//
//   nerf_mesh_point_crossings  one thread per query: the column of the query's cell is read from the query's own cell
//                              upwards by one lower bound over the sorted keys, every face is tested once, at the key
//                              of its lowest cell at or above the query's, by exact fp32 box compares, an exact
//                              orientation of the projection (a floating filter, then a Shewchuk expansion in six
//                              registers) and a rounded-double side of the plane; brute force's counts bit for bit.
//   nerf_box_points            one thread per point: three counter random numbers, lo + u (hi - lo) in fp32.
//
// No LDS, no atomics: every output element has one writer and is a function of the input alone.  The kernels do not
// check indices or finiteness: that is the caller's duty (kernels.py validates before launching).
#include "common.hpp"
#include "mesh_grid_host.hpp"
#include "mesh_inside_core.hpp"

namespace {

constexpr int NTHREADS = 256;
using nerf_grid::aligned8;
using nerf_grid::LIMIT;
using nerf_grid::make_grid;

__global__ __launch_bounds__(NTHREADS) void point_crossings_kernel(const float* __restrict__ query, int64_t n,
                                                                   const int64_t* __restrict__ keys, int64_t n_keys,
                                                                   const float* __restrict__ verts,
                                                                   const int32_t* __restrict__ faces, nerf_mm::Grid g,
                                                                   int32_t* __restrict__ crossings,
                                                                   int32_t* __restrict__ winding) {
  const int64_t i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (i >= n) return;
  const float q[3] = {query[3 * i], query[3 * i + 1], query[3 * i + 2]};
  const nerf_mi::Count c = nerf_mi::count_crossings(g, q, keys, n_keys, verts, faces);
  crossings[i] = c.crossings;
  winding[i] = c.winding;
}

struct Box {
  float lo[3], hi[3];
};

__global__ __launch_bounds__(NTHREADS) void box_points_kernel(int64_t n, uint64_t seed, Box box,
                                                              float* __restrict__ points) {
  const int64_t i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (i >= n) return;
  nerf_mi::box_point(seed, i, box.lo, box.hi, points);
}

}  // namespace

extern "C" int nerf_mesh_point_crossings(const float* query, int64_t n, const int64_t* sorted_keys, int64_t n_keys,
                                         const float* vertices, const int32_t* faces, int64_t F, const float* lo,
                                         float cell, float inv, const int32_t* dims, int32_t* crossings,
                                         int32_t* winding, hipStream_t stream) {
  nerf_mm::Grid g;
  NERF_CHECK_ARG(n >= 0 && n < LIMIT && n_keys >= 0 && n_keys < LIMIT && F >= 0 && 3 * F < LIMIT &&
                 make_grid(lo, cell, inv, dims, g));
  if (n == 0) return NERF_OK;
  NERF_CHECK_ARG(query && crossings && winding && (n_keys == 0 || (sorted_keys && vertices && faces && F > 0)));
  if (n_keys && !aligned8(sorted_keys)) return NERF_E_ALIGN;
  point_crossings_kernel<<<(unsigned)nerf_cdiv(n, NTHREADS), NTHREADS, 0, stream>>>(query, n, sorted_keys, n_keys,
                                                                                   vertices, faces, g, crossings, winding);
  return nerf_launch_status();
}

extern "C" int nerf_box_points(int64_t n, uint64_t seed, const float* lo, const float* hi, float* points,
                               hipStream_t stream) {
  NERF_CHECK_ARG(n >= 0 && n < LIMIT && lo && hi);
  Box box;
  for (int c = 0; c < 3; ++c) {
    NERF_CHECK_ARG(isfinite(lo[c]) && isfinite(hi[c]) && lo[c] <= hi[c] && isfinite(hi[c] - lo[c]));
    box.lo[c] = lo[c];
    box.hi[c] = hi[c];
  }
  if (n == 0) return NERF_OK;
  NERF_CHECK_ARG(points);
  box_points_kernel<<<(unsigned)nerf_cdiv(n, NTHREADS), NTHREADS, 0, stream>>>(n, seed, box, points);
  return nerf_launch_status();
}
