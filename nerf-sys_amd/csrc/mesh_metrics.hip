// Mesh metrics on the device (the shared core is mesh_metrics_core.hpp).
//
//   nerf_mesh_face_areas     one thread per face: half the length of the cross product of two edges, in double.
//   (the caller turns the areas into an integer CDF: a max, a scale by a power of two, rint, an int64 cumsum)
//   nerf_mesh_sample_surface one thread per sample: three counter random numbers, a bounded binary search of the CDF,
//                            an integer fold onto the triangle, the point (and a normal) in double.
//   nerf_points_cell_keys    one thread per point: (cell_id << 32) | index of the fp32 cell of the clustering grid.
//   (the caller sorts the keys ascending and gathers the points in key order)
//   nerf_points_nearest      one thread per query: Chebyshev shells around the query's cell, per column one lower
//                            bound over the sorted keys and a walk over the run; brute force's result bit for bit.
//
// No LDS, no atomics: every output element has one writer and is a function of the input alone.  The kernels do not
// check indices or finiteness: that is the caller's duty (kernels.py validates before launching).
#include "common.hpp"
#include "mesh_grid_host.hpp"
#include "mesh_metrics_core.hpp"

namespace {

constexpr int NTHREADS = 256;
using nerf_grid::aligned8;
using nerf_grid::LIMIT;
using nerf_grid::make_grid;

__global__ __launch_bounds__(NTHREADS) void face_areas_kernel(const float* __restrict__ verts,
                                                              const int32_t* __restrict__ faces, int64_t F,
                                                              double* __restrict__ area) {
  const int64_t f = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (f >= F) return;
  area[f] = nerf_mm::face_area(verts, faces, f);
}

__global__ __launch_bounds__(NTHREADS) void sample_surface_kernel(const float* __restrict__ verts,
                                                                  const int32_t* __restrict__ faces, int64_t F,
                                                                  const int64_t* __restrict__ cdf, uint64_t total,
                                                                  const float* __restrict__ vertex_normals, int64_t n,
                                                                  uint64_t seed, float* __restrict__ points,
                                                                  int32_t* __restrict__ face_idx,
                                                                  float* __restrict__ normals_out) {
  const int64_t i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (i >= n) return;
  nerf_mm::sample(verts, faces, F, cdf, total, vertex_normals, seed, i, points, face_idx, normals_out);
}

__global__ __launch_bounds__(NTHREADS) void cell_keys_kernel(const float* __restrict__ points, int64_t m,
                                                             nerf_mm::Grid g, int64_t* __restrict__ keys) {
  const int64_t j = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (j >= m) return;
  keys[j] = nerf_mm::point_key(g, points, j);
}

__global__ __launch_bounds__(NTHREADS) void nearest_kernel(const float* __restrict__ query, int64_t n,
                                                           const int64_t* __restrict__ keys,
                                                           const float* __restrict__ sorted_points, int64_t m,
                                                           nerf_mm::Grid g, float* __restrict__ d2,
                                                           int32_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (i >= n) return;
  const float q[3] = {query[3 * i], query[3 * i + 1], query[3 * i + 2]};
  const nerf_mm::Best best = nerf_mm::nearest(g, q, keys, sorted_points, m);
  d2[i] = best.d2;
  idx[i] = best.idx;
}

}  // namespace

extern "C" int nerf_mesh_face_areas(const float* vertices, const int32_t* faces, int64_t F, double* area,
                                    hipStream_t stream) {
  NERF_CHECK_ARG(F >= 0 && 3 * F < LIMIT);
  if (F == 0) return NERF_OK;
  NERF_CHECK_ARG(vertices && faces && area);
  if (!aligned8(area)) return NERF_E_ALIGN;
  face_areas_kernel<<<(unsigned)nerf_cdiv(F, NTHREADS), NTHREADS, 0, stream>>>(vertices, faces, F, area);
  return nerf_launch_status();
}

extern "C" int nerf_mesh_sample_surface(const float* vertices, const int32_t* faces, int64_t F, const int64_t* cdf,
                                        uint64_t total, const float* vertex_normals, int64_t n, uint64_t seed,
                                        float* points, int32_t* face_idx, float* normals_out, hipStream_t stream) {
  NERF_CHECK_ARG(n >= 0 && n < LIMIT && F >= 0 && 3 * F < LIMIT);
  if (n == 0) return NERF_OK;
  NERF_CHECK_ARG(F > 0 && total > 0 && total < (uint64_t(1) << 63));
  NERF_CHECK_ARG(vertices && faces && cdf && points && face_idx);
  NERF_CHECK_ARG(!(vertex_normals && !normals_out));
  if (!aligned8(cdf)) return NERF_E_ALIGN;
  sample_surface_kernel<<<(unsigned)nerf_cdiv(n, NTHREADS), NTHREADS, 0, stream>>>(
      vertices, faces, F, cdf, total, vertex_normals, n, seed, points, face_idx, normals_out);
  return nerf_launch_status();
}

extern "C" int nerf_points_cell_keys(const float* points, int64_t m, const float* lo, float inv, const int32_t* dims,
                                     int64_t* keys, hipStream_t stream) {
  nerf_mm::Grid g;
  NERF_CHECK_ARG(m >= 0 && m < LIMIT && make_grid(lo, 1.0f, inv, dims, g));  // the keys do not use the cell itself
  if (m == 0) return NERF_OK;
  NERF_CHECK_ARG(points && keys);
  if (!aligned8(keys)) return NERF_E_ALIGN;
  cell_keys_kernel<<<(unsigned)nerf_cdiv(m, NTHREADS), NTHREADS, 0, stream>>>(points, m, g, keys);
  return nerf_launch_status();
}

extern "C" int nerf_points_nearest(const float* query, int64_t n, const int64_t* sorted_keys,
                                   const float* sorted_points, int64_t m, const float* lo, float cell, float inv,
                                   const int32_t* dims, float* d2, int32_t* idx, hipStream_t stream) {
  nerf_mm::Grid g;
  NERF_CHECK_ARG(n >= 0 && n < LIMIT && m >= 0 && m < LIMIT && make_grid(lo, cell, inv, dims, g));
  if (n == 0) return NERF_OK;
  NERF_CHECK_ARG(query && d2 && idx && (m == 0 || (sorted_keys && sorted_points)));
  if (m && !aligned8(sorted_keys)) return NERF_E_ALIGN;
  nearest_kernel<<<(unsigned)nerf_cdiv(n, NTHREADS), NTHREADS, 0, stream>>>(query, n, sorted_keys, sorted_points, m, g,
                                                                           d2, idx);
  return nerf_launch_status();
}
