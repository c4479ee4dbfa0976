// Exact point-to-surface distance on the device (the shared core is mesh_distance_core.hpp).
//
//   nerf_mesh_face_cell_counts  one thread per face: the number of cells of the face's index box.
//   (the caller turns the counts into offsets with an exclusive int64 cumsum and reads the total)
//   nerf_mesh_face_cell_keys    one thread per face: (cell_id << 32) | face for every cell of the box, at offsets[f].
//   (the caller sorts the keys ascending)
//   nerf_mesh_nearest_faces     one thread per query: Chebyshev shells around the query's cell, per column one lower
//                               bound over the sorted keys and a walk over the run, every face of the run measured
//                               in double; brute force's result bit for bit.
//
// No LDS, no atomics: every output element has one writer and is a function of the input alone.  The kernels do not
// check indices or finiteness: that is the caller's duty (kernels.py validates before launching).
#include "common.hpp"
#include "mesh_grid_host.hpp"
#include "mesh_distance_core.hpp"

namespace {

constexpr int NTHREADS = 256;
using nerf_grid::aligned8;
using nerf_grid::LIMIT;
using nerf_grid::make_grid;

__global__ __launch_bounds__(NTHREADS) void face_cell_counts_kernel(const float* __restrict__ verts,
                                                                    const int32_t* __restrict__ faces, int64_t F,
                                                                    nerf_mm::Grid g, int64_t* __restrict__ counts) {
  const int64_t f = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (f >= F) return;
  counts[f] = nerf_md::face_cell_count(g, verts, faces, f);
}

__global__ __launch_bounds__(NTHREADS) void face_cell_keys_kernel(const float* __restrict__ verts,
                                                                  const int32_t* __restrict__ faces, int64_t F,
                                                                  nerf_mm::Grid g, const int64_t* __restrict__ offsets,
                                                                  int64_t* __restrict__ keys) {
  const int64_t f = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (f >= F) return;
  nerf_md::face_keys(g, verts, faces, f, keys + offsets[f]);
}

__global__ __launch_bounds__(NTHREADS) void nearest_faces_kernel(const float* __restrict__ query, int64_t n,
                                                                 const int64_t* __restrict__ keys, int64_t n_keys,
                                                                 const float* __restrict__ verts,
                                                                 const int32_t* __restrict__ faces, nerf_mm::Grid g,
                                                                 double* __restrict__ d2, int32_t* __restrict__ face,
                                                                 float* __restrict__ closest) {
  const int64_t i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (i >= n) return;
  const float q[3] = {query[3 * i], query[3 * i + 1], query[3 * i + 2]};
  const nerf_md::BestFace best = nerf_md::nearest_face(g, q, keys, n_keys, verts, faces);
  d2[i] = best.d2;
  face[i] = best.face;
  if (closest) {
    closest[3 * i] = best.p[0];
    closest[3 * i + 1] = best.p[1];
    closest[3 * i + 2] = best.p[2];
  }
}

}  // namespace

extern "C" int nerf_mesh_face_cell_counts(const float* vertices, const int32_t* faces, int64_t F, const float* lo,
                                          float inv, const int32_t* dims, int64_t* counts, hipStream_t stream) {
  nerf_mm::Grid g;
  NERF_CHECK_ARG(F >= 0 && 3 * F < LIMIT && make_grid(lo, 1.0f, inv, dims, g));  // the keys do not use the cell itself
  if (F == 0) return NERF_OK;
  NERF_CHECK_ARG(vertices && faces && counts);
  if (!aligned8(counts)) return NERF_E_ALIGN;
  face_cell_counts_kernel<<<(unsigned)nerf_cdiv(F, NTHREADS), NTHREADS, 0, stream>>>(vertices, faces, F, g, counts);
  return nerf_launch_status();
}

extern "C" int nerf_mesh_face_cell_keys(const float* vertices, const int32_t* faces, int64_t F, const float* lo,
                                        float inv, const int32_t* dims, const int64_t* offsets, int64_t* keys,
                                        hipStream_t stream) {
  nerf_mm::Grid g;
  NERF_CHECK_ARG(F >= 0 && 3 * F < LIMIT && make_grid(lo, 1.0f, inv, dims, g));
  if (F == 0) return NERF_OK;
  NERF_CHECK_ARG(vertices && faces && offsets && keys);
  if (!aligned8(offsets) || !aligned8(keys)) return NERF_E_ALIGN;
  face_cell_keys_kernel<<<(unsigned)nerf_cdiv(F, NTHREADS), NTHREADS, 0, stream>>>(vertices, faces, F, g, offsets, keys);
  return nerf_launch_status();
}

extern "C" int nerf_mesh_nearest_faces(const float* query, int64_t n, const int64_t* sorted_keys, int64_t n_keys,
                                       const float* vertices, const int32_t* faces, int64_t F, const float* lo,
                                       float cell, float inv, const int32_t* dims, double* d2, int32_t* face,
                                       float* closest, hipStream_t stream) {
  nerf_mm::Grid g;
  NERF_CHECK_ARG(n >= 0 && n < LIMIT && n_keys >= 0 && n_keys < LIMIT && F >= 0 && 3 * F < LIMIT &&
                 make_grid(lo, cell, inv, dims, g));
  if (n == 0) return NERF_OK;
  NERF_CHECK_ARG(query && d2 && face && (n_keys == 0 || (sorted_keys && vertices && faces && F > 0)));
  if (!aligned8(d2) || (n_keys && !aligned8(sorted_keys))) return NERF_E_ALIGN;
  nearest_faces_kernel<<<(unsigned)nerf_cdiv(n, NTHREADS), NTHREADS, 0, stream>>>(query, n, sorted_keys, n_keys, vertices,
                                                                                 faces, g, d2, face, closest);
  return nerf_launch_status();
}
