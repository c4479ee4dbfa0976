// Nearest-hit ray casting against a mesh on the device (the shared core is mesh_raycast_core.hpp).
//
//   nerf_mesh_ray_cast  one thread per ray: the ray is clipped to the face grid's box, the layers of cells along its
//                       major axis are walked in its direction, per layer at most 3 x 3 cells are read by a lower
//                       bound over the sorted keys and every face of their runs is tested in double; brute force's
//                       result bit for bit.
//
// No LDS, no atomics: every output element has one writer and is a function of the input alone.  The kernel does not
// check indices or finiteness: that is the caller's duty (kernels.py validates before launching).
#include "common.hpp"
#include "mesh_grid_host.hpp"
#include "mesh_raycast_core.hpp"

namespace {

constexpr int NTHREADS = 256;
using nerf_grid::aligned8;
using nerf_grid::LIMIT;
using nerf_grid::make_grid;

__global__ __launch_bounds__(NTHREADS) void ray_cast_kernel(const float* __restrict__ rays, int64_t n,
                                                            const int64_t* __restrict__ keys, int64_t n_keys,
                                                            const float* __restrict__ verts,
                                                            const int32_t* __restrict__ faces, int64_t F,
                                                            nerf_mm::Grid g, double margin, bool cull,
                                                            double* __restrict__ t, int32_t* __restrict__ face,
                                                            float* __restrict__ bary) {
  const int64_t i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (i >= n) return;
  const nerf_mr::Ray r = nerf_mr::load_ray(rays, i);
  const nerf_mr::Hit best = nerf_mr::cast(g, r, keys, n_keys, verts, faces, F, margin, cull);
  t[i] = best.t;
  face[i] = best.face;
  bary[2 * i] = best.u;
  bary[2 * i + 1] = best.v;
}

}  // namespace

extern "C" int nerf_mesh_ray_cast(const float* rays, int64_t n, const int64_t* sorted_keys, int64_t n_keys,
                                  const float* vertices, const int32_t* faces, int64_t F, const float* lo, float cell,
                                  float inv, const int32_t* dims, double margin, int cull, double* t, int32_t* face,
                                  float* bary, hipStream_t stream) {
  nerf_mm::Grid g;
  NERF_CHECK_ARG(n >= 0 && n < LIMIT && n_keys >= 0 && n_keys < LIMIT && F >= 0 && 3 * F < LIMIT &&
                 make_grid(lo, cell, inv, dims, g));
  NERF_CHECK_ARG(margin >= 0.0 && margin <= 0.0009765625 * (double)cell && (cull == 0 || cull == 1));
  if (n == 0) return NERF_OK;
  NERF_CHECK_ARG(rays && t && face && bary && (n_keys == 0 || (sorted_keys && vertices && faces && F > 0)));
  if (!aligned8(t) || (n_keys && !aligned8(sorted_keys))) return NERF_E_ALIGN;
  ray_cast_kernel<<<(unsigned)nerf_cdiv(n, NTHREADS), NTHREADS, 0, stream>>>(rays, n, sorted_keys, n_keys, vertices,
                                                                            faces, F, g, margin, cull != 0, t, face, bary);
  return nerf_launch_status();
}
