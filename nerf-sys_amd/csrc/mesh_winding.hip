// The generalised winding number on the device (the shared core is mesh_winding_core.hpp).
//
//   nerf_mesh_winding_keys     one thread per face: the key (brick << 32) | face of the cell of its fp32 centroid.
//   nerf_mesh_winding_soup     one thread per sorted position: the corners of its face, 9 floats, so that the two
//                              kernels below stream the faces of a brick contiguously.
//   nerf_mesh_winding_moments  one thread per occupied brick, the single owner of its sums: the run [start, end), the
//                              area-weighted centroid p, the dipole n and the squared radius r2, in sorted order.
//   nerf_mesh_winding          one thread per query, one double accumulator: the bricks in ascending order, a far
//                              brick by its dipole, a near brick by the exact solid angles of its run.
//
// The brick loop of the query kernel is the same for every lane, so a brick's record and a face's corners sit at
// wave-uniform addresses: the lanes of a wave read the same words, no LDS tile.  Only the near / far choice differs
// between lanes.  No LDS, no atomics: every output element has one writer and is a function of the input alone.  The
// kernels do not check indices or finiteness: that is the caller's duty (kernels.py validates before launching).
#include "common.hpp"
#include "mesh_grid_host.hpp"
#include "mesh_winding_core.hpp"

namespace {

constexpr int NTHREADS = 256;
constexpr int NOWNERS = 64;  // a moments thread walks a whole run: one wave per block spreads the runs over the CUs
using nerf_grid::aligned8;
using nerf_grid::LIMIT;
using nerf_grid::make_grid;

__global__ __launch_bounds__(NTHREADS) void winding_keys_kernel(const float* __restrict__ verts,
                                                                const int32_t* __restrict__ faces, int64_t F,
                                                                nerf_grid::Grid g, int64_t* __restrict__ keys) {
  const int64_t f = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (f >= F) return;
  keys[f] = nerf_mw::face_brick_key(g, verts, faces, f);
}

__global__ __launch_bounds__(NTHREADS) void winding_soup_kernel(const float* __restrict__ verts,
                                                                const int32_t* __restrict__ faces, int64_t F,
                                                                const int64_t* __restrict__ sorted_keys,
                                                                float* __restrict__ soup) {
  const int64_t j = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (j >= F) return;
  nerf_mw::write_soup(verts, faces, sorted_keys, j, soup);
}

__global__ __launch_bounds__(NOWNERS) void winding_moments_kernel(const float* __restrict__ soup, int64_t F,
                                                                  const int64_t* __restrict__ starts, int64_t B,
                                                                  int32_t* __restrict__ runs,
                                                                  double* __restrict__ moments) {
  const int64_t b = (int64_t)blockIdx.x * NOWNERS + threadIdx.x;
  if (b >= B) return;
  nerf_mw::brick_moments(soup, F, starts, B, b, runs + nerf_mw::RUN * b, moments + nerf_mw::MOMENTS * b);
}

__global__ __launch_bounds__(NTHREADS) void winding_kernel(const float* __restrict__ query, int64_t n,
                                                           const int32_t* __restrict__ runs,
                                                           const double* __restrict__ moments, int64_t B,
                                                           const float* __restrict__ soup, double beta2, bool exact,
                                                           double* __restrict__ w) {
  const int64_t i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (i >= n) return;
  const float q[3] = {query[3 * i], query[3 * i + 1], query[3 * i + 2]};
  w[i] = nerf_mw::winding(q, runs, moments, B, soup, beta2, exact);
}

}  // namespace

extern "C" int nerf_mesh_winding_keys(const float* vertices, const int32_t* faces, int64_t F, const float* lo,
                                      float inv, const int32_t* dims, int64_t* keys, hipStream_t stream) {
  nerf_grid::Grid g;
  NERF_CHECK_ARG(F >= 0 && 3 * F < LIMIT && make_grid(lo, 1.0f, inv, dims, g));  // the keys do not use the cell itself
  if (F == 0) return NERF_OK;
  NERF_CHECK_ARG(vertices && faces && keys);
  if (!aligned8(keys)) return NERF_E_ALIGN;
  winding_keys_kernel<<<(unsigned)nerf_cdiv(F, NTHREADS), NTHREADS, 0, stream>>>(vertices, faces, F, g, keys);
  return nerf_launch_status();
}

extern "C" int nerf_mesh_winding_soup(const float* vertices, const int32_t* faces, int64_t F,
                                      const int64_t* sorted_keys, float* soup, hipStream_t stream) {
  NERF_CHECK_ARG(F >= 0 && 3 * F < LIMIT);
  if (F == 0) return NERF_OK;
  NERF_CHECK_ARG(vertices && faces && sorted_keys && soup);
  if (!aligned8(sorted_keys)) return NERF_E_ALIGN;
  winding_soup_kernel<<<(unsigned)nerf_cdiv(F, NTHREADS), NTHREADS, 0, stream>>>(vertices, faces, F, sorted_keys, soup);
  return nerf_launch_status();
}

extern "C" int nerf_mesh_winding_moments(const float* soup, int64_t F, const int64_t* starts, int64_t B, int32_t* runs,
                                         double* moments, hipStream_t stream) {
  NERF_CHECK_ARG(F >= 0 && 3 * F < LIMIT && B >= 0 && B <= F);
  if (B == 0) return NERF_OK;
  NERF_CHECK_ARG(soup && starts && runs && moments);
  if (!aligned8(starts) || !aligned8(moments)) return NERF_E_ALIGN;
  winding_moments_kernel<<<(unsigned)nerf_cdiv(B, NOWNERS), NOWNERS, 0, stream>>>(soup, F, starts, B, runs, moments);
  return nerf_launch_status();
}

extern "C" int nerf_mesh_winding(const float* query, int64_t n, const int32_t* runs, const double* moments, int64_t B,
                                 const float* soup, int64_t F, double beta, int exact, double* w, hipStream_t stream) {
  NERF_CHECK_ARG(n >= 0 && n < LIMIT && F >= 0 && 3 * F < LIMIT && B >= 0 && B <= F && (B > 0) == (F > 0) &&
                 isfinite(beta) && beta >= 1.0 && (exact == 0 || exact == 1));
  if (n == 0) return NERF_OK;
  NERF_CHECK_ARG(query && w && (B == 0 || (runs && moments && soup)));
  if (!aligned8(w) || (B && !aligned8(moments))) return NERF_E_ALIGN;
  winding_kernel<<<(unsigned)nerf_cdiv(n, NTHREADS), NTHREADS, 0, stream>>>(query, n, runs, moments, B, soup,
                                                                            beta * beta, exact != 0, w);
  return nerf_launch_status();
}
