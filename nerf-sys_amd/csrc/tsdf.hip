// TSDF fusion of depth views into a truncated signed distance lattice, and the filter that keeps the triangles of
// observed cells.
//
//   nerf_tsdf_integrate      one thread per voxel, linear in p, so a wave walks iz as the mesh kernels do.  The view
//                            loop runs inside the kernel: tsdf and weight are read once, stay in registers over all
//                            views and are written once, and only where a view updated them.  The camera rows come
//                            through a const __restrict__ pointer indexed by the (wave-uniform) view number, so they are
//                            scalar loads; the one divergent access is the depth gather, and a wave's 64 voxels along
//                            iz project onto a short image segment.  The entry point hands the kernel at most
//                            VIEWS_PER_LAUNCH views at a time (below): the waves in flight are spread over all the
//                            views of a launch, so the images of one launch should fit the caches.
//   nerf_tsdf_face_observed  one thread per lattice point p: keep[f] for the faces of the cell at p, which
//                            nerf_mesh_emit wrote at [face_off[p], face_off[p+1]).
//
// The per-voxel work is csrc/tsdf_core.hpp, shared with host builds.  No LDS, no atomics: every output slot has one
// writer, so equal inputs give equal bits.  This file is compiled with -ffp-contract=off (Makefile): every product,
// sum, quotient and root is rounded once, as the numpy reference rounds them.
#include "common.hpp"
#include "tsdf_core.hpp"

namespace {

using nerf_tsdf::Camera;
using nerf_tsdf::Volume;
constexpr int NTHREADS = 256;
// Views per launch.  The waves of one launch do not march through the views in step, so at any time they gather from
// all of the launch's depth images.  With 800x800 images (2.56 MB each) 8 views per launch ran at 246-354 G voxel-views
// per second on 128^3 to 512^3 volumes, all 64 views in one launch at 79-235 G, below 64 launches of one view on the
// two smaller volumes (profiles/tsdf_integrate_one_launch.json).  The launches of one call follow each other on the
// stream, and the rule applies the views one after the other, so the split changes no bit.
constexpr int VIEWS_PER_LAUNCH = 8;

__device__ __forceinline__ bool point_of_thread(const Volume& L, int64_t P, int64_t& p, int& ix, int& iy, int& iz) {
  p = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (p >= P) return false;
  const int q = (int)p;  // P < 2^31
  const int r = q / L.nz;
  iz = q - r * L.nz;
  ix = r / L.ny;
  iy = r - ix * L.ny;
  return true;
}

__global__ __launch_bounds__(NTHREADS) void tsdf_integrate_kernel(float* __restrict__ tsdf, float* __restrict__ weight,
                                                                  Volume L, int64_t P,
                                                                  const float* __restrict__ depth,
                                                                  const float* __restrict__ c2w, int n_views,
                                                                  Camera C) {
  int64_t p;
  int ix, iy, iz;
  if (!point_of_thread(L, P, p, ix, iy, iz)) return;
  float x[3];
  nerf_tsdf::lattice_point(L, ix, iy, iz, x);
  float t = tsdf[p], w = weight[p];
  bool touched = false;
  const int64_t image = (int64_t)C.H * C.W;
  for (int v = 0; v < n_views; ++v)
    touched |= nerf_tsdf::integrate_view(x, c2w + 12 * (int64_t)v, depth + v * image, C, t, w);
  if (touched) {
    tsdf[p] = t;
    weight[p] = w;
  }
}

__global__ __launch_bounds__(NTHREADS) void tsdf_face_observed_kernel(const int32_t* __restrict__ face_off,
                                                                      const float* __restrict__ weight, Volume L,
                                                                      int64_t P, float min_weight, int64_t F,
                                                                      uint8_t* __restrict__ keep) {
  int64_t p;
  int ix, iy, iz;
  if (!point_of_thread(L, P, p, ix, iy, iz)) return;
  if (face_off[p + 1] <= face_off[p]) return;  // no faces: most points; the 8 weights are not read
  nerf_tsdf::mark_faces(face_off, p, F, nerf_tsdf::cell_observed(weight, L, ix, iy, iz, p, min_weight), keep);
}

bool lattice_ok(int nx, int ny, int nz, int64_t& P) {
  if (nx < 2 || ny < 2 || nz < 2) return false;
  P = (int64_t)nx * ny * nz;
  return P < (int64_t(1) << 31);
}

bool positive_finite(float v) { return v > 0.0f && v < INFINITY; }

}  // namespace

extern "C" int nerf_tsdf_integrate(float* tsdf, float* weight, int nx, int ny, int nz, const float* lo, const float* hi,
                                   const float* depth, const float* c2w, int n_views, int H, int W, float fx, float fy,
                                   float cx, float cy, float trunc, hipStream_t stream) {
  int64_t P = 0;
  NERF_CHECK_ARG(lattice_ok(nx, ny, nz, P));
  NERF_CHECK_ARG(lo && hi && n_views >= 0);
  NERF_CHECK_ARG(lo[0] < hi[0] && lo[1] < hi[1] && lo[2] < hi[2]);
  NERF_CHECK_ARG(positive_finite(trunc) && positive_finite(fx) && positive_finite(fy) && isfinite(cx) && isfinite(cy));
  if (n_views == 0) return NERF_OK;  // nothing to fuse: no launch
  // H, W <= 2^24: (float)W is W itself, so u < (float)W keeps floor(u) below W
  NERF_CHECK_ARG(H >= 1 && W >= 1 && H <= (1 << 24) && W <= (1 << 24) && tsdf && weight && depth && c2w);
  Volume L{nx, ny, nz, {lo[0], lo[1], lo[2]}, {0.f, 0.f, 0.f}};
  const int n[3] = {nx, ny, nz};
  for (int a = 0; a < 3; ++a) L.h[a] = (hi[a] - lo[a]) / (float)(n[a] - 1);
  const Camera C{H, W, fx, fy, cx, cy, trunc};
  const int64_t image = (int64_t)H * W;
  for (int v0 = 0; v0 < n_views; v0 += VIEWS_PER_LAUNCH) {
    const int n = n_views - v0 < VIEWS_PER_LAUNCH ? n_views - v0 : VIEWS_PER_LAUNCH;
    tsdf_integrate_kernel<<<(unsigned)nerf_cdiv(P, NTHREADS), NTHREADS, 0, stream>>>(
        tsdf, weight, L, P, depth + v0 * image, c2w + 12 * (int64_t)v0, n, C);
    const int status = nerf_launch_status();
    if (status != NERF_OK) return status;
  }
  return NERF_OK;
}

extern "C" int nerf_tsdf_face_observed(const int32_t* face_off, const float* weight, int nx, int ny, int nz,
                                       float min_weight, int64_t F, uint8_t* keep, hipStream_t stream) {
  int64_t P = 0;
  NERF_CHECK_ARG(lattice_ok(nx, ny, nz, P));
  NERF_CHECK_ARG(F >= 0 && F <= 12 * P && !isnan(min_weight));
  if (F == 0) return NERF_OK;  // no faces: no launch
  NERF_CHECK_ARG(face_off && weight && keep);
  const Volume L{nx, ny, nz, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
  tsdf_face_observed_kernel<<<(unsigned)nerf_cdiv(P, NTHREADS), NTHREADS, 0, stream>>>(face_off, weight, L, P,
                                                                                       min_weight, F, keep);
  return nerf_launch_status();
}
