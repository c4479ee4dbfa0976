// TSDF fusion of depth views into a truncated signed distance lattice, and the filter that keeps the triangles of
// observed cells; the same fusion with colour and the fused colour at points.
//
//   nerf_tsdf_integrate      one thread per voxel, linear in p, so a wave walks iz as the mesh kernels do.  The view
//                            loop runs inside the kernel: tsdf and weight are read once, stay in registers over all
//                            views and are written once, and only where a view updated them.  The camera rows come
//                            through a const __restrict__ pointer indexed by the (wave-uniform) view number, so they are
//                            scalar loads; the one divergent access is the depth gather, and a wave's 64 voxels along
//                            iz project onto a short image segment.  The entry point hands the kernel at most
//                            VIEWS_PER_LAUNCH views at a time (below): the waves in flight are spread over all the
//                            views of a launch, so the images of one launch should fit the caches.
//   nerf_tsdf_integrate_color  the same walk with the voxel's (r, g, b, cw) as one aligned 16-byte load and store
//                            per lane (a wave along iz touches 1 KB contiguous) and the view's pixel colour gathered
//                            next to its depth, where the update is inside the band.  Its own kernel and its own
//                            views-per-launch cap; nerf_tsdf_integrate's kernel is what it was.
//   nerf_tsdf_sample_color   one thread per point: the 8 corners' (r, g, b, cw), each weighted by its trilinear
//                            weight times its colour weight.
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
// Views per launch of the colour path, which gathers 16 bytes per pixel and view (depth and three channels) where the
// plain path gathers 4, so the cap above was not taken over but measured (profiles/tsdf_color.json): 64 views of
// 800x800 as launches of 1, 2, 4 and 8 views took 0.97 / 0.76 / 0.66 / 0.64 ms at 128^3, 8.13 / 6.32 / 5.25 / 5.55 ms at
// 256^3 and 58.5 / 44.2 / 35.0 / 31.3 ms at 512^3.  8 is the fastest on two of the three (by 12 % at 512^3) and 6 %
// behind 4 at 256^3.  More than 8 was not measured.  As above, the split changes no bit.
constexpr int COLOR_VIEWS_PER_LAUNCH = 8;

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

__global__ __launch_bounds__(NTHREADS) void tsdf_integrate_color_kernel(
    float* __restrict__ tsdf, float* __restrict__ weight, float4* __restrict__ color, Volume L, int64_t P,
    const float* __restrict__ depth, const float* __restrict__ rgb, const float* __restrict__ c2w, int n_views,
    Camera C) {
  int64_t p;
  int ix, iy, iz;
  if (!point_of_thread(L, P, p, ix, iy, iz)) return;
  float x[3];
  nerf_tsdf::lattice_point(L, ix, iy, iz, x);
  float t = tsdf[p], w = weight[p];
  const float4 c4 = color[p];
  float c[4] = {c4.x, c4.y, c4.z, c4.w};
  bool touched = false, coloured = false;
  const int64_t image = (int64_t)C.H * C.W;
  for (int v = 0; v < n_views; ++v)
    touched |= nerf_tsdf::integrate_view_color(x, c2w + 12 * (int64_t)v, depth + v * image, rgb + 3 * (v * image), C,
                                               t, w, c, coloured);
  if (touched) {
    tsdf[p] = t;
    weight[p] = w;
  }
  if (coloured) color[p] = make_float4(c[0], c[1], c[2], c[3]);
}

__global__ __launch_bounds__(NTHREADS) void tsdf_sample_color_kernel(const float* __restrict__ color, Volume L,
                                                                     const float* __restrict__ points, int64_t N,
                                                                     float* __restrict__ rgb_out,
                                                                     float* __restrict__ cover_out) {
  const int64_t i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (i >= N) return;
  const float x[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
  float rgb[3], cover;
  nerf_tsdf::sample_color(color, L, x, rgb, cover);
  rgb_out[3 * i] = rgb[0];
  rgb_out[3 * i + 1] = rgb[1];
  rgb_out[3 * i + 2] = rgb[2];
  cover_out[i] = cover;
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

Volume lattice_of(int nx, int ny, int nz, const float* lo, const float* hi) {
  Volume L{nx, ny, nz, {lo[0], lo[1], lo[2]}, {0.f, 0.f, 0.f}};
  const int n[3] = {nx, ny, nz};
  for (int a = 0; a < 3; ++a) L.h[a] = (hi[a] - lo[a]) / (float)(n[a] - 1);
  return L;
}

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

extern "C" int nerf_tsdf_integrate_color(float* tsdf, float* weight, float* color, int nx, int ny, int nz,
                                         const float* lo, const float* hi, const float* depth, const float* rgb,
                                         const float* c2w, int n_views, int H, int W, float fx, float fy, float cx,
                                         float cy, float trunc, hipStream_t stream) {
  int64_t P = 0;
  NERF_CHECK_ARG(lattice_ok(nx, ny, nz, P));
  NERF_CHECK_ARG(lo && hi && n_views >= 0);
  NERF_CHECK_ARG(lo[0] < hi[0] && lo[1] < hi[1] && lo[2] < hi[2]);
  NERF_CHECK_ARG(positive_finite(trunc) && positive_finite(fx) && positive_finite(fy) && isfinite(cx) && isfinite(cy));
  if (n_views == 0) return NERF_OK;  // nothing to fuse: no launch
  NERF_CHECK_ARG(H >= 1 && W >= 1 && H <= (1 << 24) && W <= (1 << 24));
  NERF_CHECK_ARG(tsdf && weight && color && depth && rgb && c2w);
  if (!nerf_aligned16(color)) return NERF_E_ALIGN;  // one 16-byte load and store per voxel
  const Volume L = lattice_of(nx, ny, nz, lo, hi);
  const Camera C{H, W, fx, fy, cx, cy, trunc};
  const int64_t image = (int64_t)H * W;
  for (int v0 = 0; v0 < n_views; v0 += COLOR_VIEWS_PER_LAUNCH) {
    const int n = n_views - v0 < COLOR_VIEWS_PER_LAUNCH ? n_views - v0 : COLOR_VIEWS_PER_LAUNCH;
    tsdf_integrate_color_kernel<<<(unsigned)nerf_cdiv(P, NTHREADS), NTHREADS, 0, stream>>>(
        tsdf, weight, reinterpret_cast<float4*>(color), L, P, depth + v0 * image, rgb + 3 * (v0 * image),
        c2w + 12 * (int64_t)v0, n, C);
    const int status = nerf_launch_status();
    if (status != NERF_OK) return status;
  }
  return NERF_OK;
}

extern "C" int nerf_tsdf_sample_color(const float* color, int nx, int ny, int nz, const float* lo, const float* hi,
                                      const float* points, int64_t N, float* rgb_out, float* cover_out,
                                      hipStream_t stream) {
  int64_t P = 0;
  NERF_CHECK_ARG(lattice_ok(nx, ny, nz, P));
  NERF_CHECK_ARG(lo && hi && N >= 0 && N < (int64_t(1) << 31) * NTHREADS);
  NERF_CHECK_ARG(lo[0] < hi[0] && lo[1] < hi[1] && lo[2] < hi[2]);
  if (N == 0) return NERF_OK;  // no points: no launch
  NERF_CHECK_ARG(color && points && rgb_out && cover_out);
  tsdf_sample_color_kernel<<<(unsigned)nerf_cdiv(N, NTHREADS), NTHREADS, 0, stream>>>(
      color, lattice_of(nx, ny, nz, lo, hi), points, N, rgb_out, cover_out);
  return nerf_launch_status();
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
