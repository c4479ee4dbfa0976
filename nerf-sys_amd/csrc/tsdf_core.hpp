// TSDF fusion of depth views into a lattice (colour §3.11.9): the per-voxel work of
// nerf_tsdf_integrate and nerf_tsdf_integrate_color and the per-point work of nerf_tsdf_face_observed and
// nerf_tsdf_sample_color (tsdf.hip), written once for the device and for a host compiler so that
// the rule can be run and checked under a host sanitizer without a GPU.  tests/tsdf_reference.py and
// tests/tsdf_color_reference.py restate it in numpy.
//
// The volume is mesh_extract's lattice: (nx,ny,nz), linear index p = (ix ny + iy) nz + iz, the point at
// lo + (ix,iy,iz) h.  A view is a row-major 3x4 camera-to-world matrix M (camera looking along -z, y up, pixel
// centres: the inverse of make_ray in rays.hip) and an (H,W) image of ranges along unit ray directions.  Everything
// is fp32 and every operation is rounded once: the including .hip file is compiled with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NERF_TSDF_HD __host__ __device__ __forceinline__
#else
#define NERF_TSDF_HD inline
#endif

namespace nerf_tsdf {

struct Volume {
  int nx, ny, nz;
  float lo[3], h[3];  // integrate and sample_color only
};

struct Camera {
  int H, W;
  float fx, fy, cx, cy, trunc;
};

NERF_TSDF_HD void lattice_point(const Volume& L, int ix, int iy, int iz, float x[3]) {
  const int i[3] = {ix, iy, iz};
#pragma unroll
  for (int a = 0; a < 3; ++a) x[a] = L.lo[a] + (float)i[a] * L.h[a];
}

// One view applied to the voxel at x: true iff the view updated (tsdf, w).  M: the view's 12 floats, depth: the
// view's own (H,W) image.  Every comparison is written so that a NaN skips.
NERF_TSDF_HD bool integrate_view(const float x[3], const float* __restrict__ M, const float* __restrict__ depth,
                                 const Camera& C, float& tsdf, float& w) {
  const float q0 = x[0] - M[3], q1 = x[1] - M[7], q2 = x[2] - M[11];
  const float c0 = q0 * M[0] + q1 * M[4] + q2 * M[8];
  const float c1 = q0 * M[1] + q1 * M[5] + q2 * M[9];
  const float c2 = q0 * M[2] + q1 * M[6] + q2 * M[10];
  const float zc = -c2;
  if (!(zc > 0.0f)) return false;  // behind the camera (or NaN)
  const float u = C.fx * (c0 / zc) + C.cx;
  const float v = C.fy * ((-c1) / zc) + C.cy;
  if (!(u >= 0.0f && u < (float)C.W && v >= 0.0f && v < (float)C.H)) return false;  // in float, before any int
  const int col = (int)floorf(u), row = (int)floorf(v);
  const float d = depth[(int64_t)row * C.W + col];
  if (!(d > 0.0f && d < INFINITY)) return false;  // +inf: a miss; NaN, 0, negative: no surface seen
  const float r = sqrtf(q0 * q0 + q1 * q1 + q2 * q2);
  const float s = d - r;
  if (s < -C.trunc) return false;  // hidden behind the surface
  const float tq = s / C.trunc;
  const float t = tq < 1.0f ? tq : 1.0f;
  tsdf = (tsdf * w + t) / (w + 1.0f);
  w = w + 1.0f;
  return true;
}

// integrate_view with colour.  The geometry and the update of (tsdf, w) are integrate_view's, line
// for line: they are written out again, not shared, so that the plain kernel's code stays what it was (sharing them
// through a helper changed its control flow and register use); the tests and tools/tsdf_color_host_check.cpp hold the
// two to the same bits.  rgb: the view's own (H,W,3) image; c: the voxel's r, g, b and colour weight cw.  Where the
// view updated the voxel, the update was not clamped (tq < 1: the voxel lies within trunc of the surface the pixel
// saw) and the pixel's three channels are finite, every channel becomes (c cw + pixel) / (cw + 1), then cw = cw + 1,
// and coloured is set.
NERF_TSDF_HD bool integrate_view_color(const float x[3], const float* __restrict__ M, const float* __restrict__ depth,
                                       const float* __restrict__ rgb, const Camera& C, float& tsdf, float& w,
                                       float c[4], bool& coloured) {
  const float q0 = x[0] - M[3], q1 = x[1] - M[7], q2 = x[2] - M[11];
  const float c0 = q0 * M[0] + q1 * M[4] + q2 * M[8];
  const float c1 = q0 * M[1] + q1 * M[5] + q2 * M[9];
  const float c2 = q0 * M[2] + q1 * M[6] + q2 * M[10];
  const float zc = -c2;
  if (!(zc > 0.0f)) return false;
  const float u = C.fx * (c0 / zc) + C.cx;
  const float v = C.fy * ((-c1) / zc) + C.cy;
  if (!(u >= 0.0f && u < (float)C.W && v >= 0.0f && v < (float)C.H)) return false;
  const int col = (int)floorf(u), row = (int)floorf(v);
  const int64_t pixel = (int64_t)row * C.W + col;
  const float d = depth[pixel];
  if (!(d > 0.0f && d < INFINITY)) return false;
  const float r = sqrtf(q0 * q0 + q1 * q1 + q2 * q2);
  const float s = d - r;
  if (s < -C.trunc) return false;
  const float tq = s / C.trunc;
  const float t = tq < 1.0f ? tq : 1.0f;
  tsdf = (tsdf * w + t) / (w + 1.0f);
  w = w + 1.0f;
  if (tq < 1.0f) {
    const float* px = rgb + 3 * pixel;
    const float p0 = px[0], p1 = px[1], p2 = px[2];
    if (fabsf(p0) < INFINITY && fabsf(p1) < INFINITY && fabsf(p2) < INFINITY) {  // a NaN fails the comparison
      const float cw = c[3], cw1 = cw + 1.0f;
      c[0] = (c[0] * cw + p0) / cw1;
      c[1] = (c[1] * cw + p1) / cw1;
      c[2] = (c[2] * cw + p2) / cw1;
      c[3] = cw1;
      coloured = true;
    }
  }
  return true;
}

// The fused colour at the point x: the trilinear mean of the 8 corners of the cell that holds x,
// every corner weighted by its trilinear weight times its colour weight.  color: (nx,ny,nz,4) r, g, b, cw.  Per axis
// g = (x - lo) / h clamped to [0, n - 1], i = min((int)floor(g), n - 2), f = g - (float)i; the corners in
// cell_observed's order (bit 0 = x, bit 1 = y, bit 2 = z), a set bit weighted f, a clear one 1 - f:
// k = ((wx wy) wz) cw, cover += k, acc_j += k c_j.  rgb_j = acc_j / cover where cover > 0, else 0; a NaN coordinate
// gives cover = 0.
NERF_TSDF_HD void sample_color(const float* __restrict__ color, const Volume& L, const float x[3], float rgb[3],
                               float& cover) {
  rgb[0] = rgb[1] = rgb[2] = 0.0f;
  cover = 0.0f;
  if (x[0] != x[0] || x[1] != x[1] || x[2] != x[2]) return;
  const int n[3] = {L.nx, L.ny, L.nz};
  int i[3];
  float f[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float g = (x[a] - L.lo[a]) / L.h[a];
    const float top = (float)(n[a] - 1);
    g = g > 0.0f ? (g < top ? g : top) : 0.0f;  // written so that a NaN (inf over an infinite h) lands on 0 too
    const int fl = (int)floorf(g);
    i[a] = fl < n[a] - 2 ? fl : n[a] - 2;
    f[a] = g - (float)i[a];
  }
  const int64_t sx = (int64_t)L.ny * L.nz, sy = L.nz;
  const int64_t p = (int64_t)i[0] * sx + (int64_t)i[1] * sy + i[2];
  float acc[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float* v = color + 4 * (p + ((c & 1) ? sx : 0) + ((c & 2) ? sy : 0) + ((c & 4) ? 1 : 0));
    const float wx = (c & 1) ? f[0] : 1.0f - f[0];
    const float wy = (c & 2) ? f[1] : 1.0f - f[1];
    const float wz = (c & 4) ? f[2] : 1.0f - f[2];
    const float k = ((wx * wy) * wz) * v[3];
    cover = cover + k;
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[j] = acc[j] + k * v[j];
  }
  if (cover > 0.0f) {
#pragma unroll
    for (int j = 0; j < 3; ++j) rgb[j] = acc[j] / cover;
  }
}

// every one of the 8 corners of the cell with low corner p has weight >= min_weight; false where p owns no cell
NERF_TSDF_HD bool cell_observed(const float* __restrict__ weight, const Volume& L, int ix, int iy, int iz, int64_t p,
                                float min_weight) {
  if (!(ix + 1 < L.nx && iy + 1 < L.ny && iz + 1 < L.nz)) return false;
  const int64_t sx = (int64_t)L.ny * L.nz, sy = L.nz;
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 8; ++c)
    ok = ok && (weight[p + ((c & 1) ? sx : 0) + ((c & 2) ? sy : 0) + ((c & 4) ? 1 : 0)] >= min_weight);
  return ok;
}

// keep[f] = ok for the faces [face_off[p], face_off[p+1]) of the cell at p; a slot outside [0, F) (offsets that do
// not belong to this list) is not written
NERF_TSDF_HD void mark_faces(const int32_t* __restrict__ face_off, int64_t p, int64_t F, bool ok,
                             uint8_t* __restrict__ keep) {
  const int64_t b = face_off[p], e = face_off[p + 1];
  for (int64_t f = b < 0 ? 0 : b; f < e && f < F; ++f) keep[f] = ok ? 1 : 0;
}

}  // namespace nerf_tsdf
