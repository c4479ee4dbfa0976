// Host check of csrc/tsdf_core.hpp: the per-voxel fusion rule and the face-range logic of
// nerf_tsdf_integrate / nerf_tsdf_face_observed run on the CPU against a plain restatement written here without the
// header's helpers, over lattices that are no multiple of anything, cameras outside, inside and rolled, depth images
// with +inf, NaN, 0 and negative entries, and face offsets with empty ranges and ranges of 12.  Stand-alone:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/tsdf_host_check.cpp -o tsdf_host_check && ./tsdf_host_check
//
// Every buffer is a std::vector of exactly the size the C-ABI asks for, so an index past an image, the volume or the
// offsets is an AddressSanitizer error.  Exit status 0 and "ok" when every case agrees bit for bit.  It needs no GPU
// and loads nothing of the Python package.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../nerf-sys_amd/csrc/tsdf_core.hpp"

namespace {

using nerf_tsdf::Camera;
using nerf_tsdf::Volume;

uint32_t bits(float v) {
  uint32_t b;
  std::memcpy(&b, &v, 4);
  return b;
}

Volume volume(int nx, int ny, int nz, const float lo[3], const float hi[3]) {
  Volume L{nx, ny, nz, {lo[0], lo[1], lo[2]}, {0.f, 0.f, 0.f}};
  const int n[3] = {nx, ny, nz};
  for (int a = 0; a < 3; ++a) L.h[a] = (hi[a] - lo[a]) / (float)(n[a] - 1);
  return L;
}

// c2w rows of a camera at c looking at the origin, rolled about its axis
void look_at(const double c[3], double roll, float M[12]) {
  double z[3], x[3], y[3], up[3] = {0.0, 0.0, 1.0};
  const double nz = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
  for (int a = 0; a < 3; ++a) z[a] = c[a] / nz;
  x[0] = up[1] * z[2] - up[2] * z[1], x[1] = up[2] * z[0] - up[0] * z[2], x[2] = up[0] * z[1] - up[1] * z[0];
  double nx = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  if (nx < 1e-8) x[0] = 1.0, x[1] = 0.0, x[2] = 0.0, nx = 1.0;
  for (int a = 0; a < 3; ++a) x[a] /= nx;
  y[0] = z[1] * x[2] - z[2] * x[1], y[1] = z[2] * x[0] - z[0] * x[2], y[2] = z[0] * x[1] - z[1] * x[0];
  const double cr = std::cos(roll), sr = std::sin(roll);
  for (int a = 0; a < 3; ++a) {
    M[4 * a + 0] = (float)(cr * x[a] + sr * y[a]);
    M[4 * a + 1] = (float)(-sr * x[a] + cr * y[a]);
    M[4 * a + 2] = (float)z[a];
    M[4 * a + 3] = (float)c[a];
  }
}

// the rule as the issue numbers it, one voxel and one view, written out again
bool plain_view(float x0, float x1, float x2, const float* M, const std::vector<float>& depth, size_t image0, int H,
                int W, float fx, float fy, float cx, float cy, float trunc, float& tsdf, float& w) {
  const float q0 = x0 - M[3], q1 = x1 - M[7], q2 = x2 - M[11];
  float c[3];
  for (int j = 0; j < 3; ++j) {
    float acc = q0 * M[j];
    acc = acc + q1 * M[4 + j];
    acc = acc + q2 * M[8 + j];
    c[j] = acc;
  }
  const float zc = -c[2];
  if (std::isnan(zc) || zc <= 0.0f) return false;
  const float u = fx * (c[0] / zc) + cx, v = fy * ((-c[1]) / zc) + cy;
  if (std::isnan(u) || std::isnan(v) || u < 0.0f || v < 0.0f || u >= (float)W || v >= (float)H) return false;
  const long col = (long)std::floor(u), row = (long)std::floor(v);
  const float d = depth.at(image0 + (size_t)row * W + col);
  if (!std::isfinite(d) || d <= 0.0f) return false;
  float sum = q0 * q0;
  sum = sum + q1 * q1;
  sum = sum + q2 * q2;
  const float r = (float)std::sqrt((double)sum);  // the correctly rounded fp32 root
  const float s = d - r;
  if (s < -trunc) return false;
  const float t = std::fmin(1.0f, s / trunc);
  tsdf = (tsdf * w + t) / (w + 1.0f);
  w = w + 1.0f;
  return true;
}

bool integrate_case(const char* name, int nx, int ny, int nz, int H, int W, int n_views, uint32_t seed) {
  std::mt19937 rng(seed);
  std::uniform_real_distribution<float> uni(0.f, 1.f);
  const float lo[3] = {-0.5f, -0.75f, -1.5f}, hi[3] = {0.5f, 0.75f, 1.5f};
  const Volume L = volume(nx, ny, nz, lo, hi);
  const Camera C{H, W, 0.6f * W, 0.5f * H, 0.45f * W, 0.55f * H, 0.3f};  // wide: a 1x1 image still holds the box
  std::vector<float> c2w(12 * (size_t)n_views), depth((size_t)n_views * H * W);
  for (int v = 0; v < n_views; ++v) {
    const double far = v % 3 == 1 ? 0.3 : 3.5;  // every third camera sits inside the box
    const double c[3] = {far * (uni(rng) - 0.5), far * (uni(rng) - 0.5), far * (0.4 + uni(rng))};
    look_at(c, 2.0 * uni(rng), &c2w[12 * (size_t)v]);
  }
  const float special[5] = {INFINITY, NAN, 0.0f, -1.5f, -INFINITY};
  for (size_t i = 0; i < depth.size(); ++i) {
    depth[i] = 0.2f + 4.0f * uni(rng);
    if (uni(rng) < 0.2f) depth[i] = special[rng() % 5];
  }
  const size_t P = (size_t)nx * ny * nz;
  std::vector<float> tsdf(P, 1.0f), weight(P, 0.0f), tsdf_ref(P, 1.0f), weight_ref(P, 0.0f);
  size_t touched = 0, updates = 0, bad = 0;
  for (int ix = 0; ix < nx; ++ix)
    for (int iy = 0; iy < ny; ++iy)
      for (int iz = 0; iz < nz; ++iz) {
        const size_t p = ((size_t)ix * ny + iy) * nz + iz;
        float x[3];
        nerf_tsdf::lattice_point(L, ix, iy, iz, x);
        bool any = false;
        for (int v = 0; v < n_views; ++v) {
          const bool a = nerf_tsdf::integrate_view(x, &c2w[12 * (size_t)v], depth.data() + (size_t)v * H * W, C,
                                                   tsdf[p], weight[p]);
          const bool b = plain_view(lo[0] + (float)ix * L.h[0], lo[1] + (float)iy * L.h[1], lo[2] + (float)iz * L.h[2],
                                    &c2w[12 * (size_t)v], depth, (size_t)v * H * W, H, W, C.fx, C.fy, C.cx, C.cy,
                                    C.trunc, tsdf_ref[p], weight_ref[p]);
          bad += a != b;
          any |= a;
          updates += a;
        }
        touched += any;
        bad += bits(tsdf[p]) != bits(tsdf_ref[p]) || bits(weight[p]) != bits(weight_ref[p]);
      }
  const bool ok = bad == 0 && touched > 0 && updates < P * (size_t)n_views;  // views update and views skip
  std::printf("%-22s %dx%dx%d, %d views of %dx%d: %zu of %zu voxels touched, %zu updates, %zu mismatches %s\n", name,
              nx, ny, nz, n_views, H, W, touched, P, updates, bad, ok ? "ok" : "MISMATCH");
  return ok;
}

bool faces_case(const char* name, int nx, int ny, int nz, uint32_t seed) {
  std::mt19937 rng(seed);
  const float zero[3] = {0.f, 0.f, 0.f}, one[3] = {1.f, 1.f, 1.f};
  const Volume L = volume(nx, ny, nz, zero, one);
  const size_t P = (size_t)nx * ny * nz;
  std::vector<int32_t> face_off(P + 1, 0);
  std::vector<float> weight(P);
  for (auto& w : weight) w = (float)(rng() % 10 ? 1 + rng() % 2 : 0);
  for (int ix = 0; ix < nx; ++ix)
    for (int iy = 0; iy < ny; ++iy)
      for (int iz = 0; iz < nz; ++iz) {
        const size_t p = ((size_t)ix * ny + iy) * nz + iz;
        const bool cell = ix + 1 < nx && iy + 1 < ny && iz + 1 < nz;
        const bool last = ix == nx - 2 && iy == ny - 2 && iz == nz - 2;
        face_off[p + 1] = face_off[p] + (cell ? (last ? 12 : (int)(rng() % 3 == 0 ? 0 : rng() % 13)) : 0);
      }
  const int64_t F = face_off[P];
  bool ok = F > 0;
  for (float min_weight : {0.0f, 1.0f, 2.0f}) {
    std::vector<uint8_t> keep((size_t)F, 7), want((size_t)F, 7);
    for (int ix = 0; ix < nx; ++ix)
      for (int iy = 0; iy < ny; ++iy)
        for (int iz = 0; iz < nz; ++iz) {
          const int64_t p = ((int64_t)ix * ny + iy) * nz + iz;
          // the kernel's order: the weights are read only where the range is not empty
          if (face_off[p + 1] > face_off[p])
            nerf_tsdf::mark_faces(face_off.data(), p, F,
                                  nerf_tsdf::cell_observed(weight.data(), L, ix, iy, iz, p, min_weight), keep.data());
          if (ix + 1 >= nx || iy + 1 >= ny || iz + 1 >= nz) continue;
          bool seen = true;
          for (int dx = 0; dx < 2; ++dx)
            for (int dy = 0; dy < 2; ++dy)
              for (int dz = 0; dz < 2; ++dz)
                seen = seen && weight.at(((size_t)(ix + dx) * ny + iy + dy) * nz + iz + dz) >= min_weight;
          for (int32_t f = face_off[p]; f < face_off[p + 1]; ++f) want.at(f) = seen;
        }
    size_t kept = 0;
    for (uint8_t k : keep) kept += k == 1;
    const bool same = keep == want;
    std::printf("%-22s %dx%dx%d min_weight %.0f: %zu of %lld faces kept %s\n", name, nx, ny, nz, min_weight, kept,
                (long long)F, same ? "ok" : "MISMATCH");
    ok = ok && same && (min_weight > 0.0f || kept == (size_t)F);
  }
  // offsets that do not belong to this list: slots outside [0, F) are not written
  {
    std::vector<int32_t> foreign = {-3, 2, 40};
    std::vector<uint8_t> keep(5, 7);
    nerf_tsdf::mark_faces(foreign.data(), 0, 5, true, keep.data());
    nerf_tsdf::mark_faces(foreign.data(), 1, 5, false, keep.data());
    ok = ok && keep == std::vector<uint8_t>({1, 1, 0, 0, 0});
  }
  return ok;
}

}  // namespace

int main() {
  bool ok = true;
  ok = integrate_case("main lattice", 5, 6, 67, 5, 7, 3, 1) && ok;
  ok = integrate_case("minimum lattice", 2, 2, 2, 1, 1, 6, 2) && ok;
  ok = integrate_case("33 views", 5, 6, 67, 3, 3, 33, 3) && ok;
  ok = integrate_case("cube, larger image", 17, 17, 17, 48, 48, 14, 4) && ok;
  ok = faces_case("face ranges", 5, 6, 67, 5) && ok;
  ok = faces_case("face ranges, minimum", 2, 2, 2, 6) && ok;
  std::printf(ok ? "ok\n" : "FAILED\n");
  return ok ? 0 : 1;
}
