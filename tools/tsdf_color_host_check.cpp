// Host check of the colour rules of csrc/tsdf_core.hpp: the per-voxel fusion with colour of
// nerf_tsdf_integrate_color and the per-point sampling of nerf_tsdf_sample_color run on the CPU against a plain
// restatement written here without the header's helpers, over lattices that are no multiple of anything, cameras
// outside, inside and rolled, depth images with +inf, NaN, 0 and negative entries, colour images with NaN and inf
// channels, and sample points on lattice points, edges and faces, outside the box and NaN.  The (tsdf, weight) of the
// colour rule are also held to integrate_view's bits.  Stand-alone:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/tsdf_color_host_check.cpp -o tsdf_color_host_check && ./tsdf_color_host_check
//
// Every buffer is a std::vector of exactly the size the C-ABI asks for, so an index past an image, the volume or the
// point list is an AddressSanitizer error.  Exit status 0 and "ok" when every case agrees bit for bit.  It needs no
// GPU and loads nothing of the Python package.
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

// the fusion rule with colour, one voxel and one view, written out again; c = r, g, b, cw
bool plain_view(float x0, float x1, float x2, const float* M, const std::vector<float>& depth,
                const std::vector<float>& rgb, size_t image0, int H, int W, float fx, float fy, float cx, float cy,
                float trunc, float& tsdf, float& w, float c[4], bool& coloured) {
  const float q0 = x0 - M[3], q1 = x1 - M[7], q2 = x2 - M[11];
  float cam[3];
  for (int j = 0; j < 3; ++j) {
    float acc = q0 * M[j];
    acc = acc + q1 * M[4 + j];
    acc = acc + q2 * M[8 + j];
    cam[j] = acc;
  }
  const float zc = -cam[2];
  if (std::isnan(zc) || zc <= 0.0f) return false;
  const float u = fx * (cam[0] / zc) + cx, v = fy * ((-cam[1]) / zc) + cy;
  if (std::isnan(u) || std::isnan(v) || u < 0.0f || v < 0.0f || u >= (float)W || v >= (float)H) return false;
  const size_t pixel = image0 + (size_t)std::floor(v) * W + (size_t)std::floor(u);
  const float d = depth.at(pixel);
  if (!std::isfinite(d) || d <= 0.0f) return false;
  float sum = q0 * q0;
  sum = sum + q1 * q1;
  sum = sum + q2 * q2;
  const float r = (float)std::sqrt((double)sum);  // the correctly rounded fp32 root
  const float s = d - r;
  if (s < -trunc) return false;
  const float tq = s / trunc;
  tsdf = (tsdf * w + std::fmin(1.0f, tq)) / (w + 1.0f);
  w = w + 1.0f;
  if (tq >= 1.0f) return true;  // clamped: outside the band
  float px[3];
  for (int j = 0; j < 3; ++j) px[j] = rgb.at(3 * pixel + j);
  if (!std::isfinite(px[0]) || !std::isfinite(px[1]) || !std::isfinite(px[2])) return true;
  const float cw = c[3];
  for (int j = 0; j < 3; ++j) {
    float num = c[j] * cw;
    num = num + px[j];
    c[j] = num / (cw + 1.0f);
  }
  c[3] = cw + 1.0f;
  coloured = true;
  return true;
}

bool integrate_case(const char* name, int nx, int ny, int nz, int H, int W, int n_views, uint32_t seed) {
  std::mt19937 rng(seed);
  std::uniform_real_distribution<float> uni(0.f, 1.f);
  const float lo[3] = {-0.5f, -0.75f, -1.5f}, hi[3] = {0.5f, 0.75f, 1.5f};
  const Volume L = volume(nx, ny, nz, lo, hi);
  const Camera C{H, W, 0.6f * W, 0.5f * H, 0.45f * W, 0.55f * H, 0.3f};  // wide: a 1x1 image still holds the box
  const size_t image = (size_t)H * W;
  std::vector<float> c2w(12 * (size_t)n_views), depth((size_t)n_views * image), rgb(3 * (size_t)n_views * image);
  for (int v = 0; v < n_views; ++v) {
    const double far = v % 3 == 1 ? 0.3 : 3.5;  // every third camera sits inside the box
    const double c[3] = {far * (uni(rng) - 0.5), far * (uni(rng) - 0.5), far * (0.4 + uni(rng))};
    look_at(c, 2.0 * uni(rng), &c2w[12 * (size_t)v]);
  }
  const float special[5] = {INFINITY, NAN, 0.0f, -1.5f, -INFINITY};
  for (size_t i = 0; i < depth.size(); ++i) {
    // ranges around the box, so that voxels fall inside the band, in front of it and behind it
    depth[i] = 0.2f + 4.0f * uni(rng);
    if (uni(rng) < 0.2f) depth[i] = special[rng() % 5];
  }
  const float bad_channel[3] = {NAN, INFINITY, -INFINITY};
  for (size_t i = 0; i < rgb.size(); ++i) {
    rgb[i] = uni(rng);
    if (uni(rng) < 0.05f) rgb[i] = bad_channel[rng() % 3];
  }
  const size_t P = (size_t)nx * ny * nz;
  std::vector<float> tsdf(P, 1.0f), weight(P, 0.0f), color(4 * P, 0.0f);
  std::vector<float> tsdf_ref(P, 1.0f), weight_ref(P, 0.0f), color_ref(4 * P, 0.0f);
  std::vector<float> tsdf_plain(P, 1.0f), weight_plain(P, 0.0f);
  size_t updates = 0, paints = 0, painted = 0, partly = 0, bad = 0;
  for (int ix = 0; ix < nx; ++ix)
    for (int iy = 0; iy < ny; ++iy)
      for (int iz = 0; iz < nz; ++iz) {
        const size_t p = ((size_t)ix * ny + iy) * nz + iz;
        float x[3];
        nerf_tsdf::lattice_point(L, ix, iy, iz, x);
        for (int v = 0; v < n_views; ++v) {
          bool ca = false, cb = false;
          const float* M = &c2w[12 * (size_t)v];
          const bool a = nerf_tsdf::integrate_view_color(x, M, depth.data() + (size_t)v * image,
                                                         rgb.data() + 3 * (size_t)v * image, C, tsdf[p], weight[p],
                                                         &color[4 * p], ca);
          const bool b = plain_view(lo[0] + (float)ix * L.h[0], lo[1] + (float)iy * L.h[1], lo[2] + (float)iz * L.h[2],
                                    M, depth, rgb, (size_t)v * image, H, W, C.fx, C.fy, C.cx, C.cy, C.trunc,
                                    tsdf_ref[p], weight_ref[p], &color_ref[4 * p], cb);
          const bool c = nerf_tsdf::integrate_view(x, M, depth.data() + (size_t)v * image, C, tsdf_plain[p],
                                                   weight_plain[p]);
          bad += a != b || a != c || ca != cb || (ca && !a);
          updates += a;
          paints += ca;
        }
        painted += color[4 * p + 3] > 0.0f;
        partly += color[4 * p + 3] > 0.0f && color[4 * p + 3] < weight[p];
        bad += bits(tsdf[p]) != bits(tsdf_ref[p]) || bits(weight[p]) != bits(weight_ref[p]);
        bad += bits(tsdf[p]) != bits(tsdf_plain[p]) || bits(weight[p]) != bits(weight_plain[p]);
        for (int j = 0; j < 4; ++j) bad += bits(color[4 * p + j]) != bits(color_ref[4 * p + j]);
      }
  // views update and views skip, views colour and coloured voxels were also updated without colour
  const bool ok = bad == 0 && paints > 0 && paints < updates && updates < P * (size_t)n_views && painted > 0;
  std::printf("%-22s %dx%dx%d, %d views of %dx%d: %zu updates, %zu with colour, %zu of %zu voxels coloured "
              "(%zu of them cw < w), %zu mismatches %s\n", name, nx, ny, nz, n_views, H, W, updates, paints, painted, P,
              partly, bad, ok ? "ok" : "MISMATCH");
  return ok;
}

// the sampling rule at one point, written out again
void plain_sample(const std::vector<float>& color, int nx, int ny, int nz, const float lo[3], const float hi[3],
                  const float x[3], float rgb[3], float& cover) {
  rgb[0] = rgb[1] = rgb[2] = 0.0f;
  cover = 0.0f;
  if (std::isnan(x[0]) || std::isnan(x[1]) || std::isnan(x[2])) return;
  const int n[3] = {nx, ny, nz};
  long i[3];
  float f[3];
  for (int a = 0; a < 3; ++a) {
    const float h = (hi[a] - lo[a]) / (float)(n[a] - 1);
    float g = (x[a] - lo[a]) / h;
    g = std::fmin(std::fmax(g, 0.0f), (float)(n[a] - 1));
    i[a] = std::min((long)std::floor(g), (long)n[a] - 2);
    f[a] = g - (float)i[a];
  }
  float acc[3] = {0.0f, 0.0f, 0.0f};
  for (int dz = 0; dz < 2; ++dz)
    for (int dy = 0; dy < 2; ++dy)
      for (int dx = 0; dx < 2; ++dx) {  // x fastest: corner c = dx + 2 dy + 4 dz
        const size_t p = ((size_t)(i[0] + dx) * ny + (i[1] + dy)) * nz + (i[2] + dz);
        float tw = (dx ? f[0] : 1.0f - f[0]) * (dy ? f[1] : 1.0f - f[1]);
        tw = tw * (dz ? f[2] : 1.0f - f[2]);
        const float k = tw * color.at(4 * p + 3);
        cover = cover + k;
        for (int j = 0; j < 3; ++j) {
          const float term = k * color.at(4 * p + j);
          acc[j] = acc[j] + term;
        }
      }
  if (cover > 0.0f)
    for (int j = 0; j < 3; ++j) rgb[j] = acc[j] / cover;
}

bool sample_case(const char* name, int nx, int ny, int nz, int n_random, uint32_t seed) {
  std::mt19937 rng(seed);
  std::uniform_real_distribution<float> uni(0.f, 1.f);
  const float lo[3] = {-0.5f, -0.75f, -1.5f}, hi[3] = {0.5f, 0.75f, 1.5f};
  const Volume L = volume(nx, ny, nz, lo, hi);
  const size_t P = (size_t)nx * ny * nz;
  std::vector<float> color(4 * P);
  for (size_t p = 0; p < P; ++p) {
    const float cw = (float)(rng() % 4);
    for (int j = 0; j < 3; ++j) color[4 * p + j] = cw > 0.0f ? uni(rng) : 0.0f;
    color[4 * p + 3] = cw;
  }
  std::vector<float> points;
  auto add = [&](float a, float b, float c) { points.insert(points.end(), {a, b, c}); };
  for (int ix = 0; ix < nx; ++ix)  // lattice points, edge midpoints and face-diagonal midpoints
    for (int iy = 0; iy < ny; ++iy)
      for (int iz = 0; iz < nz; iz += 3) {
        float x[3];
        nerf_tsdf::lattice_point(L, ix, iy, iz, x);
        add(x[0], x[1], x[2]);
        add(x[0] + 0.5f * L.h[0], x[1], x[2]);
        add(x[0], x[1] + 0.25f * L.h[1], x[2] + 0.25f * L.h[2]);
      }
  for (int k = 0; k < n_random; ++k)
    add(lo[0] + (hi[0] - lo[0]) * (1.4f * uni(rng) - 0.2f), lo[1] + (hi[1] - lo[1]) * (1.4f * uni(rng) - 0.2f),
        lo[2] + (hi[2] - lo[2]) * (1.4f * uni(rng) - 0.2f));  // a fifth of the range outside on each side
  add(hi[0], hi[1], hi[2]);
  add(lo[0], lo[1], lo[2]);
  add(INFINITY, 0.0f, -INFINITY);
  add(NAN, 0.0f, 0.0f);
  add(0.0f, 0.0f, NAN);
  const size_t N = points.size() / 3;
  std::vector<float> rgb(3 * N, 7.0f), cover(N, 7.0f);
  size_t bad = 0, unseen = 0;
  for (size_t i = 0; i < N; ++i) {
    nerf_tsdf::sample_color(color.data(), L, &points[3 * i], &rgb[3 * i], cover[i]);
    float want[3], want_cover;
    plain_sample(color, nx, ny, nz, lo, hi, &points[3 * i], want, want_cover);
    bad += bits(cover[i]) != bits(want_cover);
    for (int j = 0; j < 3; ++j) bad += bits(rgb[3 * i + j]) != bits(want[j]);
    unseen += cover[i] == 0.0f;
  }
  const bool ok = bad == 0 && unseen >= 2 && unseen < N;
  std::printf("%-22s %dx%dx%d, %zu points: %zu with cover 0, %zu mismatches %s\n", name, nx, ny, nz, N, unseen, bad,
              ok ? "ok" : "MISMATCH");
  return ok;
}

}  // namespace

int main() {
  bool ok = true;
  ok = integrate_case("main lattice", 5, 6, 67, 5, 7, 3, 1) && ok;
  ok = integrate_case("minimum lattice", 2, 2, 2, 1, 1, 6, 2) && ok;
  ok = integrate_case("33 views", 5, 6, 67, 3, 3, 33, 3) && ok;
  ok = integrate_case("cube, larger image", 17, 17, 17, 48, 48, 14, 4) && ok;
  ok = sample_case("samples", 5, 6, 67, 2000, 5) && ok;
  ok = sample_case("samples, minimum", 2, 2, 2, 200, 6) && ok;
  std::printf(ok ? "ok\n" : "FAILED\n");
  return ok ? 0 : 1;
}
