// Host check of csrc/mesh_texture_core.hpp (texture baking): make_atlas, texel and lookup run
// serially, one call per texel and per lookup exactly as the kernels run them (one call per thread).  Every array has
// exactly its size, so a slot read or written out of range is caught by the sanitizer.  Checked: the layout against a
// plain search for cols, and its limits; every texel written once, the owners a partition of every full cell, the
// weights in [0, 1] with sum 1 to rounding, a texel inside its UV triangle inverting the corner mix, the position
// inside the face's box, unit or zero normals, zeros at unowned texels, a NaN vertex propagating; a texture that
// holds one constant per owning face returning that constant exactly at interior and boundary points of every face
// (no bleeding), for C = 1..4; face = -1 giving zeros; faces and pairs that are out of range, huge, infinite or NaN
// reading inside the texture (the clamp) without an undefined conversion.  Stand-alone:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/mesh_texture_host_check.cpp -o mesh_texture_host_check && ./mesh_texture_host_check
//
// Exit status 0 and "ok" when every case agrees.  It needs no GPU and loads nothing of the Python package.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../nerf-sys_amd/csrc/mesh_texture_core.hpp"

namespace {

using nerf_mt::Atlas;

bool check_layout() {
  bool ok = true;
  Atlas A;
  for (int64_t F = 0; F <= 5000; ++F) {
    const int64_t cells = F > 1 ? (F + 1) / 2 : 1;
    int64_t cols = 1;
    while (cols * cols < cells) ++cols;
    if (!nerf_mt::make_atlas(F, 7, A) || A.cols != cols || A.T != 7 * cols || A.S != 7 || A.F != F) {
      std::printf("layout: F = %lld\n", (long long)F);
      ok = false;
    }
  }
  const int64_t full = 2 * (int64_t)3276 * 3276;  // 3276 * 5 = 16380 <= 16384 < 3277 * 5
  if (!nerf_mt::make_atlas(full, 5, A) || A.cols != 3276) ok = false, std::printf("layout: the largest atlas\n");
  if (nerf_mt::make_atlas(full + 1, 5, A)) ok = false, std::printf("layout: T > 16384 accepted\n");
  if (nerf_mt::make_atlas(2, 4, A) || nerf_mt::make_atlas(-1, 8, A) || nerf_mt::make_atlas(2, 16385, A))
    ok = false, std::printf("layout: a bad argument accepted\n");
  if (nerf_mt::make_atlas(std::numeric_limits<int64_t>::max(), 5, A)) ok = false, std::printf("layout: huge F accepted\n");
  return ok;
}

struct Mesh {
  std::vector<float> v, n;
  std::vector<int32_t> f;
};

Mesh random_mesh(std::mt19937& rng, int64_t V, int64_t F) {
  Mesh m;
  std::uniform_real_distribution<float> u(-1.0f, 1.0f);
  std::uniform_int_distribution<int32_t> vi(0, (int32_t)V - 1);
  m.v.resize((size_t)(3 * V));
  m.n.resize((size_t)(3 * V));
  for (auto& x : m.v) x = u(rng);
  for (auto& x : m.n) x = u(rng);
  m.f.resize((size_t)(3 * F));
  for (auto& x : m.f) x = vi(rng);
  if (F > 1) m.f[3] = m.f[4] = m.f[5];  // a face without area
  return m;
}

bool run_case(std::mt19937& rng, int64_t F, int S, bool nan_vertex) {
  bool ok = true;
  auto fail = [&](const char* what) {
    std::printf("F = %lld, S = %d%s: %s\n", (long long)F, S, nan_vertex ? ", NaN vertex" : "", what);
    ok = false;
  };
  Atlas A;
  if (!nerf_mt::make_atlas(F, S, A)) return fail("make_atlas"), false;
  const int64_t V = 12, P = (int64_t)A.T * A.T;
  Mesh m = random_mesh(rng, V, F);
  if (nan_vertex && F) m.v[3 * m.f[0] + 1] = NAN;
  const float unset = -12345.0f;

  for (int with_vn = 0; with_vn < 2; ++with_vn) {
    std::vector<int32_t> face((size_t)P, -7);
    std::vector<float> bary((size_t)(2 * P), unset), pos((size_t)(3 * P), unset), nrm((size_t)(3 * P), unset);
    for (int64_t p = 0; p < P; ++p)
      nerf_mt::texel(A, F ? m.v.data() : nullptr, F ? m.f.data() : nullptr, with_vn && F ? m.n.data() : nullptr, p,
                     face.data(), bary.data(), pos.data(), nrm.data());
    std::vector<int64_t> owned((size_t)(F + 1), 0);
    for (int64_t p = 0; p < P; ++p) {
      const int32_t f = face[p];
      const int i = (int)(p % A.T) % S, j = (int)(p / A.T) % S;
      const int64_t cell = (p / A.T / S) * A.cols + (p % A.T) / S;
      const int64_t want = 2 * cell + (i + j >= S);
      if (f != (want < F ? want : -1)) fail("owner");
      for (int k = 0; k < 3; ++k)
        if (pos[3 * p + k] == unset || nrm[3 * p + k] == unset || bary[2 * p + (k & 1)] == unset) fail("unwritten slot");
      if (f < 0) {
        for (int k = 0; k < 3; ++k)
          if (pos[3 * p + k] != 0.0f || nrm[3 * p + k] != 0.0f || bary[2 * p + (k & 1)] != 0.0f) fail("unowned texel not zero");
        continue;
      }
      ++owned[f];
      const float b1 = bary[2 * p], b2 = bary[2 * p + 1], b0 = 1.0f - b1 - b2;
      if (!(b1 >= 0.0f && b2 >= 0.0f && b1 <= 1.0f && b2 <= 1.0f && b0 >= -2e-7f)) fail("weights outside [0, 1]");
      // inside the UV triangle the pair inverts the corner mix
      const float xc = (float)i + 0.5f, yc = (float)j + 0.5f;
      const float x = (f & 1) ? (float)S - xc : xc, y = (f & 1) ? (float)S - yc : yc;
      if (x >= 1.0f && y >= 1.0f && x + y <= (float)(S - 2)) {
        float px[3], py[3];
        for (int k = 0; k < 3; ++k) nerf_mt::corner_uv(S, f & 1, k, px[k], py[k]);
        const float mx = b0 * px[0] + b1 * px[1] + b2 * px[2], my = b0 * py[0] + b1 * py[1] + b2 * py[2];
        if (std::fabs(mx - xc) > 1e-5f * S || std::fabs(my - yc) > 1e-5f * S) fail("the pair does not invert the mix");
      }
      const bool poisoned = nan_vertex && (m.f[3 * f] == m.f[0] || m.f[3 * f + 1] == m.f[0] || m.f[3 * f + 2] == m.f[0]);
      if (poisoned) {
        if (!std::isnan(pos[3 * p + 1])) fail("a NaN vertex must propagate to the position");
        continue;
      }
      double len = 0.0;
      for (int k = 0; k < 3; ++k) {
        float lo = INFINITY, hi = -INFINITY;
        for (int c = 0; c < 3; ++c) {
          lo = std::fmin(lo, m.v[3 * m.f[3 * f + c] + k]);
          hi = std::fmax(hi, m.v[3 * m.f[3 * f + c] + k]);
        }
        if (!(pos[3 * p + k] >= lo - 1e-6f && pos[3 * p + k] <= hi + 1e-6f)) fail("the point left its face's box");
        len += (double)nrm[3 * p + k] * nrm[3 * p + k];
      }
      if (!(len == 0.0 || std::fabs(len - 1.0) < 1e-6)) fail("a normal is neither a unit vector nor zero");
      if (!with_vn && f == 1 && len != 0.0) fail("a face without area must have a zero normal");
    }
    // the owned texels of a face: its half cell, S (S + 1) / 2 for an even face and S (S - 1) / 2 for an odd one
    for (int64_t f = 0; f < F; ++f)
      if (owned[f] != ((f & 1) ? (int64_t)S * (S - 1) / 2 : (int64_t)S * (S + 1) / 2)) fail("a face's texel count");

    if (with_vn) continue;
    // no bleeding: one constant per owning face, a sentinel on unowned texels
    for (int C = 1; C <= 4; ++C) {
      std::vector<float> tex((size_t)(P * C));
      for (int64_t p = 0; p < P; ++p)
        for (int c = 0; c < C; ++c) tex[(size_t)(p * C + c)] = face[p] < 0 ? -1000.0f : (float)(face[p] * 4 + c) + 0.25f;
      const int64_t per_face = 256, N = F * per_face + 8;
      std::vector<int32_t> qf((size_t)N);
      std::vector<float> qb((size_t)(2 * N)), out((size_t)(N * C), unset);
      std::uniform_real_distribution<float> u01(0.0f, 1.0f);
      const float special[6][2] = {{0, 0}, {1, 0}, {0, 1}, {0.5f, 0}, {0, 0.5f}, {0.5f, 0.5f}};
      for (int64_t f = 0; f < F; ++f)
        for (int64_t k = 0; k < per_face; ++k) {
          float a = u01(rng), b = u01(rng);
          if (a + b > 1.0f) a = 1.0f - a, b = 1.0f - b;
          if (k < 6) a = special[k][0], b = special[k][1];
          else if (k < 64) b = 1.0f - a;  // on the hypotenuse, u + v = 1 exactly
          else if (k < 96) b = 0.0f;
          else if (k < 128) a = 0.0f;
          qf[(size_t)(f * per_face + k)] = (int32_t)f;
          qb[(size_t)(2 * (f * per_face + k))] = a, qb[(size_t)(2 * (f * per_face + k) + 1)] = b;
        }
      // the tail: no face, faces past the end, pairs far outside, infinite and NaN
      const int32_t tail_f[8] = {-1, -5, (int32_t)F, (int32_t)F + 1001, 2147483647, 0, 0, 0};
      const float tail_b[8][2] = {{0.3f, 0.3f}, {NAN, 0}, {0.2f, 0.2f}, {0.9f, 0.05f}, {0.5f, 0.5f}, {1e30f, -1e30f},
                                  {INFINITY, 0.0f}, {NAN, NAN}};
      for (int k = 0; k < 8; ++k) {
        qf[(size_t)(F * per_face + k)] = tail_f[k];
        qb[(size_t)(2 * (F * per_face + k))] = tail_b[k][0], qb[(size_t)(2 * (F * per_face + k) + 1)] = tail_b[k][1];
      }
      for (int64_t n = 0; n < N; ++n) nerf_mt::lookup(A, tex.data(), C, qf.data(), qb.data(), n, out.data());
      for (int64_t n = 0; n < F * per_face; ++n)
        for (int c = 0; c < C; ++c)
          if (out[(size_t)(n * C + c)] != (float)(qf[n] * 4 + c) + 0.25f) fail("a lookup blended another face's texel");
      for (int c = 0; c < C; ++c) {
        if (out[(size_t)((F * per_face) * C + c)] != 0.0f || out[(size_t)((F * per_face + 1) * C + c)] != 0.0f)
          fail("face < 0 must give zeros");
        for (int k = 2; k < 8; ++k)
          if (out[(size_t)((F * per_face + k) * C + c)] == unset) fail("unwritten lookup");
      }
    }
  }
  return ok;
}

}  // namespace

int main() {
  std::mt19937 rng(11);
  bool ok = check_layout();
  const int cases[][2] = {{0, 5}, {1, 5}, {2, 6}, {3, 7}, {8, 7}, {9, 7}, {33, 16}, {128, 9}, {3, 5}, {128, 8}, {50, 19}};
  for (const auto& c : cases) {
    ok &= run_case(rng, c[0], c[1], false);
    ok &= run_case(rng, c[0], c[1], true);
  }
  std::printf(ok ? "ok\n" : "FAILED\n");
  return ok ? 0 : 1;
}
