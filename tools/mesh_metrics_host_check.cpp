// Host check of csrc/mesh_metrics_core.hpp: the grid search run serially, one loop iteration per
// thread exactly as the kernels call it, against a brute-force search (fp32 d2 bits and indices), and the sampler
// against a plain restatement (a linear scan of the CDF, 128-bit products).  Stand-alone:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/mesh_metrics_host_check.cpp -o mesh_metrics_host_check && ./mesh_metrics_host_check
//
// Exit status 0 and "ok" when every case agrees.  It needs no GPU and loads nothing of the Python package.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../nerf-sys_amd/csrc/mesh_metrics_core.hpp"

namespace {

using nerf_mm::Grid;

bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// the grid of kernels.points_grid: lo = the minimum, dims = floor((max - lo) * inv) + 1 in fp32
bool make_grid(const std::vector<float>& p, float cell, Grid& g) {
  const int64_t m = (int64_t)p.size() / 3;
  g.cell = cell;
  g.inv = 1.0f / cell;
  for (int c = 0; c < 3; ++c) {
    float lo = 0.0f, hi = 0.0f;
    for (int64_t j = 0; j < m; ++j) {
      lo = j == 0 || p[3 * j + c] < lo ? p[3 * j + c] : lo;
      hi = j == 0 || p[3 * j + c] > hi ? p[3 * j + c] : hi;
    }
    g.lo[c] = lo;
    const float cells = floorf((hi - lo) * g.inv);
    if (!(cells + 1.0f <= (float)nerf_mm::MAX_DIM)) return false;
    g.dims[c] = (int32_t)cells + 1;
  }
  return true;
}

bool check_nearest(const char* name, const std::vector<float>& ref, const std::vector<float>& query, const Grid& g) {
  const int64_t m = (int64_t)ref.size() / 3, n = (int64_t)query.size() / 3;
  std::vector<int64_t> keys((size_t)m);
  for (int64_t j = 0; j < m; ++j) keys[j] = nerf_mm::point_key(g, ref.data(), j);
  std::sort(keys.begin(), keys.end());
  std::vector<float> sorted((size_t)(3 * m));
  for (int64_t j = 0; j < m; ++j) {
    const int64_t o = (int64_t)((uint64_t)keys[j] & 0xffffffffu);
    if (o < 0 || o >= m) return std::printf("%s: key index out of range\n", name), false;
    for (int c = 0; c < 3; ++c) sorted[3 * j + c] = ref[3 * o + c];
  }
  for (int64_t i = 0; i < n; ++i) {
    const float* q = &query[3 * i];
    const nerf_mm::Best got = nerf_mm::nearest(g, q, keys.data(), sorted.data(), m);
    float best = INFINITY;
    int32_t at = -1;
    for (int64_t j = 0; j < m; ++j) {
      const float dx = q[0] - ref[3 * j], dy = q[1] - ref[3 * j + 1], dz = q[2] - ref[3 * j + 2];
      const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
      const float d2 = (xx + yy) + zz;
      if (d2 < best || at < 0) best = d2, at = (int32_t)j;
    }
    if (!same_bits(got.d2, best) || got.idx != at) {
      std::printf("%s: query %lld: got (%a, %d), brute force (%a, %d)\n", name, (long long)i, got.d2, got.idx, best, at);
      return false;
    }
  }
  return true;
}

std::vector<float> uniform(std::mt19937& rng, int64_t n, float a, float b) {
  std::uniform_real_distribution<float> u(a, b);
  std::vector<float> out((size_t)(3 * n));
  for (auto& x : out) x = u(rng);
  return out;
}

bool nearest_cases() {
  std::mt19937 rng(7);
  bool ok = true;
  Grid g;
  auto run = [&](const char* name, const std::vector<float>& ref, const std::vector<float>& query, float cell) {
    if (!make_grid(ref, cell, g)) return std::printf("%s: the grid has more than 1024 cells\n", name), false;
    return check_nearest(name, ref, query, g);
  };
  // empty sets
  ok &= run("m0", {}, uniform(rng, 20, -1, 1), 1.0f);
  ok &= run("n0", uniform(rng, 20, -1, 1), {}, 0.5f);
  // m = 1, all points equal
  ok &= run("m1", {0.25f, -0.5f, 0.75f}, uniform(rng, 200, -3, 3), 1.0f);
  {
    std::vector<float> eq;
    for (int j = 0; j < 50; ++j) eq.insert(eq.end(), {0.1f, 0.2f, 0.3f});
    ok &= run("all_equal", eq, uniform(rng, 200, -1, 1), 0.01f);
  }
  // points on cell faces and grid corners: an integer lattice with cell = 1 and with cell = 1/3; queries at the cube
  // centres (8-way ties), on the points, and far outside the grid
  {
    std::vector<float> lat, q;
    for (int x = 0; x < 6; ++x)
      for (int y = 0; y < 6; ++y)
        for (int z = 0; z < 6; ++z) lat.insert(lat.end(), {(float)x, (float)y, (float)z});
    q = lat;
    for (int x = 0; x < 5; ++x)
      for (int y = 0; y < 5; ++y)
        for (int z = 0; z < 5; ++z) q.insert(q.end(), {x + 0.5f, y + 0.5f, z + 0.5f});
    const std::vector<float> far = uniform(rng, 100, -60, 60);
    q.insert(q.end(), far.begin(), far.end());
    ok &= run("lattice", lat, q, 1.0f);
    ok &= run("lattice_third", lat, q, 1.0f / 3.0f);
    ok &= run("lattice_coarse", lat, q, 2.5f);
  }
  // dims = (1,1,1) and (1024,1,1)
  ok &= run("one_cell", uniform(rng, 300, -1, 1), uniform(rng, 300, -2, 2), 4.0f);
  {
    std::vector<float> line;
    std::uniform_real_distribution<float> u(0.0f, 1.0f);
    for (int j = 0; j < 1500; ++j) line.insert(line.end(), {1023.5f * u(rng), 0.0f, 0.0f});
    line.insert(line.end(), {0.0f, 0.0f, 0.0f});
    line.insert(line.end(), {1023.5f, 0.0f, 0.0f});
    std::vector<float> q = uniform(rng, 300, -5, 5);
    for (int64_t i = 0; i < 300; ++i) q[3 * i] = 1200.0f * u(rng) - 80.0f;
    ok &= run("line1024", line, q, 1.0f);
    if (g.dims[0] != 1024 || g.dims[1] != 1 || g.dims[2] != 1) ok = false, std::printf("line1024: dims\n");
  }
  // two far clusters with a fine cell: many empty shells
  {
    std::normal_distribution<float> nd(0.0f, 0.05f);
    std::vector<float> ref;
    for (int j = 0; j < 600; ++j) ref.insert(ref.end(), {nd(rng) + (j & 1 ? 3.0f : 0.0f), nd(rng), nd(rng)});
    std::vector<float> q = uniform(rng, 150, -0.3f, 0.3f);
    for (int64_t i = 0; i < 150; ++i) q[3 * i] = 0.2f + 2.6f * (float)i / 150.0f;
    const std::vector<float> far = uniform(rng, 100, -9, 9);
    q.insert(q.end(), far.begin(), far.end());
    ok &= run("clusters", ref, q, 0.1f);
  }
  // duplicates, a flat set, random sets of a few thousand points
  {
    const std::vector<float> five = uniform(rng, 5, -1, 1);
    std::vector<float> ref;
    for (int r = 0; r < 40; ++r) ref.insert(ref.end(), five.begin(), five.end());
    ok &= run("duplicates", ref, uniform(rng, 300, -1.5f, 1.5f), 0.2f);
    std::vector<float> flat = uniform(rng, 500, -1, 1);
    for (int64_t j = 0; j < 500; ++j) flat[3 * j + 2] = 0.25f;
    ok &= run("flat", flat, uniform(rng, 300, -1, 1), 0.1f);
  }
  for (float cell : {0.05f, 0.13f, 0.5f})
    ok &= run("random", uniform(rng, 3000, -1, 1), uniform(rng, 2000, -1.2f, 1.2f), cell);
  ok &= run("random_fine", uniform(rng, 4000, 0, 1), uniform(rng, 300, 0, 1), 1.0f / 1000.0f);
  return ok;
}

// ---------------------------------------------------------------- the sampler

struct Soup {
  std::vector<float> v;
  std::vector<int32_t> f;
};

bool check_sampler(const char* name, const Soup& s, const std::vector<int64_t>& weights, uint64_t seed, int64_t n,
                   bool with_vertex_normals) {
  const int64_t F = (int64_t)s.f.size() / 3, V = (int64_t)s.v.size() / 3;
  std::vector<int64_t> cdf((size_t)F);
  int64_t acc = 0;
  for (int64_t f = 0; f < F; ++f) cdf[f] = acc += weights[f];
  const uint64_t total = (uint64_t)acc;
  std::vector<float> vn;
  if (with_vertex_normals) {
    std::mt19937 rng(3);
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    vn.resize((size_t)(3 * V));
    for (auto& x : vn) x = u(rng);
  }
  std::vector<float> pts((size_t)(3 * n)), nrm((size_t)(3 * n));
  std::vector<int32_t> face((size_t)n);
  for (int64_t i = 0; i < n; ++i)
    nerf_mm::sample(s.v.data(), s.f.data(), F, cdf.data(), total, with_vertex_normals ? vn.data() : nullptr, seed, i,
                    pts.data(), face.data(), nrm.data());
  for (int64_t i = 0; i < n; ++i) {
    // the plain restatement: a 128-bit product, a linear scan of the weights, the same double operations
    const uint64_t z0 = nerf_mm::rand64(seed, 0x6d657368ULL, (uint64_t)i), z1 = nerf_mm::rand64(seed, 0x6d657369ULL, (uint64_t)i),
                   z2 = nerf_mm::rand64(seed, 0x6d65736aULL, (uint64_t)i);
    const uint64_t target = (uint64_t)(((unsigned __int128)z0 * total) >> 64);
    if (target >= total) return std::printf("%s: target not below total\n", name), false;
    int64_t f = 0;
    uint64_t run = 0;
    for (; f < F; ++f) {
      run += (uint64_t)weights[f];
      if (run > target) break;
    }
    if (f >= F || weights[f] == 0 || face[i] != f)
      return std::printf("%s: sample %lld: face %d, expected %lld\n", name, (long long)i, face[i], (long long)f), false;
    int64_t k1 = (int64_t)(z1 >> 40), k2 = (int64_t)(z2 >> 40);
    if (k1 + k2 > (1 << 24)) k1 = (1 << 24) - k1, k2 = (1 << 24) - k2;
    if (k1 < 0 || k2 < 0 || k1 + k2 > (1 << 24)) return std::printf("%s: fold\n", name), false;
    const double u1 = std::ldexp((double)k1, -24), u2 = std::ldexp((double)k2, -24);
    const int32_t* c = &s.f[3 * f];
    double g[3];
    for (int a = 0; a < 3; ++a) {
      const double o = s.v[3 * c[0] + a], e1 = (double)s.v[3 * c[1] + a] - o, e2 = (double)s.v[3 * c[2] + a] - o;
      const double t1 = u1 * e1, t2 = u2 * e2, sum = o + t1;
      if (!same_bits(pts[3 * i + a], (float)(sum + t2)))
        return std::printf("%s: sample %lld: point\n", name, (long long)i), false;
      if (with_vertex_normals) {
        const double w0 = (1.0 - u1) - u2;
        const double t0 = w0 * vn[3 * c[0] + a], s1 = u1 * vn[3 * c[1] + a], s2 = u2 * vn[3 * c[2] + a];
        g[a] = (t0 + s1) + s2;
      }
    }
    if (!with_vertex_normals) nerf_mm::face_cross(s.v.data(), s.f.data(), f, g);
    const double len = std::sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
    const double d = with_vertex_normals ? (len > 1e-12 ? len : 1e-12) : (len > 0.0 ? len : 1.0);
    for (int a = 0; a < 3; ++a)
      if (!same_bits(nrm[3 * i + a], (float)(g[a] / d)))
        return std::printf("%s: sample %lld: normal\n", name, (long long)i), false;
  }
  return true;
}

bool sampler_cases() {
  std::mt19937 rng(11);
  Soup s;
  const int64_t V = 50, F = 200;
  s.v = uniform(rng, V, -1, 1);
  std::uniform_int_distribution<int32_t> vi(0, (int32_t)V - 1);
  for (int64_t i = 0; i < 3 * F; ++i) s.f.push_back(vi(rng));
  bool ok = true;
  // the weights of the areas, as the Python layer derives them
  std::vector<double> area((size_t)F);
  double amax = 0.0;
  for (int64_t f = 0; f < F; ++f) amax = std::max(amax, area[f] = nerf_mm::face_area(s.v.data(), s.f.data(), f));
  int ex;
  std::frexp(amax, &ex);
  std::vector<int64_t> w((size_t)F);
  for (int64_t f = 0; f < F; ++f) {
    w[f] = (int64_t)std::rint(std::ldexp(area[f], 32 - ex));
    const int32_t* c = &s.f[3 * f];
    if ((c[0] == c[1] || c[1] == c[2] || c[0] == c[2]) && area[f] != 0.0) ok = false, std::printf("area of a repeated index\n");
  }
  if (*std::max_element(w.begin(), w.end()) < (int64_t(1) << 31) || *std::max_element(w.begin(), w.end()) > (int64_t(1) << 32))
    ok = false, std::printf("largest weight\n");
  for (uint64_t seed : {0ULL, 0x9e3779b97f4a7c15ULL}) {
    ok &= check_sampler("areas", s, w, seed, 3000, false);
    ok &= check_sampler("areas_vn", s, w, seed, 3000, true);
  }
  // faces of weight 0 between faces of weight > 0, at both ends too
  std::vector<int64_t> gaps((size_t)F, 0);
  for (int64_t f = 1; f + 1 < F; f += 3) gaps[f] = 1 + (f % 7);
  ok &= check_sampler("gaps", s, gaps, 5, 3000, false);
  // total near 2^62: F weights of 2^62 / F
  std::vector<int64_t> big((size_t)F, (int64_t(1) << 62) / F);
  big[3] = 0;
  ok &= check_sampler("total_2^62", s, big, 9, 3000, true);
  // one face
  Soup one{{0, 0, 0, 1, 0, 0, 0, 1, 0}, {0, 1, 2}};
  ok &= check_sampler("one_face", one, {int64_t(1) << 31}, 1, 500, false);
  ok &= check_sampler("one_face_max", one, {INT64_MAX}, 1, 500, false);
  return ok;
}

}  // namespace

int main() {
  const bool a = nearest_cases();
  const bool b = sampler_cases();
  std::printf(a && b ? "ok\n" : "FAILED\n");
  return a && b ? 0 : 1;
}
