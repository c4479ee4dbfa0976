// Host check of csrc/mesh_inside_core.hpp: the face registration of mesh_distance_core.hpp, then the
// column walk of every query run serially, one loop iteration per thread exactly as the kernel calls it, against the
// test of every face in turn (crossings and winding), on a random soup with faces without area, on a mesh with one
// tiny and one large face at 1024 cells per axis and on a closed sphere, over three grids each; the exact sign of the
// orientation against int64 arithmetic on integer-valued coordinates below 2^20, scaled by powers of two; the tables
// of the contract; the box points against the counter random numbers.  Stand-alone:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/mesh_inside_host_check.cpp -o mesh_inside_host_check && ./mesh_inside_host_check
//
// Exit status 0 and "ok" when every case agrees.  It needs no GPU and loads nothing of the Python package.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "../nerf-sys_amd/csrc/mesh_inside_core.hpp"
#include "mesh_host_check_common.hpp"

namespace {

using namespace mesh_check;

struct Tally {
  int64_t queries = 0, inside = 0, scanned = 0, tested = 0, exact = 0, odd_winding = 0;
  int32_t wmin = 0, wmax = 0;
};

// the walk of every query against the test of every face; query (n, 3)
bool check(const char* name, const Soup& s, const std::vector<float>& query, float cell, Tally* tally = nullptr) {
  Grid g;
  if (!make_grid(s.v, cell, g)) return std::printf("%s: the grid has more than 1024 cells\n", name), false;
  const int64_t F = (int64_t)s.f.size() / 3, n = (int64_t)query.size() / 3;
  const std::vector<int64_t> keys = sorted_keys(g, s);
  const int64_t n_keys = (int64_t)keys.size();
  if (n_keys >= (int64_t(1) << 31)) return std::printf("%s: too many keys\n", name), false;
  for (int64_t i = 0; i < n; ++i) {
    const float* q = query.data() + 3 * i;
    int64_t counts[3];
    const nerf_mi::Count got = nerf_mi::count_crossings(g, q, keys.data(), n_keys, s.v.data(), s.f.data(), counts);
    const nerf_mi::Count want = nerf_mi::brute(q, s.v.data(), s.f.data(), F);
    if (got.crossings != want.crossings || got.winding != want.winding) {
      std::printf("%s: query %lld (%a, %a, %a): got (%d, %d), brute force (%d, %d)\n", name, (long long)i, q[0], q[1],
                  q[2], got.crossings, got.winding, want.crossings, want.winding);
      return false;
    }
    if (counts[0] > n_keys || counts[1] > F || counts[1] > counts[0])
      return std::printf("%s: query %lld: %lld keys, %lld faces\n", name, (long long)i, (long long)counts[0],
                         (long long)counts[1]), false;
    if (tally) {
      tally->queries += 1, tally->inside += got.crossings & 1, tally->scanned += counts[0], tally->tested += counts[1];
      tally->exact += counts[2], tally->odd_winding += (got.winding != 0) != ((got.crossings & 1) != 0);
      tally->wmin = std::min(tally->wmin, got.winding), tally->wmax = std::max(tally->wmax, got.winding);
    }
  }
  return true;
}

// ---------------------------------------------------------------- queries

// n random points of the box widened by a tenth of its extent, then the columns of every vertex and of the fp32
// midpoint of every face's first edge, each from below the box and from a random height
std::vector<float> queries(std::mt19937& rng, const Soup& s, int64_t n) {
  const Box b = box_of(s.v);
  std::uniform_real_distribution<float> u(0.0f, 1.0f);
  std::vector<float> q;
  for (int64_t i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) q.push_back(b.lo[k] - 0.1f * b.ext + u(rng) * (b.hi[k] - b.lo[k] + 0.2f * b.ext));
  auto column = [&](float x, float y) {
    q.insert(q.end(), {x, y, b.lo[2] - 0.5f});
    q.insert(q.end(), {x, y, b.lo[2] + u(rng) * (b.hi[2] - b.lo[2])});
  };
  for (size_t j = 0; j < s.v.size() / 3; ++j) column(s.v[3 * j], s.v[3 * j + 1]);
  for (size_t f = 0; f < s.f.size() / 3; ++f) {
    const float* a = s.v.data() + 3 * s.f[3 * f];
    const float* c = s.v.data() + 3 * s.f[3 * f + 1];
    column((a[0] + c[0]) * 0.5f, (a[1] + c[1]) * 0.5f);
  }
  return q;
}

bool three_grids(const char* name, std::mt19937& rng, const Soup& s, const float cells[3], const std::vector<float>& q,
                 bool closed) {
  bool ok = true;
  for (int c = 0; c < 3; ++c) {
    Tally tally;
    char label[96];
    std::snprintf(label, sizeof label, "%s/cell %g", name, cells[c]);
    ok &= check(label, s, q, cells[c], &tally);
    if (tally.queries)
      std::printf("%-28s inside %5.1f %%  keys %8.1f  faces tested %7.1f per query  exact path %lld  winding %d..%d\n",
                  label, 100.0 * tally.inside / tally.queries, (double)tally.scanned / tally.queries,
                  (double)tally.tested / tally.queries, (long long)tally.exact, tally.wmin, tally.wmax);
    if (closed && (tally.odd_winding || tally.wmin < 0 || tally.wmax > 1))
      ok = false, std::printf("%s: a closed mesh wound outwards has winding %d..%d\n", label, tally.wmin, tally.wmax);
  }
  (void)rng;
  return ok;
}

// ---------------------------------------------------------------- the exact sign

int sign64(int64_t x) { return (x > 0) - (x < 0); }

bool orient_against_int64(std::mt19937& rng) {
  bool ok = true;
  std::uniform_int_distribution<int32_t> big(-(1 << 20) + 1, (1 << 20) - 1), small(-3, 3), shift(-40, 40);
  int64_t zeros = 0, exact = 0;
  for (int i = 0; i < 200000 && ok; ++i) {
    int64_t p[2], q[2], r[2];
    const int kind = i % 4;
    p[0] = big(rng), p[1] = big(rng);
    if (kind == 0) {  // anywhere
      q[0] = big(rng), q[1] = big(rng), r[0] = big(rng), r[1] = big(rng);
    } else if (kind == 1) {  // a few units apart, far from the origin
      q[0] = p[0] + small(rng), q[1] = p[1] + small(rng), r[0] = p[0] + small(rng), r[1] = p[1] + small(rng);
    } else {  // exactly collinear, then (kind 3) one unit off
      const int64_t dx = small(rng) * 50 + small(rng), dy = small(rng) * 50 + small(rng), j = small(rng) * 40, k = small(rng) * 30;
      q[0] = p[0] + j * dx, q[1] = p[1] + j * dy, r[0] = p[0] + k * dx + (kind == 3), r[1] = p[1] + k * dy;
    }
    bool fits = true;
    for (int64_t x : {q[0], q[1], r[0], r[1]}) fits &= x > -(1 << 20) && x < (1 << 20);
    if (!fits) continue;
    const int want = sign64((q[0] - p[0]) * (r[1] - p[1]) - (q[1] - p[1]) * (r[0] - p[0]));
    const float sx = ldexpf(1.0f, shift(rng)), sy = ldexpf(1.0f, shift(rng));  // exact scalings keep the sign
    int64_t took = 0;
    const int got = nerf_mi::orient((float)p[0] * sx, (float)p[1] * sy, (float)q[0] * sx, (float)q[1] * sy,
                                    (float)r[0] * sx, (float)r[1] * sy, &took);
    zeros += want == 0, exact += took;
    if (got != want)
      ok = false, std::printf("orient: (%lld %lld) (%lld %lld) (%lld %lld): got %d, int64 %d\n", (long long)p[0],
                              (long long)p[1], (long long)q[0], (long long)q[1], (long long)r[0], (long long)r[1], got, want);
  }
  std::printf("orient against int64: %lld zeros, %lld through the exact path\n", (long long)zeros, (long long)exact);
  if (zeros < 1000 || exact < zeros) ok = false, std::printf("orient: the hard cases were not met\n");
  // cancellation across the exponent range: the expansion alone
  if (nerf_mi::exact_sign6(1e300, 1.0, -1e300, -1.0, 0x1p-1000, 0.0) != 1 ||
      nerf_mi::exact_sign6(1e300, 1.0, -1e300, -1.0, -0x1p-1000, 0.0) != -1 ||
      nerf_mi::exact_sign6(1e300, 1.0, -1e300, -1.0, 0.0, 0.0) != 0 || nerf_mi::exact_sign6(0, 0, 0, 0, 0, 0) != 0)
    ok = false, std::printf("exact_sign6: cancellation\n");
  return ok;
}

}  // namespace

int main() {
  std::mt19937 rng(7);
  bool ok = orient_against_int64(rng);
  // the tables of the contract
  {
    const Soup one{{0, 0, 0, 1, 0, 0, 0, 1, 0}, {0, 1, 2}}, flipped{{0, 0, 0, 1, 0, 0, 0, 1, 0}, {0, 2, 1}};
    const float rows[7][3] = {{.25f, .25f, 1}, {.5f, 0, 1}, {0, .5f, 1}, {.5f, .5f, 0}, {0, 0, 1}, {1, 0, 0}, {0, 1, 0}};
    for (const auto& row : rows) {
      for (float qz : {-1.0f, 0.0f, 1.0f}) {
        const float q[3] = {row[0], row[1], qz};
        const nerf_mi::Count a = nerf_mi::brute(q, one.v.data(), one.f.data(), 1);
        const nerf_mi::Count b = nerf_mi::brute(q, flipped.v.data(), flipped.f.data(), 1);
        const int want = qz < 0 ? (int)row[2] : 0;
        if (a.crossings != want || a.winding != want || b.crossings != want || b.winding != -want)
          ok = false, std::printf("table (%g, %g, %g): (%d, %d) and (%d, %d)\n", q[0], q[1], q[2], a.crossings, a.winding,
                                  b.crossings, b.winding);
        ok &= check("table", one, std::vector<float>(q, q + 3), 0.25f);
      }
    }
    const Soup octa{{1, 0, 0, -1, 0, 0, 0, 1.5f, 0, 0, -1.5f, 0, 0, 0, 2, 0, 0, -2},
                    {0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5}};
    const float cases[6][5] = {{0, 0, 0, 1, 1},    {0, 0, 2, 0, 0},  {.5f, 0, -2, 2, 0},
                               {1, 0, -2, 0, 0},   {0, 1, -2, 2, 0}, {.5f, .5f, 0, 1, 1}};
    for (const auto& c : cases) {
      const nerf_mi::Count got = nerf_mi::brute(c, octa.v.data(), octa.f.data(), 8);
      if (got.crossings != (int)c[3] || got.winding != (int)c[4])
        ok = false, std::printf("octahedron (%g, %g, %g): (%d, %d)\n", c[0], c[1], c[2], got.crossings, got.winding);
      ok &= check("octahedron", octa, std::vector<float>(c, c + 3), 0.5f);
    }
  }
  // a random soup with faces without area: one cell, a coarse grid, 32 cells per axis
  {
    const Soup s = soup(rng, 40, 60);
    const float cells[3] = {4.0f, 0.5f, 2.0f / 31.5f};
    ok &= three_grids("soup", rng, s, cells, queries(rng, s, 1000), false);
    Soup none;  // no face at all
    none.v = s.v;
    ok &= check("no_faces", none, queries(rng, s, 50), 0.5f);
  }
  // one tiny and one large face, up to 1024 cells per axis; queries under both faces and far outside the grid
  {
    const Soup s{{0, 0, 0, 1, 0, 0, 0, 1, 0, 2, 2, 2, 2 + 0x1p-17f, 2, 2, 2, 2 + 0x1p-17f, 2}, {3, 4, 5, 0, 1, 2}};
    std::vector<float> q = queries(rng, s, 1000);
    for (int i = -1; i < 10; ++i)
      for (int j = -1; j < 10; ++j)
        for (float z : {1.5f, 2.0f - 0x1p-18f, 2.0f, -50.0f})
          q.insert(q.end(), {2.0f + (float)i * 0x1p-20f, 2.0f + (float)j * 0x1p-20f, z});
    for (float x : {-1e6f, 0.25f, 1e6f})
      for (float z : {-1e6f, 1e6f}) q.insert(q.end(), {x, 0.25f, z});
    const float cells[3] = {5.0f, 2.0f, (2.0f + 0x1p-17f) / 1023.5f};
    ok &= three_grids("tiny_face", rng, s, cells, q, false);
  }
  // a closed sphere wound outwards: parity and winding agree, and agree with the analytic sphere away from it
  {
    const float centre[3] = {0.3f, -0.2f, 1.1f};
    const Soup s = sphere(16, 24, 0.8f, centre);
    const std::vector<float> q = queries(rng, s, 2000);
    const float cells[3] = {4.0f, 0.2f, 1.6f / 31.5f};
    ok &= three_grids("sphere", rng, s, cells, q, true);
    int64_t judged = 0;
    for (size_t i = 0; i < q.size() / 3; ++i) {
      const double d[3] = {q[3 * i] - (double)centre[0], q[3 * i + 1] - (double)centre[1], q[3 * i + 2] - (double)centre[2]};
      const double r = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
      if (std::fabs(r - 0.8) < 0.05) continue;  // the polyhedron lies within 0.8 (1 - cos(pi / 16)) < 0.016 of the sphere
      const nerf_mi::Count got = nerf_mi::brute(q.data() + 3 * i, s.v.data(), s.f.data(), (int64_t)s.f.size() / 3);
      ++judged;
      if ((got.winding == 1) != (r < 0.8) || (got.crossings & 1) != (r < 0.8))
        ok = false, std::printf("sphere: query %zu at r = %g: (%d, %d)\n", i, r, got.crossings, got.winding);
    }
    if (4 * judged < 3 * (int64_t)(q.size() / 3)) ok = false, std::printf("sphere: only %lld queries judged\n", (long long)judged);
  }
  // the box points: the counter random numbers, the fp32 arithmetic, a prefix of a longer run
  {
    const float lo[3] = {-1.0f, 0.5f, 2.0f}, hi[3] = {1.0f, 0.75f, 2.0f};
    std::vector<float> p(3 * 257), again(3 * 100);
    for (int64_t i = 0; i < 257; ++i) nerf_mi::box_point(5, i, lo, hi, p.data());
    for (int64_t i = 0; i < 100; ++i) nerf_mi::box_point(5, i, lo, hi, again.data());
    for (int64_t i = 0; i < 257; ++i)
      for (int c = 0; c < 3; ++c) {
        const uint64_t k = nerf_mm::rand64(5, nerf_mi::BOX_STREAM + (uint64_t)c, (uint64_t)i) >> 40;
        const float want = lo[c] + (float)((double)k / 16777216.0) * (hi[c] - lo[c]);
        if (p[3 * i + c] != want || !(p[3 * i + c] >= lo[c] && p[3 * i + c] <= hi[c]) || (i < 100 && again[3 * i + c] != want))
          ok = false, std::printf("box point %lld[%d]: %a, expected %a\n", (long long)i, c, p[3 * i + c], want);
      }
    if (nerf_mi::BOX_STREAM == nerf_mm::SAMPLE_STREAM) ok = false;
  }
  std::printf(ok ? "ok\n" : "FAILED\n");
  return ok ? 0 : 1;
}
