// Host check of csrc/mesh_distance_core.hpp: the face registration, the grid search run serially, one
// loop iteration per thread exactly as the kernels call it, against a brute-force search over all faces (d2 bits,
// face index, closest-point bits), on a random soup with faces without area and on a mesh with one huge face.
// Stand-alone:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/mesh_distance_host_check.cpp -o mesh_distance_host_check && ./mesh_distance_host_check
//
// Exit status 0 and "ok" when every case agrees.  It needs no GPU and loads nothing of the Python package.
// With an argument it also writes d2 (hex float), face and closest point of every query of the first soup case to
// that file, for a comparison with tests/mesh_distance_reference.py.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../nerf-sys_amd/csrc/mesh_distance_core.hpp"
#include "mesh_host_check_common.hpp"

namespace {

using namespace mesh_check;

template <class T>
bool same_bits(T a, T b) {
  return std::memcmp(&a, &b, sizeof a) == 0;
}

bool check(const char* name, const Soup& s, const std::vector<float>& query, float cell, std::FILE* dump = nullptr) {
  Grid g;
  if (!make_grid(s.v, cell, g)) return std::printf("%s: the grid has more than 1024 cells\n", name), false;
  const int64_t F = (int64_t)s.f.size() / 3, n = (int64_t)query.size() / 3;
  // registration: counts, an exclusive sum, the keys of every face at its offset, a sort
  std::vector<int64_t> offsets((size_t)F + 1, 0);
  for (int64_t f = 0; f < F; ++f) {
    const int64_t count = nerf_md::face_cell_count(g, s.v.data(), s.f.data(), f);
    if (count < 1) return std::printf("%s: face %lld has no cell\n", name, (long long)f), false;
    offsets[f + 1] = offsets[f] + count;
  }
  const int64_t n_keys = offsets[F];
  if (n_keys >= (int64_t(1) << 31)) return std::printf("%s: too many keys\n", name), false;
  std::vector<int64_t> keys((size_t)n_keys, -1);
  for (int64_t f = 0; f < F; ++f) {
    nerf_md::face_keys(g, s.v.data(), s.f.data(), f, keys.data() + offsets[f]);
    for (int64_t j = offsets[f]; j < offsets[f + 1]; ++j) {
      if ((int64_t)((uint64_t)keys[j] & 0xffffffffu) != f || (j > offsets[f] && keys[j] <= keys[j - 1]))
        return std::printf("%s: keys of face %lld\n", name, (long long)f), false;
    }
    int32_t lo[3], hi[3];  // every corner's own cell lies in the face's box
    nerf_md::face_box(g, s.v.data(), s.f.data(), f, lo, hi);
    for (int k = 0; k < 3; ++k)
      for (int c = 0; c < 3; ++c) {
        const int32_t i = nerf_mm::cell_index(g, c, s.v[3 * s.f[3 * f + k] + c]);
        if (i < lo[c] || i > hi[c]) return std::printf("%s: a corner outside its face's box\n", name), false;
      }
  }
  std::sort(keys.begin(), keys.end());
  for (int64_t i = 0; i < n; ++i) {
    const float* q = &query[3 * i];
    const nerf_md::BestFace got = nerf_md::nearest_face(g, q, keys.data(), n_keys, s.v.data(), s.f.data());
    nerf_md::BestFace best = {(double)INFINITY, -1, {q[0], q[1], q[2]}};
    for (int64_t f = 0; f < F; ++f) {
      float r[3];
      const double d2 = nerf_md::closest_on_face(s.v.data(), s.f.data(), f, q, r);
      if (!(d2 >= 0.0) || !std::isfinite(d2) || !std::isfinite(r[0]) || !std::isfinite(r[1]) || !std::isfinite(r[2]))
        return std::printf("%s: query %lld face %lld: d2 = %a\n", name, (long long)i, (long long)f, d2), false;
      if (d2 < best.d2 || best.face < 0) best.d2 = d2, best.face = (int32_t)f, std::memcpy(best.p, r, sizeof r);
    }
    if (!same_bits(got.d2, best.d2) || got.face != best.face || std::memcmp(got.p, best.p, sizeof got.p) != 0) {
      std::printf("%s: query %lld: got (%a, %d), brute force (%a, %d)\n", name, (long long)i, got.d2, got.face, best.d2,
                  best.face);
      return false;
    }
    if (dump) std::fprintf(dump, "%a %d %a %a %a\n", got.d2, got.face, got.p[0], got.p[1], got.p[2]);
  }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  std::mt19937 rng(5);
  bool ok = true;
  // the table of the issue: one query per region of the walk
  {
    const Soup one{{0, 0, 0, 1, 0, 0, 0, 1, 0}, {0, 1, 2}};
    const float q[9][3] = {{.25f, .25f, 1}, {-1, -1, 0}, {2, 0, 0}, {0, 3, 0}, {1, 1, 0}, {.5f, -2, 0}, {-2, .5f, 0},
                           {.25f, .25f, 0}, {1, 1, 1}};
    const double want[9] = {1, 2, 1, 4, 0.5, 4, 4, 0, 1.5};
    for (int i = 0; i < 9; ++i) {
      float r[3];
      const double d2 = nerf_md::closest_on_face(one.v.data(), one.f.data(), 0, q[i], r);
      if (d2 != want[i]) ok = false, std::printf("table row %d: d2 = %a\n", i, d2);
    }
  }
  const Soup s = soup(rng, 40, 60);
  std::vector<float> q = uniform(rng, 900, -1.2f, 1.2f);
  const std::vector<float> far = uniform(rng, 100, -60, 60);
  q.insert(q.end(), far.begin(), far.end());
  std::FILE* dump = argc > 1 ? std::fopen(argv[1], "w") : nullptr;
  if (dump) {
    for (size_t i = 0; i < s.v.size(); ++i) std::fprintf(dump, "v %a\n", s.v[i]);
    for (size_t i = 0; i < s.f.size(); ++i) std::fprintf(dump, "f %d\n", s.f[i]);
    for (size_t i = 0; i < q.size(); ++i) std::fprintf(dump, "q %a\n", q[i]);
  }
  ok &= check("soup", s, q, 0.5f, dump);
  if (dump) std::fclose(dump);
  ok &= check("soup_one_cell", s, q, 4.0f);
  ok &= check("soup_fine", s, q, 2.0f / 40.0f);
  // every face without area
  {
    Soup dead = s;
    dead.f.resize(15);
    ok &= check("dead", dead, q, 0.25f);
  }
  // no face at all
  {
    Soup none;
    none.v = s.v;
    ok &= check("no_faces", none, q, 0.5f);
  }
  // one huge face over a cloud of small ones: the huge face is registered in every cell of a 64 x 64 x 1 slab
  {
    Soup big;
    big.v = {-8, -8, 0, 24, -8, 0, -8, 24, 0};
    big.f = {0, 1, 2};
    std::uniform_real_distribution<float> u(-8.0f, 8.0f), e(-0.2f, 0.2f);
    for (int t = 0; t < 200; ++t) {
      const float c[3] = {u(rng), u(rng), u(rng)};
      const int32_t base = (int32_t)big.v.size() / 3;
      for (int k = 0; k < 3; ++k) big.v.insert(big.v.end(), {c[0] + e(rng), c[1] + e(rng), c[2] + e(rng)});
      big.f.insert(big.f.end(), {base, base + 1, base + 2});
    }
    std::vector<float> bq = uniform(rng, 400, -9, 9);
    const std::vector<float> bfar = uniform(rng, 50, -100, 100);
    bq.insert(bq.end(), bfar.begin(), bfar.end());
    ok &= check("huge_face", big, bq, 0.5f);
    ok &= check("huge_face_coarse", big, bq, 5.0f);
  }
  // 1024 cells along one axis
  {
    Soup line;
    std::uniform_real_distribution<float> u(0.0f, 1.0f);
    line.v = {0, 0, 0, 1023.5f, 0, 0, 0, 1, 0};
    line.f = {0, 1, 2};
    for (int t = 0; t < 300; ++t) {
      const float x = 1020.0f * u(rng);
      const int32_t base = (int32_t)line.v.size() / 3;
      line.v.insert(line.v.end(), {x, u(rng), 0, x + 3.0f * u(rng), u(rng), 0, x, u(rng), 0});
      line.f.insert(line.f.end(), {base, base + 1, base + 2});
    }
    std::vector<float> lq = uniform(rng, 300, -5, 5);
    for (int64_t i = 0; i < 300; ++i) lq[3 * i] = 1200.0f * u(rng) - 80.0f;
    ok &= check("line1024", line, lq, 1.0f);
  }
  std::printf(ok ? "ok\n" : "FAILED\n");
  return ok ? 0 : 1;
}
