// Host check of csrc/mesh_smooth_core.hpp: the key packing and unpacking, the lower bound, the run
// flags, the row build, the smoothing pass and the vertex normals, run serially over generated face lists exactly as
// the kernels run them (one loop iteration per thread) and compared with a std::set-based adjacency and with plain
// restatements of the arithmetic.  Stand-alone:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/mesh_smooth_host_check.cpp -o mesh_smooth_host_check && ./mesh_smooth_host_check
//
// Exit status 0 and "ok" when every case agrees.  It needs no GPU and loads nothing of the Python package.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>
#include <vector>

#include "../nerf-sys_amd/csrc/mesh_smooth_core.hpp"

namespace {

struct Csr {
  std::vector<int32_t> row_off, col;
  std::vector<uint8_t> boundary;
};

// the device pipeline on the host: keys -> sort -> flags (+ boundary) -> exclusive scan -> build
Csr build(const std::vector<int32_t>& faces, int64_t V, int mode) {
  const int64_t F = (int64_t)faces.size() / 3, n = (mode == 0 ? 6 : 3) * F;
  std::vector<int64_t> keys((size_t)n);
  for (int64_t i = 0; i < n; ++i)
    keys[i] = mode == 0 ? nerf_ms::pair_key(faces.data(), i) : nerf_ms::vertex_face_key(faces.data(), i);
  std::sort(keys.begin(), keys.end());
  std::vector<int32_t> flags((size_t)n), pos((size_t)n + 1, 0);
  Csr out;
  out.boundary.assign((size_t)V, 0);
  for (int64_t i = 0; i < n; ++i) {
    flags[i] = nerf_ms::run_flag(keys.data(), i);
    if (mode == 0 && flags[i] && nerf_ms::run_is_single(keys.data(), n, i))
      out.boundary[nerf_ms::key_row(keys[i])] = 1;
  }
  for (int64_t i = 0; i < n; ++i) pos[i + 1] = pos[i] + flags[i];
  const int64_t E = pos[n];
  out.col.assign((size_t)E, -1);
  out.row_off.assign((size_t)V + 1, -1);
  for (int64_t i = 0; i < n; ++i)
    if (flags[i]) out.col[pos[i]] = nerf_ms::key_entry(keys[i]);
  for (int64_t v = 0; v <= V; ++v) out.row_off[v] = nerf_ms::row_start(keys.data(), n, pos.data(), v);
  return out;
}

bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; }

bool run(const char* name, const std::vector<int32_t>& faces, int64_t V, uint32_t seed) {
  const int64_t F = (int64_t)faces.size() / 3;
  bool ok = true;
  auto fail = [&](const char* what, int64_t at) {
    if (ok) std::printf("%s: %s at %lld\n", name, what, (long long)at);
    ok = false;
  };
  // the references: sets of neighbours and of faces per vertex, and the count of every directed pair
  std::vector<std::set<int32_t>> nb((size_t)V), vf((size_t)V);
  std::multiset<std::pair<int32_t, int32_t>> pairs;
  for (int64_t f = 0; f < F; ++f)
    for (int e = 0; e < 3; ++e) {
      const int32_t a = faces[3 * f + e], b = faces[3 * f + (e + 1) % 3];
      vf[a].insert((int32_t)f);
      if (a == b) continue;
      nb[a].insert(b), nb[b].insert(a);
      pairs.insert({a, b}), pairs.insert({b, a});
    }
  const Csr adj = build(faces, V, 0), vfc = build(faces, V, 1);
  for (int pass = 0; pass < 2; ++pass) {
    const Csr& c = pass ? vfc : adj;
    const auto& ref = pass ? vf : nb;
    if (c.row_off[0] != 0 || c.row_off[V] != (int32_t)c.col.size()) fail("row_off ends", pass);
    for (int64_t v = 0; v < V && ok; ++v) {
      if (c.row_off[v + 1] < c.row_off[v]) fail("row_off decreases", v);
      const std::vector<int32_t> row(c.col.begin() + c.row_off[v], c.col.begin() + c.row_off[v + 1]);
      if (row != std::vector<int32_t>(ref[v].begin(), ref[v].end())) fail(pass ? "face row" : "neighbour row", v);
    }
  }
  for (int64_t v = 0; v < V && ok; ++v) {
    bool once = false;
    for (int32_t u : nb[v]) once = once || pairs.count({(int32_t)v, u}) == 1;
    if (adj.boundary[v] != (once ? 1 : 0)) fail("boundary", v);
  }
  if (!ok) return false;

  // the pass and the normals against their restatements
  std::mt19937 rng(seed);
  std::uniform_real_distribution<float> uni(-1.0f, 1.0f);
  std::vector<float> p((size_t)(3 * V)), out((size_t)(3 * V)), nrm((size_t)(3 * V));
  std::vector<uint8_t> fixed((size_t)V);
  for (auto& x : p) x = uni(rng);
  if (V) p[0] = -0.0f;
  for (auto& x : fixed) x = (rng() % 4) == 0;
  const float factors[4] = {0.0f, 0.5f, 1.0f, -0.53f};
  for (float s : factors)
    for (int with_fixed = 0; with_fixed < 2; ++with_fixed) {
      const uint8_t* fx = with_fixed ? fixed.data() : nullptr;
      for (int64_t v = 0; v < V; ++v)
        nerf_ms::smooth_vertex(p.data(), adj.row_off.data(), adj.col.data(), fx, v, s, out.data());
      for (int64_t v = 0; v < V && ok; ++v)
        for (int c = 0; c < 3; ++c) {
          float want = p[3 * v + c];
          if (!nb[v].empty() && s != 0.0f && !(fx && fx[v])) {
            volatile double acc = 0.0;  // volatile: one rounded addition at a time, whatever the compiler would like
            bool first = true;
            for (int32_t u : nb[v]) {
              acc = first ? (double)p[3 * u + c] : acc + (double)p[3 * u + c];
              first = false;
            }
            volatile double m = acc / (double)nb[v].size();
            volatile double diff = m - (double)p[3 * v + c];
            volatile double step = (double)s * diff;
            want = (float)((double)p[3 * v + c] + step);
          }
          if (!same_bits(out[3 * v + c], want)) fail("smoothing pass", v);
        }
    }
  for (int64_t v = 0; v < V; ++v)
    nerf_ms::vertex_normal(p.data(), faces.data(), vfc.row_off.data(), vfc.col.data(), v, nrm.data());
  for (int64_t v = 0; v < V && ok; ++v) {
    volatile double g[3] = {0.0, 0.0, 0.0};
    for (int32_t f : vf[v]) {
      const int32_t* t = &faces[3 * (int64_t)f];
      volatile double a[3], b[3];
      for (int c = 0; c < 3; ++c) {
        a[c] = (double)p[3 * t[1] + c] - (double)p[3 * t[0] + c];
        b[c] = (double)p[3 * t[2] + c] - (double)p[3 * t[0] + c];
      }
      for (int c = 0; c < 3; ++c) {
        const int i = (c + 1) % 3, j = (c + 2) % 3;
        volatile double l = a[i] * b[j], r = a[j] * b[i];
        g[c] = g[c] + (l - r);
      }
    }
    volatile double xx = g[0] * g[0], yy = g[1] * g[1], zz = g[2] * g[2];
    volatile double xy = xx + yy;
    const double len = std::sqrt(xy + zz);
    for (int c = 0; c < 3; ++c)
      if (!same_bits(nrm[3 * v + c], (float)(g[c] / std::max(len, 1e-12)))) fail("vertex normal", v);
    if (vf[v].empty() && (nrm[3 * v] != 0.0f || nrm[3 * v + 1] != 0.0f || nrm[3 * v + 2] != 0.0f))
      fail("normal of an unused vertex", v);
  }
  return ok;
}

bool keys_check() {
  bool ok = true;
  const int32_t big = 0x7fffffff - 1;  // V - 1 for the largest V: the row uses every bit of the key's upper half
  const int32_t rows[4] = {0, 1, 65536, big}, entries[4] = {0, 7, 0x7fffffff, big};
  for (int32_t r : rows)
    for (int32_t e : entries) {
      const int64_t k = nerf_ms::pack(r, e);
      if (k < 0 || k == nerf_ms::SENTINEL || nerf_ms::key_row(k) != r || nerf_ms::key_entry(k) != e) ok = false;
      if (k < nerf_ms::pack(r, 0) || (r < big && k >= nerf_ms::pack(r + 1, 0))) ok = false;  // ordered by (row, entry)
    }
  // two vertices at the top of the index range: the rows of V - 2 and V - 1 and the row start of V itself
  const int64_t V = 0x7fffffff;
  const std::vector<int32_t> faces = {big, big - 1, 3, 3, 3, 3};
  std::vector<int64_t> keys;
  for (int64_t i = 0; i < 12; ++i) keys.push_back(nerf_ms::pair_key(faces.data(), i));
  std::sort(keys.begin(), keys.end());
  std::vector<int32_t> pos(13, 0);
  for (int64_t i = 0; i < 12; ++i) pos[i + 1] = pos[i] + nerf_ms::run_flag(keys.data(), i);
  const int64_t probe[6] = {0, 3, 4, big - 1, big, V};
  const int32_t want[6] = {0, 0, 2, 2, 4, 6};
  for (int i = 0; i < 6; ++i)
    if (nerf_ms::row_start(keys.data(), 12, pos.data(), probe[i]) != want[i]) ok = false;
  if (pos[12] != 6 || keys[6] != nerf_ms::SENTINEL) ok = false;
  // the lower bound on every position of a sorted array with runs, and on the empty array
  const std::vector<int64_t> a = {1, 1, 4, 4, 4, 9, nerf_ms::SENTINEL, nerf_ms::SENTINEL};
  for (int64_t t = 0; t <= 10; ++t)
    if (nerf_ms::lower_bound(a.data(), 8, t) != std::lower_bound(a.begin(), a.end(), t) - a.begin()) ok = false;
  if (nerf_ms::lower_bound(a.data(), 8, nerf_ms::SENTINEL) != 6 || nerf_ms::lower_bound(nullptr, 0, 5) != 0) ok = false;
  if (!ok) std::printf("keys: packing, order or lower bound\n");
  return ok;
}

std::vector<int32_t> soup(int64_t V, int64_t F, uint32_t seed) {
  std::mt19937 rng(seed);
  std::vector<int32_t> f((size_t)(3 * F));
  for (auto& x : f) x = (int32_t)(rng() % (uint32_t)V);
  return f;
}

}  // namespace

int main() {
  bool ok = keys_check();
  ok &= run("empty", {}, 0, 1);
  ok &= run("no faces", {}, 5, 2);
  ok &= run("one triangle", {0, 1, 2}, 3, 3);
  ok &= run("two triangles and unused vertices", {1, 2, 4, 4, 2, 6}, 9, 4);
  {
    std::vector<int32_t> fan;  // centre 0, rim 1..1000, closed
    for (int32_t i = 1; i <= 1000; ++i) fan.insert(fan.end(), {0, i, i % 1000 + 1});
    ok &= run("fan 1000", fan, 1001, 5);
    fan.resize(fan.size() - 3);
    ok &= run("open fan", fan, 1001, 6);
  }
  ok &= run("all degenerate: every key is the sentinel", {0, 0, 0, 2, 2, 2, 3, 3, 3, 2, 2, 2}, 4, 7);
  ok &= run("repeated indices", {0, 0, 1, 2, 2, 2, 3, 1, 3, 1, 2, 2}, 4, 9);
  ok &= run("duplicated and mirrored", {0, 1, 2, 2, 1, 3, 0, 1, 2, 0, 2, 1, 3, 1, 2}, 4, 8);
  const int64_t sizes[][2] = {{1, 4}, {2, 9}, {63, 250}, {64, 256}, {65, 260}, {257, 1000}, {2049, 8000}, {5000, 20000},
                              {40, 20000}};
  uint32_t seed = 100;
  for (const auto& s : sizes) {
    char name[64];
    std::snprintf(name, sizeof name, "soup V=%lld F=%lld", (long long)s[0], (long long)s[1]);
    ok &= run(name, soup(s[0], s[1], seed), s[0], seed + 1);
    seed += 2;
  }
  std::printf(ok ? "ok\n" : "FAILED\n");
  return ok ? 0 : 1;
}
