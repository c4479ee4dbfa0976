// Host check of the lock-free hash set of csrc/mesh_simplify_core.hpp: insert and lookup, serially
// and with several host threads racing over the items, against a serial map from key to smallest item.  Stand-alone:
//
//   g++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/mesh_simplify_host_check.cpp -o mesh_simplify_host_check && ./mesh_simplify_host_check
//   g++ -std=c++17 -O1 -g -pthread -fsanitize=thread tools/mesh_simplify_host_check.cpp -o check_tsan && ./check_tsan
//
// Exit status 0 and "ok" when every case agrees.  It needs no GPU and loads nothing of the Python package.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <numeric>
#include <random>
#include <thread>
#include <vector>

#include "../nerf-sys_amd/csrc/mesh_simplify_core.hpp"

namespace {

struct SameKey {
  const int64_t* keys;
  bool operator()(int32_t a, int32_t b) const { return keys[a] == keys[b]; }
};

// the kernels' two phases on the host: insert (n_threads racing, items dealt round-robin), then lookup; compare
bool run(const char* name, const std::vector<int64_t>& keys, int table_log2, int n_threads) {
  const int32_t n = (int32_t)keys.size();
  const uint32_t mask = (uint32_t)((int64_t(1) << table_log2) - 1);
  std::vector<int32_t> table((size_t)mask + 1, nerf_hs::EMPTY);
  std::vector<uint32_t> longest(n_threads, 0);
  std::vector<int> bad(n_threads, 0);
  const SameKey same{keys.data()};
  auto work = [&](int t) {
    for (int32_t v = t; v < n; v += n_threads) {
      uint32_t probes = 0;
      if (!nerf_hs::insert(table.data(), mask, nerf_hs::mix((uint64_t)keys[v]), v, same, probes)) bad[t] = 1;
      longest[t] = std::max(longest[t], probes);
    }
  };
  std::vector<std::thread> pool;
  for (int t = 1; t < n_threads; ++t) pool.emplace_back(work, t);
  work(0);
  for (auto& th : pool) th.join();

  std::map<int64_t, int32_t> first;
  for (int32_t v = n - 1; v >= 0; --v) first[keys[v]] = v;
  bool ok = !*std::max_element(bad.begin(), bad.end());
  // one slot per key, holding the smallest item of that key
  size_t filled = 0;
  for (int32_t s : table) {
    if (s == nerf_hs::EMPTY) continue;
    ++filled;
    if (s < 0 || s >= n || first[keys[s]] != s) {
      std::printf("%s: a slot holds %d, not the smallest item of its key\n", name, s);
      ok = false;
    }
  }
  if (filled != first.size()) {
    std::printf("%s: %zu slots filled for %zu keys\n", name, filled, first.size());
    ok = false;
  }
  uint32_t look = 0;
  for (int32_t v = 0; v < n; ++v) {
    uint32_t probes = 0;
    const int32_t l = nerf_hs::lookup(table.data(), mask, nerf_hs::mix((uint64_t)keys[v]), v, same, probes);
    look = std::max(look, probes);
    if (l != first[keys[v]]) {
      std::printf("%s: lookup(%d) = %d, expected %d\n", name, v, l, first[keys[v]]);
      ok = false;
      break;
    }
  }
  std::printf("%-22s n=%-6d keys=%-6zu slots=2^%-2d threads=%d longest insert=%u lookup=%u %s\n", name, n, first.size(),
              table_log2, n_threads, *std::max_element(longest.begin(), longest.end()), look, ok ? "ok" : "MISMATCH");
  return ok;
}

int minimal_log2(int64_t n) {
  int k = 0;
  while ((int64_t(1) << k) <= n) ++k;
  return k;
}

// the canonical form and hash of faces: rotations agree, mirror images do not
bool faces_ok() {
  const int32_t tri[3][3] = {{3, 7, 5}, {7, 5, 3}, {5, 3, 7}};
  int32_t k0[3], k[3], m[3];
  nerf_hs::canonical(tri[0][0], tri[0][1], tri[0][2], k0);
  bool ok = k0[0] == 3 && k0[1] == 7 && k0[2] == 5;
  for (int r = 1; r < 3; ++r) {
    nerf_hs::canonical(tri[r][0], tri[r][1], tri[r][2], k);
    ok = ok && k[0] == k0[0] && k[1] == k0[1] && k[2] == k0[2] && nerf_hs::face_hash(k) == nerf_hs::face_hash(k0);
  }
  nerf_hs::canonical(3, 5, 7, m);
  ok = ok && m[0] == 3 && m[1] == 5 && m[2] == 7;
  std::printf("%-22s %s\n", "canonical faces", ok ? "ok" : "MISMATCH");
  return ok;
}

// the cell arithmetic at the grid's edges: clamped before the conversion, exact boundaries, a one-cell axis
bool grid_ok() {
  nerf_hs::Grid g{{-1.0f, 0.5f, 2.0f}, 0.25f, 4.0f, {5, 1, 3}};
  bool ok = nerf_hs::cell_index(g, 0, -1.0f) == 0 && nerf_hs::cell_index(g, 0, -1e30f) == 0 &&
            nerf_hs::cell_index(g, 0, 1e30f) == 4 && nerf_hs::cell_index(g, 0, 0.25f) == 4 &&
            nerf_hs::cell_index(g, 0, -0.75f) == 1 && nerf_hs::cell_index(g, 1, 77.0f) == 0 &&
            nerf_hs::cell_index(g, 2, 2.74f) == 2;
  const float p[3] = {-0.4f, 0.6f, 2.3f};  // cells (2, 0, 1)
  ok = ok && nerf_hs::cell_key(g, p) == (2 * 1 + 0) * 3 + 1;
  ok = ok && nerf_hs::quant_pos(g, 0, 0.25f) == 16777216u && nerf_hs::quant_pos(g, 0, -1.0f) == 0u &&
       nerf_hs::quant_pos(g, 0, -2.0f) == 0u && nerf_hs::quant_pos(g, 0, -0.875f) == 8388608u;
  ok = ok && nerf_hs::quant_color(NAN) == 0u && nerf_hs::quant_color(2.0f) == 16777216u &&
       nerf_hs::quant_normal(NAN) == -1048576 && nerf_hs::quant_normal(0.5f) == 524288;
  ok = ok && nerf_hs::mean_pos(g, 0, 1, 3 * 8388608ull, 3) == -0.625f && nerf_hs::mean_color(16777216ull, 2) == 0.5f;
  const int64_t zero[3] = {0, 0, 0}, up[3] = {0, 0, 5};
  float o[3];
  nerf_hs::unit_normal(zero, o);
  ok = ok && o[0] == 0.0f && o[1] == 0.0f && o[2] == 0.0f;
  nerf_hs::unit_normal(up, o);
  ok = ok && o[0] == 0.0f && o[1] == 0.0f && o[2] == 1.0f;
  std::printf("%-22s %s\n", "cell arithmetic", ok ? "ok" : "MISMATCH");
  return ok;
}

}  // namespace

int main() {
  bool ok = faces_ok();
  ok = grid_ok() && ok;
  std::mt19937_64 rng(7);
  for (int n : {1, 63, 64, 65, 255, 256, 257, 2049, 20000})
    for (int threads : {1, 8}) {
      // one key: every insert after the first meets an occupied slot or fails its compare-and-swap
      std::vector<int64_t> one(n, int64_t(1) << 40);
      ok = run("one-key", one, minimal_log2(n), threads) && ok;
      // all distinct at the minimal capacity: the load factor approaches 1 and the chains wrap around
      std::vector<int64_t> distinct(n);
      std::iota(distinct.begin(), distinct.end(), int64_t(0));
      std::shuffle(distinct.begin(), distinct.end(), rng);
      ok = run("all-distinct-minimal", distinct, minimal_log2(n), threads) && ok;
      // random keys from a small range (many members per key), in the default and in the minimal table
      std::vector<int64_t> random(n);
      for (auto& k : random) k = (int64_t)(rng() % (uint64_t)(n / 4 + 1)) * 0x100000001LL;
      ok = run("random", random, std::max(6, minimal_log2(2 * (int64_t)n - 1)), threads) && ok;
      ok = run("random-minimal", random, minimal_log2(n), threads) && ok;
    }
  std::printf(ok ? "ok\n" : "FAILED\n");
  return ok ? 0 : 1;
}
