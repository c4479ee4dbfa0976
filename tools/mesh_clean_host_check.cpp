// Host check of the lock-free union-find of csrc/mesh_clean_core.hpp: the strip cases of the tests,
// serially and with several host threads racing over the faces, against a plain serial union-find.  Stand-alone:
//
//   g++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/mesh_clean_host_check.cpp -o mesh_clean_host_check && ./mesh_clean_host_check
//
// Exit status 0 and "ok" when every case agrees.  It needs no GPU and loads nothing of the Python package.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <thread>
#include <vector>

#include "../nerf-sys_amd/csrc/mesh_clean_core.hpp"

namespace {

std::vector<int32_t> serial_labels(const std::vector<int32_t>& faces, int32_t V) {
  std::vector<int32_t> p(V);
  std::iota(p.begin(), p.end(), 0);
  auto find = [&](int32_t v) {
    while (p[v] != v) v = p[v] = p[p[v]];
    return v;
  };
  for (size_t f = 0; f < faces.size() / 3; ++f)
    for (int k = 0; k < 2; ++k) {
      const int32_t a = find(faces[3 * f + k]), b = find(faces[3 * f + k + 1]);
      if (a != b) p[std::max(a, b)] = std::min(a, b);
    }
  std::vector<int32_t> out(V);
  for (int32_t v = 0; v < V; ++v) out[v] = find(v);
  return out;
}

// the kernels' three phases on the host: unite (n_threads racing, faces dealt round-robin), flatten, compare
bool run(const char* name, const std::vector<int32_t>& faces, int32_t V, int n_threads) {
  std::vector<int32_t> parent(V);
  std::iota(parent.begin(), parent.end(), 0);
  const size_t F = faces.size() / 3;
  std::vector<uint32_t> steps(n_threads, 0);
  std::vector<int> bad(n_threads, 0);
  auto work = [&](int t) {
    for (size_t f = t; f < F; f += n_threads) {
      uint32_t s = 0;
      if (!nerf_uf::unite_face(parent.data(), &faces[3 * f], V, s)) bad[t] = 1;
      steps[t] = std::max(steps[t], s);
    }
  };
  std::vector<std::thread> pool;
  for (int t = 1; t < n_threads; ++t) pool.emplace_back(work, t);
  work(0);
  for (auto& th : pool) th.join();
  for (int32_t v = 0; v < V; ++v) {
    if (parent[v] > v) {
      std::printf("%s: parent[%d] = %d breaks parent <= v\n", name, v, parent[v]);
      return false;
    }
  }
  for (int32_t v = 0; v < V; ++v) {
    uint32_t s = 0;
    const int32_t r = nerf_uf::find<false>(parent.data(), v, (uint32_t)V, s);
    if (r < 0) {
      std::printf("%s: flatten exhausted its bound at %d\n", name, v);
      return false;
    }
    nerf_uf::store(parent.data() + v, r);
  }
  const bool ok = parent == serial_labels(faces, V) && !*std::max_element(bad.begin(), bad.end());
  std::printf("%-28s V=%-6d F=%-6zu threads=%d max steps=%u %s\n", name, V, F, n_threads,
              *std::max_element(steps.begin(), steps.end()), ok ? "ok" : "MISMATCH");
  return ok;
}

std::vector<int32_t> strip(int n_faces, int numbering, uint32_t seed) {
  const int32_t V = n_faces + 2;
  std::vector<int32_t> map(V);
  std::iota(map.begin(), map.end(), 0);
  if (numbering == 1) std::reverse(map.begin(), map.end());
  if (numbering == 2) std::shuffle(map.begin(), map.end(), std::mt19937(seed));
  std::vector<int32_t> f;
  for (int i = 0; i < n_faces; ++i)
    for (int k = 0; k < 3; ++k) f.push_back(map[i + k]);
  return f;
}

}  // namespace

int main() {
  bool ok = true;
  const char* names[3] = {"identity", "reversed", "random"};
  for (int n : {1, 63, 64, 65, 255, 256, 257, 2049, 20000})
    for (int numbering = 0; numbering < 3; ++numbering)
      for (int threads : {1, 8}) {
        char name[64];
        std::snprintf(name, sizeof name, "strip%d-%s", n, names[numbering]);
        auto f = strip(n, numbering, (uint32_t)n);
        ok = run(name, f, n + 2, threads) && ok;
        if (n == 257) {  // every face twice, plus (a,a,b) and (a,a,a) faces
          auto g = f;
          g.insert(g.end(), f.rbegin(), f.rend());
          for (int i = 0; i < n; i += 7) {
            g.insert(g.end(), {f[3 * i], f[3 * i], f[3 * i + 2]});
            g.insert(g.end(), {f[3 * i + 1], f[3 * i + 1], f[3 * i + 1]});
          }
          ok = run("  + duplicated, degenerate", g, n + 2 + 3, threads) && ok;  // 3 unused vertices at the end
        }
      }
  // two interleaved strips (even / odd vertices): two components
  {
    std::vector<int32_t> f;
    for (int i = 0; i < 500; ++i)
      for (int par = 0; par < 2; ++par) f.insert(f.end(), {2 * i + par, 2 * i + 2 + par, 2 * i + 4 + par});
    for (int threads : {1, 8}) ok = run("interleaved", f, 1004, threads) && ok;
  }
  std::printf(ok ? "ok\n" : "FAILED\n");
  return ok ? 0 : 1;
}
