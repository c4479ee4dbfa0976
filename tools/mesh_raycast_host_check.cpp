// Host check of csrc/mesh_raycast_core.hpp: the face registration of mesh_distance_core.hpp, then the
// walk of every ray run serially, one loop iteration per thread exactly as the kernel calls it, against the test of
// every face in turn (t bits, face index, barycentric bits), on a random soup with faces without area, on a mesh
// with one tiny and one large face at 1024 cells per axis, on a closed sphere, and on a sliver that only the box
// clause of the hit test rejects.  The ray sets are those of tests/test_gpu_mesh_raycast.py: aimed and random rays,
// axis-parallel rays, rays along a cell plane, rays from inside, rays that pass beside the box, far origins, near set
// just past the first hit, both culling modes, three grids.  Stand-alone:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/mesh_raycast_host_check.cpp -o mesh_raycast_host_check && ./mesh_raycast_host_check
//
// Exit status 0 and "ok" when every case agrees.  It needs no GPU and loads nothing of the Python package.
// With an argument it also writes the vertices, faces and rays of the first soup case and t (hex float), face and
// (u, v) of every ray to that file, for a comparison with tests/mesh_raycast_reference.py.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../nerf-sys_amd/csrc/mesh_raycast_core.hpp"
#include "mesh_host_check_common.hpp"

namespace {

using namespace mesh_check;

template <class T>
bool same_bits(T a, T b) {
  return std::memcmp(&a, &b, sizeof a) == 0;
}

double margin_of(const std::vector<float>& p) {
  float m = 0.0f;
  for (float x : p) m = std::max(m, std::fabs(x));
  return ldexp((double)m, -30);
}

struct Tally {
  int64_t rays = 0, hits = 0, layers = 0, tested = 0;
};

// the walk of every ray against the test of every face; rays (n, 8)
bool check(const char* name, const Soup& s, const std::vector<float>& rays, float cell, bool cull, Tally* tally = nullptr,
           std::FILE* dump = nullptr) {
  Grid g;
  if (!make_grid(s.v, cell, g)) return std::printf("%s: the grid has more than 1024 cells\n", name), false;
  const int64_t F = (int64_t)s.f.size() / 3, n = (int64_t)rays.size() / 8;
  const double margin = margin_of(s.v);
  if (!(margin <= 0.0009765625 * (double)cell)) return std::printf("%s: the cell is below 2^-20 Cmax\n", name), false;
  const std::vector<int64_t> keys = sorted_keys(g, s);
  const int64_t n_keys = (int64_t)keys.size();
  if (n_keys >= (int64_t(1) << 31)) return std::printf("%s: too many keys\n", name), false;
  for (int64_t i = 0; i < n; ++i) {
    const nerf_mr::Ray r = nerf_mr::load_ray(rays.data(), i);
    int64_t counts[2];
    const nerf_mr::Hit got = nerf_mr::cast(g, r, keys.data(), n_keys, s.v.data(), s.f.data(), F, margin, cull, counts);
    const nerf_mr::Hit want = nerf_mr::brute(r, s.v.data(), s.f.data(), F, margin, cull);
    if ((want.face < 0) != !(want.t < (double)INFINITY) || (want.face < 0 && (want.u != 0.0f || want.v != 0.0f)))
      return std::printf("%s: ray %lld: brute force (%a, %d)\n", name, (long long)i, want.t, want.face), false;
    if (!same_bits(got.t, want.t) || got.face != want.face || !same_bits(got.u, want.u) || !same_bits(got.v, want.v)) {
      std::printf("%s: ray %lld: got (%a, %d, %a, %a), brute force (%a, %d, %a, %a)\n", name, (long long)i, got.t,
                  got.face, got.u, got.v, want.t, want.face, want.u, want.v);
      return false;
    }
    const int32_t dim_max = std::max(g.dims[0], std::max(g.dims[1], g.dims[2]));
    if (counts[0] < 0 || counts[0] > dim_max) return std::printf("%s: ray %lld: %lld layers\n", name, (long long)i,
                                                                 (long long)counts[0]), false;
    if (tally) tally->rays += 1, tally->hits += got.face >= 0, tally->layers += counts[0], tally->tested += counts[1];
    if (dump) std::fprintf(dump, "%a %d %a %a\n", got.t, got.face, got.u, got.v);
  }
  return true;
}

// ---------------------------------------------------------------- rays

void push_ray(std::vector<float>& rays, const double o[3], const double d[3], float near = 0.0f, float far = INFINITY) {
  for (int k = 0; k < 3; ++k) rays.push_back((float)o[k]);
  for (int k = 0; k < 3; ++k) rays.push_back((float)d[k]);
  rays.push_back(near);
  rays.push_back(far);
}

// a random point of a random face with area
void face_point(std::mt19937& rng, const Soup& s, double p[3]) {
  std::uniform_int_distribution<int64_t> pick(0, (int64_t)s.f.size() / 3 - 1);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  for (;;) {
    const int64_t f = pick(rng);
    if (!(nerf_mm::face_area(s.v.data(), s.f.data(), f) > 0.0)) continue;
    double a = u(rng), b = u(rng);
    if (a + b > 1.0) a = 1.0 - a, b = 1.0 - b;
    for (int k = 0; k < 3; ++k)
      p[k] = (1.0 - a - b) * s.v[3 * s.f[3 * f] + k] + a * s.v[3 * s.f[3 * f + 1] + k] + b * s.v[3 * s.f[3 * f + 2] + k];
    return;
  }
}

void set_length(std::mt19937& rng, double d[3]) {
  std::uniform_real_distribution<double> len(0.5, 2.0);
  const double n = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]), l = len(rng);
  for (int k = 0; k < 3; ++k) d[k] = n > 0 ? d[k] / n * l : (k == 0 ? l : 0.0);
}

// origins in the box widened by ``pad`` extents (pad < 0: ``-pad`` extents from the centre, all aimed); every
// second ray aimed at a face point, the others with a normal-distributed direction
std::vector<float> mixed_rays(std::mt19937& rng, const Soup& s, int64_t n, double pad) {
  const Box b = box_of(s.v);
  std::normal_distribution<double> g(0.0, 1.0);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  std::vector<float> rays;
  for (int64_t i = 0; i < n; ++i) {
    double o[3], d[3], p[3];
    if (pad >= 0) {
      for (int k = 0; k < 3; ++k) o[k] = b.lo[k] - pad * b.ext + u(rng) * (b.hi[k] - b.lo[k] + 2 * pad * b.ext);
    } else {
      double dir[3] = {g(rng), g(rng), g(rng)};
      const double len = std::sqrt(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]), far = 5 + 45 * u(rng);
      for (int k = 0; k < 3; ++k) o[k] = 0.5 * (b.lo[k] + b.hi[k]) + dir[k] / len * far * b.ext;
    }
    if (pad < 0 || i % 2 == 0) {
      face_point(rng, s, p);
      for (int k = 0; k < 3; ++k) d[k] = p[k] - o[k];
    } else {
      for (int k = 0; k < 3; ++k) d[k] = g(rng);
    }
    set_length(rng, d);
    push_ray(rays, o, d);
  }
  return rays;
}

// two exact zeros in d, both signs: a face point displaced along an axis (``only_axis`` >= 0 fixes it)
std::vector<float> axis_rays(std::mt19937& rng, const Soup& s, int64_t n, int only_axis = -1) {
  const Box b = box_of(s.v);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  std::vector<float> rays;
  for (int64_t i = 0; i < n; ++i) {
    double o[3], d[3] = {0, 0, 0};
    face_point(rng, s, o);
    for (int k = 0; k < 3; ++k) o[k] = (double)(float)o[k];
    const int axis = only_axis >= 0 ? only_axis : (int)(i % 3);
    const double sign = (i / 3) % 2 ? 1.0 : -1.0;
    d[axis] = sign * (0.5 + 1.5 * u(rng));
    o[axis] -= sign * (0.1 + 1.4 * u(rng)) * b.ext;
    push_ray(rays, o, d);
  }
  return rays;
}

// the origin exactly on a cell plane lo + k cell, the ray running along it
std::vector<float> plane_rays(std::mt19937& rng, const Soup& s, float cell, int64_t n) {
  Grid g;
  std::vector<float> rays;
  if (!make_grid(s.v, cell, g)) return rays;
  const Box b = box_of(s.v);
  std::normal_distribution<double> nd(0.0, 1.0);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  for (int64_t i = 0; i < n; ++i) {
    double o[3], d[3] = {nd(rng), nd(rng), nd(rng)};
    for (int k = 0; k < 3; ++k) o[k] = b.lo[k] - 0.25 * b.ext + u(rng) * (b.hi[k] - b.lo[k] + 0.5 * b.ext);
    const int axis = (int)(i % 3);
    const int32_t plane = (int32_t)(u(rng) * (g.dims[axis] + 1));
    o[axis] = (double)(g.lo[axis] + (float)plane * g.cell);
    d[axis] = 0.0;
    set_length(rng, d);
    d[axis] = 0.0;
    push_ray(rays, o, d);
  }
  return rays;
}

// beside the box: the origin beyond one of its faces, the direction pointing farther away
std::vector<float> outside_rays(std::mt19937& rng, const Soup& s, int64_t n) {
  const Box b = box_of(s.v);
  std::normal_distribution<double> nd(0.0, 1.0);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  std::vector<float> rays;
  for (int64_t i = 0; i < n; ++i) {
    double o[3], d[3] = {nd(rng), nd(rng), nd(rng)};
    for (int k = 0; k < 3; ++k) o[k] = b.lo[k] - b.ext + u(rng) * (b.hi[k] - b.lo[k] + 2 * b.ext);
    const int axis = (int)(i % 3);
    const bool up = (i / 3) % 2;
    o[axis] = up ? b.hi[axis] + (0.05 + 2 * u(rng)) * b.ext : b.lo[axis] - (0.05 + 2 * u(rng)) * b.ext;
    d[axis] = up ? std::fabs(d[axis]) : -std::fabs(d[axis]);
    set_length(rng, d);
    push_ray(rays, o, d);
  }
  return rays;
}

// near just past the first hit (brute force's t, rounded up to fp32 and one step on): the next face is returned
std::vector<float> second_hit_rays(const Soup& s, std::vector<float> rays) {
  const double margin = margin_of(s.v);
  for (size_t i = 0; i < rays.size() / 8; ++i) {
    const nerf_mr::Hit h = nerf_mr::brute(nerf_mr::load_ray(rays.data(), (int64_t)i), s.v.data(), s.f.data(),
                                          (int64_t)s.f.size() / 3, margin, false);
    if (h.face < 0) continue;
    float near = (float)h.t;
    if ((double)near <= h.t) near = nextafterf(near, INFINITY);
    rays[8 * i + 6] = near;
  }
  return rays;
}

bool all_sets(const char* name, std::mt19937& rng, const Soup& s, const float cells[3], int axis = -1) {
  bool ok = true;
  const std::vector<float> mixed = mixed_rays(rng, s, 1000, 0.5);
  const std::vector<float> sets[6] = {mixed, axis_rays(rng, s, 300, axis), mixed_rays(rng, s, 300, 0.0),
                                      outside_rays(rng, s, 200), mixed_rays(rng, s, 100, -1.0), second_hit_rays(s, mixed)};
  const char* kinds[7] = {"mixed", "axis", "inside", "outside", "far", "second", "plane"};
  for (int c = 0; c < 3; ++c)
    for (int cull = 0; cull < 2; ++cull) {
      for (int k = 0; k < 7; ++k) {
        Tally tally;
        char label[96];
        std::snprintf(label, sizeof label, "%s/%s/cell %g/cull %d", name, kinds[k], cells[c], cull);
        ok &= check(label, s, k < 6 ? sets[k] : plane_rays(rng, s, cells[c], 200), cells[c], cull != 0, &tally);
        if (cull == 0 && tally.rays)
          std::printf("%-44s hits %5.1f %%  layers %7.1f  faces tested %8.1f per ray\n", label,
                      100.0 * tally.hits / tally.rays, (double)tally.layers / tally.rays,
                      (double)tally.tested / tally.rays);
        if (k == 3 && tally.hits) ok = false, std::printf("%s: a ray beside the box hit\n", label);
      }
    }
  return ok;
}

}  // namespace

int main(int argc, char** argv) {
  std::mt19937 rng(7);
  bool ok = true;
  // the table of the issue on one triangle: {o, d, near, far}, cull, hit, t, u, v
  {
    const Soup one{{0, 0, 0, 1, 0, 0, 0, 1, 0}, {0, 1, 2}};
    const float inf = INFINITY;
    struct Row {
      float ray[8];
      bool cull, hit;
      double t;
      float u, v;
    };
    const Row rows[] = {{{.25f, .5f, 1, 0, 0, -1, 0, inf}, false, true, 1, .25f, .5f},
                        {{.25f, .5f, 2, 0, 0, -4, 0, inf}, true, true, .5, .25f, .5f},
                        {{.25f, .5f, -1, 0, 0, 1, 0, inf}, false, true, 1, .25f, .5f},
                        {{.25f, .5f, -1, 0, 0, 1, 0, inf}, true, false, 0, 0, 0},
                        {{.5f, 0, 1, 0, 0, -1, 0, inf}, false, true, 1, .5f, 0},
                        {{.5f, .5f, 1, 0, 0, -1, 0, inf}, false, true, 1, .5f, .5f},
                        {{1, 0, 1, 0, 0, -1, 0, inf}, false, true, 1, 1, 0},
                        {{.5f, -0x1p-20f, 1, 0, 0, -1, 0, inf}, false, false, 0, 0, 0},
                        {{-1, .25f, 1, 1, 0, 0, 0, inf}, false, false, 0, 0, 0},
                        {{-1, .25f, 0, 1, 0, 0, 0, inf}, false, false, 0, 0, 0},
                        {{.25f, .5f, 1, 0, 0, 1, 0, inf}, false, false, 0, 0, 0},
                        {{.25f, .5f, 1, 0, 0, -1, 1.5f, inf}, false, false, 0, 0, 0},
                        {{.25f, .5f, 1, 0, 0, -1, 0, .5f}, false, false, 0, 0, 0},
                        {{.25f, .5f, 1, 0, 0, -1, 2, .5f}, false, false, 0, 0, 0},
                        {{.25f, .5f, 1, 0, 0, -1, 1, 1}, false, true, 1, .25f, .5f}};
    int i = 0;
    for (const Row& row : rows) {
      const nerf_mr::Hit h = nerf_mr::brute(nerf_mr::load_ray(row.ray, 0), one.v.data(), one.f.data(), 1, 0x1p-30, row.cull);
      if ((h.face == 0) != row.hit || (row.hit && (h.t != row.t || h.u != row.u || h.v != row.v)) ||
          (!row.hit && (h.face != -1 || h.t != (double)INFINITY)))
        ok = false, std::printf("table row %d: (%a, %d, %a, %a)\n", i, h.t, h.face, h.u, h.v);
      ok &= check("table", one, std::vector<float>(row.ray, row.ray + 8), 0.25f, row.cull);
      ++i;
    }
  }
  // a random soup with faces without area: one cell, a coarse grid, 32 cells per axis
  {
    const Soup s = soup(rng, 40, 60);
    std::FILE* dump = argc > 1 ? std::fopen(argv[1], "w") : nullptr;
    if (dump) {
      const std::vector<float> rays = mixed_rays(rng, s, 500, 0.5);
      for (float x : s.v) std::fprintf(dump, "v %a\n", x);
      for (int32_t x : s.f) std::fprintf(dump, "f %d\n", x);
      for (float x : rays) std::fprintf(dump, "r %a\n", x);
      ok &= check("soup_dump", s, rays, 0.5f, false, nullptr, dump);
      std::fclose(dump);
    }
    const float cells[3] = {4.0f, 0.5f, 2.0f / 31.5f};
    ok &= all_sets("soup", rng, s, cells);
    Soup none;  // no face at all
    none.v = s.v;
    ok &= check("no_faces", none, mixed_rays(rng, s, 50, 0.5), 0.5f, false);
  }
  // one tiny and one large face, up to 1024 cells per axis
  {
    const Soup s{{0, 0, 0, 1, 0, 0, 0, 1, 0, 2, 2, 2, 2 + 0x1p-17f, 2, 2, 2, 2 + 0x1p-17f, 2}, {3, 4, 5, 0, 1, 2}};
    const float cells[3] = {5.0f, 2.0f, (2.0f + 0x1p-17f) / 1023.5f};
    ok &= all_sets("tiny_face", rng, s, cells, 2);
  }
  // a closed sphere wound outwards: the first hit from outside is a front hit
  {
    const float centre[3] = {0.3f, -0.2f, 1.1f};
    const Soup s = sphere(16, 24, 0.8f, centre);
    const float cells[3] = {4.0f, 0.2f, 1.6f / 31.5f};
    ok &= all_sets("sphere", rng, s, cells);
    const std::vector<float> far = mixed_rays(rng, s, 200, -1.0);
    const double margin = margin_of(s.v);
    size_t hits = 0;  // a ray aimed at a point on the silhouette may pass it by the rounding of its direction
    for (size_t i = 0; i < far.size() / 8; ++i) {
      const nerf_mr::Ray r = nerf_mr::load_ray(far.data(), (int64_t)i);
      const nerf_mr::Hit a = nerf_mr::brute(r, s.v.data(), s.f.data(), (int64_t)s.f.size() / 3, margin, false);
      const nerf_mr::Hit b = nerf_mr::brute(r, s.v.data(), s.f.data(), (int64_t)s.f.size() / 3, margin, true);
      if (a.face != b.face || !same_bits(a.t, b.t)) ok = false, std::printf("sphere: ray %zu: culling\n", i);
      hits += a.face >= 0;
    }
    if (10 * hits < 9 * (far.size() / 8)) ok = false, std::printf("sphere: %zu of the aimed rays hit\n", hits);
  }
  // the sliver of tests/mesh_raycast_reference.py: a hit without the box clause, a miss with it
  {
    const Soup s{{0, 0, 0, 1, 0, 0, 2, 0, 0x1p-100f}, {0, 1, 2}};
    const float ray[8] = {100, 1, 1, 0, -1, -1, 0, INFINITY};
    const nerf_mr::Ray r = nerf_mr::load_ray(ray, 0);
    const nerf_mr::Hit loose = nerf_mr::brute(r, s.v.data(), s.f.data(), 1, (double)INFINITY, false);
    const nerf_mr::Hit strict = nerf_mr::brute(r, s.v.data(), s.f.data(), 1, margin_of(s.v), false);
    if (loose.face != 0 || loose.t != 1.0 || strict.face != -1) ok = false, std::printf("sliver: %d %a %d\n", loose.face, loose.t, strict.face);
    ok &= check("sliver", s, std::vector<float>(ray, ray + 8), 0.25f, false);
  }
  // an origin more than 2^32 cells away: every face is tested
  {
    const Soup s = soup(rng, 40, 60);
    std::vector<float> rays = mixed_rays(rng, s, 200, -1.0);
    for (size_t i = 0; i < rays.size() / 8; ++i)
      for (int k = 0; k < 3; ++k) rays[8 * i + k] = rays[8 * i + k] * 0x1p30f;  // 2^35 cells of 2^-5
    Tally tally;
    ok &= check("far_origin", s, rays, 0.03125f, false, &tally);
    if (tally.tested != tally.rays * 60) ok = false, std::printf("far_origin: %lld faces tested\n", (long long)tally.tested);
  }
  std::printf(ok ? "ok\n" : "FAILED\n");
  return ok ? 0 : 1;
}
