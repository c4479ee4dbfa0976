// Host check of csrc/mesh_winding_core.hpp: the bricks built as the caller of the kernels builds
// them (the key of every face, a sort, the corner soup, the first position of every occupied brick, the moments of
// every brick, one loop iteration per thread exactly as the kernels call them), then the winding number of every query
// through the bricks, exact and with the far field at beta = 2, 3, 4, against a plain loop over the faces: on a
// closed sphere (1 inside, 0 outside), on the same sphere with its polar cap removed (the far field's error must fall
// as beta grows), on a random soup with faces without area, and on a mesh with one tiny and one large face at 1024
// bricks per axis; the octant triangle and the strict near / far compare at a brick of radius zero.  Stand-alone:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/mesh_winding_host_check.cpp -o mesh_winding_host_check && ./mesh_winding_host_check
//
// Exit status 0 and "ok" when every case agrees.  It needs no GPU and loads nothing of the Python package.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "../nerf-sys_amd/csrc/mesh_winding_core.hpp"
#include "mesh_host_check_common.hpp"

namespace {

using namespace mesh_check;

struct Bricks {
  std::vector<int64_t> keys, starts;
  std::vector<float> soup;
  std::vector<int32_t> runs;
  std::vector<double> moments;
  int64_t B = 0, F = 0;
};

bool build(const char* name, const Soup& s, float cell, Bricks& br) {
  Grid g;
  if (!make_grid(s.v, cell, g)) return std::printf("%s: the grid has more than 1024 cells\n", name), false;
  const int64_t F = (int64_t)s.f.size() / 3;
  br = Bricks();
  br.F = F;
  br.keys.resize((size_t)F);
  for (int64_t f = 0; f < F; ++f) br.keys[f] = nerf_mw::face_brick_key(g, s.v.data(), s.f.data(), f);
  std::sort(br.keys.begin(), br.keys.end());
  br.soup.assign((size_t)(nerf_mw::SOUP * F), -1.0f);
  for (int64_t j = 0; j < F; ++j) nerf_mw::write_soup(s.v.data(), s.f.data(), br.keys.data(), j, br.soup.data());
  for (int64_t j = 0; j < F; ++j)
    if (j == 0 || nerf_grid::key_cell(br.keys[j]) != nerf_grid::key_cell(br.keys[j - 1])) br.starts.push_back(j);
  br.B = (int64_t)br.starts.size();
  br.runs.assign((size_t)(nerf_mw::RUN * br.B), -1);
  br.moments.assign((size_t)(nerf_mw::MOMENTS * br.B), -1.0);
  for (int64_t b = 0; b < br.B; ++b)
    nerf_mw::brick_moments(br.soup.data(), F, br.starts.data(), br.B, b, br.runs.data() + nerf_mw::RUN * b,
                           br.moments.data() + nerf_mw::MOMENTS * b);
  // the runs partition [0, F), every face occurs once, r2 covers every corner of the run
  std::vector<char> seen((size_t)F, 0);
  for (int64_t j = 0; j < F; ++j) {
    const int64_t f = (int64_t)(uint32_t)nerf_grid::key_item(br.keys[j]);
    if (f >= F || seen[f]) return std::printf("%s: face %lld twice or out of range\n", name, (long long)f), false;
    seen[f] = 1;
  }
  int64_t at = 0;
  for (int64_t b = 0; b < br.B; ++b) {
    if (br.runs[2 * b] != at || br.runs[2 * b + 1] <= at) return std::printf("%s: run %lld\n", name, (long long)b), false;
    at = br.runs[2 * b + 1];
    const double* rec = br.moments.data() + nerf_mw::MOMENTS * b;
    for (int k = 0; k < nerf_mw::MOMENTS; ++k)
      if (!std::isfinite(rec[k])) return std::printf("%s: brick %lld is not finite\n", name, (long long)b), false;
    for (int64_t j = br.runs[2 * b]; j < at; ++j)
      for (int v = 0; v < 3; ++v) {
        double d2 = 0;
        for (int k = 0; k < 3; ++k) d2 += ((double)br.soup[9 * j + 3 * v + k] - rec[k]) * ((double)br.soup[9 * j + 3 * v + k] - rec[k]);
        if (d2 > rec[6] * (1 + 1e-12)) return std::printf("%s: a corner outside r of brick %lld\n", name, (long long)b), false;
      }
  }
  return at == F || (F == 0 && br.B == 0) || (std::printf("%s: the runs end at %lld\n", name, (long long)at), false);
}

// the definition: every face in its own order
double plain(const Soup& s, const float q32[3]) {
  const double q[3] = {q32[0], q32[1], q32[2]};
  double acc = 0.0;
  for (size_t f = 0; f < s.f.size() / 3; ++f) {
    float t[9];
    for (int v = 0; v < 3; ++v)
      for (int k = 0; k < 3; ++k) t[3 * v + k] = s.v[3 * s.f[3 * f + v] + k];
    acc += nerf_mw::solid_angle(t, q);
  }
  return acc / nerf_mw::FOUR_PI;
}

struct Errors {
  double exact = 0, far[3] = {0, 0, 0}, far_bricks[3] = {0, 0, 0}, near_faces[3] = {0, 0, 0};
  int64_t n = 0;
};

// every query: exact through the bricks against the plain loop, and the far field at beta = 2, 3, 4 against exact
bool check(const char* name, const Soup& s, float cell, const std::vector<float>& query, Errors& err) {
  Bricks br;
  if (!build(name, s, cell, br)) return false;
  const double betas[3] = {2.0, 3.0, 4.0};
  err = Errors();
  err.n = (int64_t)query.size() / 3;
  for (int64_t i = 0; i < err.n; ++i) {
    const float* q = query.data() + 3 * i;
    int64_t counts[2];
    const double exact = nerf_mw::winding(q, br.runs.data(), br.moments.data(), br.B, br.soup.data(), 9.0, true, counts);
    if (counts[0] != 0 || counts[1] != br.F) return std::printf("%s: exact summed %lld faces\n", name, (long long)counts[1]), false;
    const double want = plain(s, q);
    if (!std::isfinite(exact)) return std::printf("%s: query %lld is not finite\n", name, (long long)i), false;
    err.exact = std::max(err.exact, std::fabs(exact - want));
    double last_far = (double)br.B + 1;
    for (int k = 0; k < 3; ++k) {
      const double w = nerf_mw::winding(q, br.runs.data(), br.moments.data(), br.B, br.soup.data(), betas[k] * betas[k], false, counts);
      if (!std::isfinite(w) || counts[0] > br.B || counts[1] > br.F || (double)counts[0] > last_far)
        return std::printf("%s: query %lld, beta %g: %lld far bricks, %lld faces\n", name, (long long)i, betas[k], (long long)counts[0], (long long)counts[1]), false;
      last_far = (double)counts[0];
      err.far[k] = std::max(err.far[k], std::fabs(w - exact));
      err.far_bricks[k] += (double)counts[0] / err.n, err.near_faces[k] += (double)counts[1] / err.n;
    }
  }
  std::printf("%-26s B %5lld F %5lld  exact - plain %.2e  far field max error", name, (long long)br.B, (long long)br.F, err.exact);
  for (int k = 0; k < 3; ++k) std::printf("  b%g %.2e (%.0f far, %.0f faces)", betas[k], err.far[k], err.far_bricks[k], err.near_faces[k]);
  std::printf("\n");
  // a different order of the same terms: F roundings of a sum of magnitude <= 4 pi F, far inside F 2^-50 after / 4 pi
  if (err.exact > (double)(br.F + 1) * 0x1p-50) return std::printf("%s: exact differs from the plain loop\n", name), false;
  return true;
}

std::vector<float> box_queries(std::mt19937& rng, const Soup& s, int64_t n, float pad) {
  const Box b = box_of(s.v);
  std::uniform_real_distribution<float> u(0.0f, 1.0f);
  std::vector<float> q;
  for (int64_t i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) q.push_back(b.lo[k] - pad * b.ext + u(rng) * (b.hi[k] - b.lo[k] + 2 * pad * b.ext));
  return q;
}

}  // namespace

int main() {
  std::mt19937 rng(11);
  bool ok = true;
  Errors err;
  // the octant triangle from the origin, both windings; and a brick of radius zero at the query itself
  {
    const Soup one{{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 1, 2}}, flipped{{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 2, 1}};
    const float origin[3] = {0, 0, 0};
    if (std::fabs(plain(one, origin) - 0.125) > 0x1p-50 || std::fabs(plain(flipped, origin) + 0.125) > 0x1p-50)
      ok = false, std::printf("octant: %a and %a\n", plain(one, origin), plain(flipped, origin));
    const Soup point{{0, 0, 0, 1, 0, 0, 0, 1, 0, 5, 5, 5}, {0, 1, 2, 3, 3, 3}};
    Bricks br;
    ok &= build("point", point, 1.0f, br);
    const float at[3] = {5, 5, 5};
    int64_t counts[2];
    const double w = nerf_mw::winding(at, br.runs.data(), br.moments.data(), br.B, br.soup.data(), 1.0, false, counts);
    if (br.B != 2 || br.moments[13] != 0.0 || br.moments[7] != 5.0 || !std::isfinite(w) || counts[0] != 1 || counts[1] != 1)
      ok = false, std::printf("point: B %lld, r2 %g, w %g, %lld far, %lld faces\n", (long long)br.B, br.moments[13], w, (long long)counts[0], (long long)counts[1]);
  }
  // a closed sphere wound outwards: 1 inside, 0 outside, through one brick, a coarse and a fine grid
  const float centre[3] = {0.3f, -0.2f, 1.1f};
  const Soup ball = sphere(16, 24, 0.8f, centre);
  {
    const std::vector<float> q = box_queries(rng, ball, 600, 0.25f);
    for (float cell : {4.0f, 0.3f, 1.6f / 63.5f}) {
      char label[64];
      std::snprintf(label, sizeof label, "sphere/cell %g", cell);
      ok &= check(label, ball, cell, q, err);
      if (!(err.far[1] < 0.05)) ok = false, std::printf("%s: beta 3 is off by %g\n", label, err.far[1]);
    }
    int64_t judged = 0;
    for (size_t i = 0; i < q.size() / 3; ++i) {
      const double d[3] = {q[3 * i] - (double)centre[0], q[3 * i + 1] - (double)centre[1], q[3 * i + 2] - (double)centre[2]};
      const double r = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
      if (std::fabs(r - 0.8) < 0.05) continue;  // the polyhedron lies within 0.016 of the sphere
      ++judged;
      const double w = plain(ball, q.data() + 3 * i);
      if (std::fabs(w - (r < 0.8 ? 1.0 : 0.0)) > 720 * 0x1p-50) ok = false, std::printf("sphere: query %zu at r = %g: w = %.17g\n", i, r, w);
    }
    if (4 * judged < 3 * (int64_t)(q.size() / 3)) ok = false, std::printf("sphere: only %lld queries judged\n", (long long)judged);
  }
  // the same sphere without the faces at its upper pole: open; the far field's error falls as beta grows
  {
    Soup open = ball;
    open.f.clear();
    for (size_t f = 0; f < ball.f.size() / 3; ++f) {
      bool cap = false;
      for (int v = 0; v < 3; ++v) cap |= ball.f[3 * f + v] <= 2 * 24;  // the pole and the first two rings
      if (!cap) open.f.insert(open.f.end(), ball.f.begin() + 3 * f, ball.f.begin() + 3 * f + 3);
    }
    const std::vector<float> q = box_queries(rng, open, 600, 0.25f);
    ok &= check("open sphere/cell 0.25", open, 0.25f, q, err);
    if (!(err.far[0] > err.far[1] && err.far[1] > err.far[2] && err.far[0] < 0.05 && err.far[2] > 0))
      ok = false, std::printf("open sphere: the error does not fall with beta: %g %g %g\n", err.far[0], err.far[1], err.far[2]);
    const float inside[3] = {centre[0], centre[1], centre[2] - 0.4f}, outside[3] = {centre[0], centre[1], centre[2] + 3.0f};
    if (!(plain(open, inside) > 0.8 && plain(open, outside) < 0.2 && plain(open, outside) > -0.2))
      ok = false, std::printf("open sphere: %g inside, %g outside\n", plain(open, inside), plain(open, outside));
  }
  // a random soup with faces without area (bricks whose dipole is zero, faces whose corners coincide)
  {
    const Soup s = soup(rng, 40, 60);
    for (float cell : {4.0f, 0.5f, 2.0f / 31.5f}) ok &= check("soup", s, cell, box_queries(rng, s, 500, 0.1f), err);
    Soup none;
    none.v = s.v;
    ok &= check("no_faces", none, 0.5f, box_queries(rng, s, 20, 0.1f), err);
  }
  // one tiny and one large face, up to 1024 bricks per axis, queries far outside the grid as well
  {
    const Soup s{{0, 0, 0, 1, 0, 0, 0, 1, 0, 2, 2, 2, 2 + 0x1p-17f, 2, 2, 2, 2 + 0x1p-17f, 2}, {3, 4, 5, 0, 1, 2}};
    std::vector<float> q = box_queries(rng, s, 500, 0.1f);
    for (float x : {-1e6f, 0.25f, 1e6f})
      for (float z : {-1e6f, 1e6f}) q.insert(q.end(), {x, 0.25f, z});
    for (float cell : {5.0f, 2.0f, (2.0f + 0x1p-17f) / 1023.5f}) ok &= check("tiny_face", s, cell, q, err);
  }
  std::printf(ok ? "ok\n" : "FAILED\n");
  return ok ? 0 : 1;
}
