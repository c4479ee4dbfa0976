// What the host checks of the face-grid queries share (mesh_distance_host_check.cpp, mesh_raycast_host_check.cpp,
// mesh_inside_host_check.cpp): the two mesh generators, the grid of kernels.mesh_face_grid and the sorted face keys.
// Header only; every program that includes it stays stand-alone.
#pragma once
#include <algorithm>
#include <cmath>
#include <random>
#include <vector>

#include "../nerf-sys_amd/csrc/mesh_distance_core.hpp"

namespace mesh_check {

using nerf_grid::Grid;

struct Soup {
  std::vector<float> v;
  std::vector<int32_t> f;
};

struct Box {
  float lo[3], hi[3], ext;
};

inline Box box_of(const std::vector<float>& p) {
  Box b;
  for (int c = 0; c < 3; ++c) {
    b.lo[c] = b.hi[c] = p[c];
    for (size_t j = 0; j < p.size() / 3; ++j) {
      b.lo[c] = std::min(b.lo[c], p[3 * j + c]);
      b.hi[c] = std::max(b.hi[c], p[3 * j + c]);
    }
  }
  b.ext = std::max(b.hi[0] - b.lo[0], std::max(b.hi[1] - b.lo[1], b.hi[2] - b.lo[2]));
  return b;
}

// the grid of kernels.mesh_face_grid: lo = the minimum of the vertices, dims = floor((max - lo) * inv) + 1 in fp32
inline bool make_grid(const std::vector<float>& p, float cell, Grid& g) {
  const Box b = box_of(p);
  g.cell = cell;
  g.inv = 1.0f / cell;
  for (int c = 0; c < 3; ++c) {
    g.lo[c] = b.lo[c];
    const float cells = floorf((b.hi[c] - b.lo[c]) * g.inv);
    if (!(cells + 1.0f <= (float)nerf_grid::MAX_DIM)) return false;
    g.dims[c] = (int32_t)cells + 1;
  }
  return true;
}

// registration as the caller of the kernels does it: counts, an exclusive sum, the keys of every face, a sort
inline std::vector<int64_t> sorted_keys(const Grid& g, const Soup& s) {
  const int64_t F = (int64_t)s.f.size() / 3;
  std::vector<int64_t> offsets((size_t)F + 1, 0);
  for (int64_t f = 0; f < F; ++f) offsets[f + 1] = offsets[f] + nerf_grid::face_cell_count(g, s.v.data(), s.f.data(), f);
  std::vector<int64_t> keys((size_t)offsets[F], -1);
  for (int64_t f = 0; f < F; ++f) nerf_grid::face_keys(g, s.v.data(), s.f.data(), f, keys.data() + offsets[f]);
  std::sort(keys.begin(), keys.end());
  return keys;
}

inline std::vector<float> uniform(std::mt19937& rng, int64_t n, float a, float b) {
  std::uniform_real_distribution<float> u(a, b);
  std::vector<float> out((size_t)(3 * n));
  for (auto& x : out) x = u(rng);
  return out;
}

// a random soup with faces of a repeated index and exactly collinear corners
inline Soup soup(std::mt19937& rng, int64_t V, int64_t F) {
  Soup s;
  s.v = uniform(rng, V, -1, 1);
  const float line[9] = {0.25f, 0.5f, -0.5f, 0.5f, 0.5f, -0.5f, 1.0f, 0.5f, -0.5f};
  std::copy(line, line + 9, s.v.end() - 9);
  std::uniform_int_distribution<int32_t> vi(0, (int32_t)V - 4);
  for (int64_t i = 0; i < 3 * F; ++i) s.f.push_back(vi(rng));
  const int32_t dead[] = {3, 3, 9, 12, 7, 12, 20, 20, 20, (int32_t)V - 3, (int32_t)V - 2, (int32_t)V - 1,
                          (int32_t)V - 1, (int32_t)V - 3, (int32_t)V - 2};
  std::copy(dead, dead + 15, s.f.begin());
  return s;
}

// a latitude / longitude sphere, closed and wound outwards
inline Soup sphere(int rings, int segments, float radius, const float centre[3]) {
  Soup s;
  const double pi = 3.14159265358979323846;
  s.v = {centre[0], centre[1], centre[2] + radius};
  for (int i = 1; i < rings; ++i)
    for (int j = 0; j < segments; ++j) {
      const double th = pi * i / rings, ph = 2 * pi * j / segments;
      s.v.insert(s.v.end(), {centre[0] + radius * (float)(sin(th) * cos(ph)), centre[1] + radius * (float)(sin(th) * sin(ph)),
                             centre[2] + radius * (float)cos(th)});
    }
  s.v.insert(s.v.end(), {centre[0], centre[1], centre[2] - radius});
  const int32_t last = (int32_t)s.v.size() / 3 - 1;
  auto at = [&](int i, int j) { return 1 + (i - 1) * segments + j % segments; };
  for (int j = 0; j < segments; ++j) {
    s.f.insert(s.f.end(), {0, at(1, j), at(1, j + 1)});
    s.f.insert(s.f.end(), {last, at(rings - 1, j + 1), at(rings - 1, j)});
    for (int i = 1; i < rings - 1; ++i) {
      s.f.insert(s.f.end(), {at(i, j), at(i + 1, j), at(i + 1, j + 1)});
      s.f.insert(s.f.end(), {at(i, j), at(i + 1, j + 1), at(i, j + 1)});
    }
  }
  return s;
}

}  // namespace mesh_check
