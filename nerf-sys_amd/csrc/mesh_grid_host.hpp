// The checks that the mesh entry points share (host side only): the size limit, the alignment of 64-bit arrays and
// the grid arguments lo, cell, inv, dims of include/nerf_amd.h.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mesh_grid_core.hpp"

namespace nerf_grid {

constexpr int64_t LIMIT = int64_t(1) << 31;

inline bool aligned8(const void* p) { return (((uintptr_t)p) & 7u) == 0; }

// the arguments as they stand, unchecked
inline Grid fill_grid(const float* lo, float cell, float inv, const int32_t* dims) {
  Grid g;
  for (int c = 0; c < 3; ++c) g.lo[c] = lo[c], g.dims[c] = dims[c];
  g.cell = cell;
  g.inv = inv;
  return g;
}

// lo, cell, inv, dims as the header states them; false on a value outside the contract
inline bool make_grid(const float* lo, float cell, float inv, const int32_t* dims, Grid& g) {
  if (!lo || !dims) return false;
  if (!(cell > 0.0f) || !(inv > 0.0f) || !isfinite(cell) || !isfinite(inv)) return false;
  for (int c = 0; c < 3; ++c)
    if (!isfinite(lo[c]) || dims[c] < 1 || dims[c] > MAX_DIM) return false;
  g = fill_grid(lo, cell, inv, dims);
  return true;
}

}  // namespace nerf_grid
