// Host check of the traversal of csrc/mesh_grid_core.hpp, which the queries' own checks see only through their
// results: walk_shells with a stop predicate that never fires must hand the scanner every cell of the grid exactly
// once, the cells before shell r being exactly the clipped cube of Chebyshev radius r - 1 around the query's clamped
// cell; for_run over one key per cell must visit exactly the keys of (ix, iy, z0 .. z1), in order, and nothing of an
// empty array.  Grids of 1 x 1 x 1, 1 x 3 x 5 and 4 x 4 x 4 cells, queries in every cell and outside every face of the
// box: the smallest shapes where the clipping, the rim / cap split and the early exit can go wrong.
// Stand-alone:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/mesh_grid_host_check.cpp -o mesh_grid_host_check && ./mesh_grid_host_check
//
// Exit status 0 and "ok" when every case agrees.  It needs no GPU and loads nothing of the Python package.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../nerf-sys_amd/csrc/mesh_grid_core.hpp"

namespace {

using nerf_grid::Grid;

int32_t cheb(const int32_t a[3], int32_t ix, int32_t iy, int32_t iz) {
  return std::max(std::abs(ix - a[0]), std::max(std::abs(iy - a[1]), std::abs(iz - a[2])));
}

// the cells of the grid within Chebyshev radius r of cell a
int64_t cube_cells(const Grid& g, const int32_t a[3], int32_t r) {
  int64_t n = 1;
  for (int c = 0; c < 3; ++c) n *= std::min(a[c] + r, g.dims[c] - 1) - std::max(a[c] - r, 0) + 1;
  return n;
}

// q lies in cell a (or is clamped into it)
bool check_shells(const Grid& g, const float q[3], const int32_t a[3]) {
  const int64_t cells = (int64_t)g.dims[0] * g.dims[1] * g.dims[2];
  std::vector<int> seen((size_t)cells, 0);
  int64_t handed = 0;
  int32_t shell = 0;  // the largest radius handed over so far: it must never decrease
  bool ok = true;
  auto fail = [&](const char* what) {
    if (ok) std::printf("dims %d %d %d, query %g %g %g: %s\n", g.dims[0], g.dims[1], g.dims[2], q[0], q[1], q[2], what);
    ok = false;
  };
  for (int c = 0; c < 3; ++c)
    if (nerf_grid::cell_index(g, c, q[c]) != a[c]) fail("the query's cell");
  nerf_grid::walk_shells(
      g, q,
      [&](int32_t r) {
        if (r < 2) fail("stop asked before shell 2");
        if (handed != cube_cells(g, a, r - 1)) fail("the cells before a shell are not the clipped cube");
        return false;
      },
      [&](int32_t ix, int32_t iy, int32_t z0, int32_t z1) {
        if (ix < 0 || ix >= g.dims[0] || iy < 0 || iy >= g.dims[1] || z0 < 0 || z1 >= g.dims[2] || z0 > z1)
          return fail("a run outside the grid");
        for (int32_t iz = z0; iz <= z1; ++iz) {
          const int32_t r = cheb(a, ix, iy, iz);
          if (r < shell) fail("a cell of an earlier shell after a later one");
          if (r > shell && handed != cube_cells(g, a, r - 1)) fail("a shell begun before the cube inside it was done");
          shell = std::max(shell, r);
          if (seen[(size_t)nerf_grid::cell_id(g, ix, iy, iz)]++) fail("a cell handed over twice");
          ++handed;
        }
      });
  if (handed != cells) fail("not every cell was handed over");
  return ok;
}

bool check_runs(const Grid& g) {
  const int64_t cells = (int64_t)g.dims[0] * g.dims[1] * g.dims[2];
  std::vector<int64_t> keys;  // one key per cell; the item tells the cell apart from its neighbours
  for (int64_t id = 0; id < cells; ++id) keys.push_back(nerf_grid::make_key(id, (uint32_t)(7 * id + 3)));
  for (int32_t ix = 0; ix < g.dims[0]; ++ix)
    for (int32_t iy = 0; iy < g.dims[1]; ++iy)
      for (int32_t z0 = 0; z0 < g.dims[2]; ++z0)
        for (int32_t z1 = z0; z1 < g.dims[2]; ++z1) {
          std::vector<int64_t> got, want;
          bool ok = true;
          nerf_grid::for_run(g, keys.data(), cells, ix, iy, z0, z1, [&](int64_t j, int64_t cell, int32_t item) {
            ok &= j >= 0 && j < cells && keys[(size_t)j] == nerf_grid::make_key(cell, (uint32_t)item);
            got.push_back(j);
          });
          for (int32_t iz = z0; iz <= z1; ++iz) want.push_back(nerf_grid::cell_id(g, ix, iy, iz));  // position == cell_id
          if (!ok || got != want)
            return std::printf("dims %d %d %d: the run (%d, %d, %d .. %d)\n", g.dims[0], g.dims[1], g.dims[2], ix, iy, z0,
                               z1), false;
          int64_t visited = 0;
          nerf_grid::for_run(g, keys.data(), 0, ix, iy, z0, z1, [&](int64_t, int64_t, int32_t) { ++visited; });
          nerf_grid::for_run(g, nullptr, 0, ix, iy, z0, z1, [&](int64_t, int64_t, int32_t) { ++visited; });
          if (visited) return std::printf("a visit of an empty array\n"), false;
        }
  return true;
}

}  // namespace

int main() {
  const int32_t shapes[3][3] = {{1, 1, 1}, {1, 3, 5}, {4, 4, 4}};
  bool ok = true;
  int64_t walks = 0;
  for (const auto& dims : shapes) {
    Grid g = {{-1.0f, 2.0f, 0.5f}, 0.25f, 4.0f, {dims[0], dims[1], dims[2]}};
    ok &= check_runs(g);
    // per axis: the centre of every cell, and one point beyond each of the two faces of the box
    std::vector<float> at[3];
    std::vector<int32_t> cell[3];
    for (int c = 0; c < 3; ++c) {
      at[c].push_back(g.lo[c] - 3.0f * g.cell), cell[c].push_back(0);
      for (int32_t i = 0; i < dims[c]; ++i) at[c].push_back(g.lo[c] + ((float)i + 0.5f) * g.cell), cell[c].push_back(i);
      at[c].push_back(g.lo[c] + ((float)dims[c] + 3.0f) * g.cell), cell[c].push_back(dims[c] - 1);
    }
    for (size_t x = 0; x < at[0].size(); ++x)
      for (size_t y = 0; y < at[1].size(); ++y)
        for (size_t z = 0; z < at[2].size(); ++z) {
          const float q[3] = {at[0][x], at[1][y], at[2][z]};
          const int32_t a[3] = {cell[0][x], cell[1][y], cell[2][z]};
          ok &= check_shells(g, q, a);
          ++walks;
        }
  }
  std::printf("%lld shell walks over 3 grids\n%s\n", (long long)walks, ok ? "ok" : "FAILED");
  return ok ? 0 : 1;
}
