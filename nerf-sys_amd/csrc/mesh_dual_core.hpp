// Dual contouring of a lattice: the per-point work of nerf_mesh_dual_classify / _edges / _cells (mesh_dual.hip),
// written once for the device and for a host compiler so that every branch can be run and checked under a host
// sanitizer without a GPU.  DESIGN §3.11.11 states the rule; tests/mesh_dual_reference.py restates it in numpy.
// Build with -ffp-contract=off: every operation below rounds on its own, in the order written.
//
// The lattice, the box, inside iff field > iso and the linear index p = (ix ny + iy) nz + iz are those of
// mesh_core.hpp.  Point p owns the axis edges p -> p + e_a, a = 0,1,2 (bit a of its edge mask), and cell p is the cell
// whose low corner is p.  Corner c of cell p is p + (c&1, c>>1&1, c>>2&1), so the axis edge a of corner c runs to
// corner c | (1 << a).
//
//  * A crossing edge carries the Hermite point marching tetrahedra puts on it (emit_vertex of mesh_core.hpp, reused,
//    so the bits are the same) and that function's grid normal.
//  * An active cell (it exists and its 8 inside bits are mixed) carries one vertex: the mean of its crossing edges'
//    points in the cell's centred coordinates, or the minimiser of their plane quadric (nerf_mq::add_plane / solve)
//    that starts at that mean; a solve that fails keeps the mean.
//  * An interior crossing edge (its four cells exist) carries one quad over those cells, two triangles.
//
// Slots at or past the totals (offsets that do not belong to this field) are neither read nor written.
#pragma once
#include "mesh_core.hpp"
#include "mesh_quadric_core.hpp"

namespace nerf_dual {

using nerf_mesh::Lattice;
using nerf_mesh::popc;

constexpr int PLACE_MEAN = 0, PLACE_QEF = 1;

// bit a: the owned axis edge a crosses; cell_flag: cell p is active; face_count: 2 per interior crossing edge
NERF_MESH_HD void classify_point(const float* __restrict__ field, const Lattice& L, int ix, int iy, int iz, int64_t p,
                                 uint8_t& edge_mask, int& edge_count, int& cell_flag, int& face_count) {
  float f[8];
  unsigned valid;
  const unsigned in = nerf_mesh::load_corners(field, L, ix, iy, iz, p, f, valid);
  const unsigned differ = (in ^ ((in & 1u) ? 0xffu : 0u)) & valid;  // bit c: corner c differs from corner 0
  const unsigned m = ((differ >> 1) & 1u) | (((differ >> 2) & 1u) << 1) | (((differ >> 4) & 1u) << 2);
  edge_mask = (uint8_t)m;
  edge_count = popc(m);
  cell_flag = (valid == 0xffu && in != 0u && in != 0xffu) ? 1 : 0;
  const bool mx = ix >= 1 && ix <= L.nx - 2, my = iy >= 1 && iy <= L.ny - 2, mz = iz >= 1 && iz <= L.nz - 2;
  face_count = ((m & 1u) && my && mz ? 2 : 0) + ((m & 2u) && mz && mx ? 2 : 0) + ((m & 4u) && mx && my ? 2 : 0);
}

// Hermite data of the edges point p owns: points (and grid normals, and keys = 3 p + a) at
// edge_off[p] + popcount(edge_mask[p] & ((1 << a) - 1))
NERF_MESH_HD void edges_point(const float* __restrict__ field, const Lattice& L, int ix, int iy, int iz, int64_t p,
                              const uint8_t* __restrict__ edge_mask, const int32_t* __restrict__ edge_off, int64_t E,
                              float* __restrict__ points, float* __restrict__ normals, int32_t* __restrict__ keys) {
  unsigned m = edge_mask[p] & 7u;
  if (ix + 1 >= L.nx) m &= ~1u;  // a bit no edge of this lattice stands behind is not followed
  if (iy + 1 >= L.ny) m &= ~2u;
  if (iz + 1 >= L.nz) m &= ~4u;
  if (!m) return;
  const int64_t sx = (int64_t)L.ny * L.nz, sy = L.nz;
  float f[8] = {field[p], 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (m & 1u) f[1] = field[p + sx];
  if (m & 2u) f[2] = field[p + sy];
  if (m & 4u) f[4] = field[p + 1];
  const int i[3] = {ix, iy, iz};
  float pa[3], ga[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int a = 0; a < 3; ++a) pa[a] = L.lo[a] + (float)i[a] * L.h[a];
  if (normals) nerf_mesh::lattice_gradient(field, L, ix, iy, iz, ga);
  const unsigned m7 = (m & 3u) | ((m & 4u) << 1);  // the bits of the edge classes 1, 2 and 4
  int64_t v = edge_off[p];
  if (v < 0) return;
  const int32_t key = 3 * (int32_t)p;
  if ((m & 1u) && keys && v < E) keys[v] = key;
  nerf_mesh::emit_vertex<1>(field, L, ix, iy, iz, m7, f, pa, ga, E, points, normals, v);
  if ((m & 2u) && keys && v < E) keys[v] = key + 1;
  nerf_mesh::emit_vertex<2>(field, L, ix, iy, iz, m7, f, pa, ga, E, points, normals, v);
  if ((m & 4u) && keys && v < E) keys[v] = key + 2;
  nerf_mesh::emit_vertex<4>(field, L, ix, iy, iz, m7, f, pa, ga, E, points, normals, v);
}

// what an active cell gathers from its crossing edges, in their order
struct CellSum {
  int count;
  double y0, y1, y2;  // the sum of the local points
  double s0, s1, s2;  // the sum of the normals
  nerf_mq::Quadric q;
};

// Edge (A, OB, OC) of the cell: axis A at the corner OB e_B + OC e_C, B = (A+1)%3, C = (A+2)%3; mk / eo: edge mask and
// first edge of the cell's corners 0..6
template <int A, int OB, int OC>
NERF_MESH_HD void cell_edge(const unsigned mk[7], const int eo[7], int64_t E, const float* __restrict__ points,
                            const float* __restrict__ normals, const float pa[3], const float h[3], bool qef,
                            CellSum& s) {
  constexpr int B = (A + 1) % 3, C = (A + 2) % 3, corner = (OB << B) | (OC << C);
  if (!((mk[corner] >> A) & 1u)) return;
  const int64_t e = (int64_t)eo[corner] + popc(mk[corner] & ((1u << A) - 1u));
  if (e < 0 || e >= E) return;
  double y[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double d = (double)points[3 * e + k] - (double)pa[k];
    y[k] = d / (double)h[k] - 0.5;
  }
  s.count += 1;
  s.y0 = s.y0 + y[0], s.y1 = s.y1 + y[1], s.y2 = s.y2 + y[2];
  if (!normals) return;
  const double n[3] = {(double)normals[3 * e], (double)normals[3 * e + 1], (double)normals[3 * e + 2]};
  s.s0 = s.s0 + n[0], s.s1 = s.s1 + n[1], s.s2 = s.s2 + n[2];
  if (qef) {
    const double m[3] = {n[0] * (double)h[0], n[1] * (double)h[1], n[2] * (double)h[2]};  // covariant: planes stay planes
    nerf_mq::add_plane(s.q, m, y);
  }
}

// the two triangles of the interior crossing edge (p, A): the cells p - e_B - e_C, p - e_C, p, p - e_B, counter-clockwise
// seen from +A, kept when p is inside (normals towards lower values) and reversed otherwise
template <int A>
NERF_MESH_HD void edge_quad(const Lattice& L, int64_t p, bool p_inside, const int32_t* __restrict__ cell_off, int64_t F,
                            int32_t* __restrict__ faces, int64_t& fo) {
  constexpr int B = (A + 1) % 3, C = (A + 2) % 3;
  const int64_t s[3] = {(int64_t)L.ny * L.nz, L.nz, 1};
  const int32_t v0 = cell_off[p - s[B] - s[C]], v1 = cell_off[p - s[C]], v2 = cell_off[p], v3 = cell_off[p - s[B]];
  if (fo >= 0 && fo + 1 < F) {
    int32_t* o = faces + 3 * fo;
    o[0] = v0, o[1] = p_inside ? v1 : v3, o[2] = v2;
    o[3] = v0, o[4] = v2, o[5] = p_inside ? v3 : v1;
  }
  fo += 2;
}

// the quads of the edges point p owns and the vertex of cell p
NERF_MESH_HD void cells_point(const float* __restrict__ field, const Lattice& L, int ix, int iy, int iz, int64_t p,
                              int64_t P, const uint8_t* __restrict__ edge_mask, const int32_t* __restrict__ edge_off,
                              const int32_t* __restrict__ cell_off, const int32_t* __restrict__ face_off,
                              const float* __restrict__ points, const float* __restrict__ normals, int placement,
                              double tol, int64_t V, int64_t F, float* __restrict__ verts, int32_t* __restrict__ faces,
                              float* __restrict__ vertex_normals, uint8_t* __restrict__ fallback) {
  float f[8];
  unsigned valid;
  const unsigned in = nerf_mesh::load_corners(field, L, ix, iy, iz, p, f, valid);
  const unsigned own = edge_mask[p];
  const bool mx = ix >= 1 && ix <= L.nx - 2, my = iy >= 1 && iy <= L.ny - 2, mz = iz >= 1 && iz <= L.nz - 2;
  if (F > 0 && (own & 7u)) {
    int64_t fo = face_off[p];
    const bool p_inside = in & 1u;
    if ((own & 1u) && my && mz) edge_quad<0>(L, p, p_inside, cell_off, F, faces, fo);
    if ((own & 2u) && mz && mx) edge_quad<1>(L, p, p_inside, cell_off, F, faces, fo);
    if ((own & 4u) && mx && my) edge_quad<2>(L, p, p_inside, cell_off, F, faces, fo);
  }
  if (valid != 0xffu || in == 0u || in == 0xffu) return;
  const int64_t v = cell_off[p];
  if (v < 0 || v >= V) return;
  const int64_t E = edge_off[P];
  const int64_t sx = (int64_t)L.ny * L.nz, sy = L.nz;
  unsigned mk[7];
  int eo[7];
#pragma unroll
  for (int c = 0; c < 7; ++c) {
    const int64_t q = p + ((c & 1) ? sx : 0) + ((c & 2) ? sy : 0) + ((c & 4) ? 1 : 0);
    mk[c] = edge_mask[q];
    eo[c] = edge_off[q];
  }
  const int i[3] = {ix, iy, iz};
  float pa[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) pa[a] = L.lo[a] + (float)i[a] * L.h[a];
  const bool qef = placement == PLACE_QEF;
  CellSum s{0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, nerf_mq::zero_quadric()};
  cell_edge<0, 0, 0>(mk, eo, E, points, normals, pa, L.h, qef, s);
  cell_edge<0, 1, 0>(mk, eo, E, points, normals, pa, L.h, qef, s);
  cell_edge<0, 0, 1>(mk, eo, E, points, normals, pa, L.h, qef, s);
  cell_edge<0, 1, 1>(mk, eo, E, points, normals, pa, L.h, qef, s);
  cell_edge<1, 0, 0>(mk, eo, E, points, normals, pa, L.h, qef, s);
  cell_edge<1, 1, 0>(mk, eo, E, points, normals, pa, L.h, qef, s);
  cell_edge<1, 0, 1>(mk, eo, E, points, normals, pa, L.h, qef, s);
  cell_edge<1, 1, 1>(mk, eo, E, points, normals, pa, L.h, qef, s);
  cell_edge<2, 0, 0>(mk, eo, E, points, normals, pa, L.h, qef, s);
  cell_edge<2, 1, 0>(mk, eo, E, points, normals, pa, L.h, qef, s);
  cell_edge<2, 0, 1>(mk, eo, E, points, normals, pa, L.h, qef, s);
  cell_edge<2, 1, 1>(mk, eo, E, points, normals, pa, L.h, qef, s);
  const double cnt = (double)s.count;  // 0 only with masks of another field: 0 / 0, a NaN vertex, never a wild write
  const double xbar[3] = {s.y0 / cnt, s.y1 / cnt, s.y2 / cnt};
  double x[3] = {xbar[0], xbar[1], xbar[2]};
  bool kept_mean = false;
  if (qef) {
    double xs[3] = {0.0, 0.0, 0.0};
    if (nerf_mq::solve(s.q, xbar, tol, xs)) x[0] = xs[0], x[1] = xs[1], x[2] = xs[2];
    else kept_mean = true;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) verts[3 * v + a] = pa[a] + (float)(x[a] + 0.5) * L.h[a];
  if (fallback) fallback[v] = kept_mean ? 1 : 0;
  if (vertex_normals) {
    const double xx = s.s0 * s.s0, yy = s.s1 * s.s1, zz = s.s2 * s.s2;
    const double len = sqrt((xx + yy) + zz);
    const double den = len > 1e-12 ? len : 1e-12;
    vertex_normals[3 * v] = (float)(s.s0 / den);
    vertex_normals[3 * v + 1] = (float)(s.s1 / den);
    vertex_normals[3 * v + 2] = (float)(s.s2 / den);
  }
}

}  // namespace nerf_dual
