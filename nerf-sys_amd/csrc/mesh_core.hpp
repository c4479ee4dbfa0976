// Marching tetrahedra over the Kuhn split of a lattice: the per-point work of nerf_mesh_classify / nerf_mesh_emit
// (mesh.hip), written once for the device and for a host compiler so that the case logic can be run and checked
// under a host sanitizer without a GPU.  DESIGN §3.11 states the rule; tests/mesh_reference.py restates it in numpy.
//
// Lattice (nx,ny,nz), linear index p = (ix ny + iy) nz + iz; inside iff field > iso.  Corner c of the cell at p is
// p + (c&1, c>>1&1, c>>2&1); the edge class d = 1..7 of point p runs to corner d.  Tetrahedron t of a cell has the
// corner masks TET[t] (a chain 0 < c1 < c2 < 7 in the subset order), so the edge between two of its corners belongs
// to the lower one with class (upper ^ lower).
//
// Tables, derived at compile time instead of typed in:
//  * the corners (A,B,C,D) of a sign case m (bit i = corner i of the tetrahedron is inside) as the rule names them,
//    and from them the tetra edges (01,02,03,12,13,23 -> 0..5) of q0..q3, 3 bits per case in one 64-bit word each;
//  * the orientation.  With midpoint vertices the rule's triangle normals are positive multiples of
//    det[B-A, C-A, D-A] times the direction from the inside to the outside corners when A is inside (one inside, and
//    two inside), and of its negative when A is outside (three inside); that determinant is the tetrahedron's
//    orientation (the sign of its axis permutation) times the sign of the permutation (A,B,C,D) of (0,1,2,3).  A
//    negative product swaps the second and third index.  The numpy reference decides the same question from cross
//    products of actual midpoints, so the two derivations are independent.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NERF_MESH_HD __host__ __device__ __forceinline__
#else
#define NERF_MESH_HD inline
#endif

namespace nerf_mesh {

constexpr int TET[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
constexpr int EI[6] = {0, 0, 0, 1, 1, 2}, EJ[6] = {1, 2, 3, 2, 3, 3};  // corners of tetra edge 0..5
constexpr int TET_SIGN[6] = {+1, -1, -1, +1, +1, -1};  // sign of the axis permutation (x,y,z), (x,z,y), ...

struct CaseCorners {
  int n, c[4];  // triangles, and (A,B,C,D)
};

constexpr CaseCorners case_corners(int m) {
  int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
  for (int i = 0; i < 4; ++i) {
    if ((m >> i) & 1) in[ni++] = i;
    else out[no++] = i;
  }
  if (ni == 0 || ni == 4) return {0, {0, 0, 0, 0}};
  if (ni == 2) return {2, {in[0], in[1], out[0], out[1]}};
  const int A = ni == 1 ? in[0] : out[0];
  CaseCorners r{1, {A, 0, 0, 0}};
  int k = 1;
  for (int i = 0; i < 4; ++i)
    if (i != A) r.c[k++] = i;
  return r;
}

constexpr int edge_id(int i, int j) {
  const int a = i < j ? i : j, b = i < j ? j : i;
  return a == 0 ? b - 1 : a + b;
}

// tetra edge of q_k for every case, 3 bits each (cases without that vertex hold 0)
constexpr uint64_t case_edges(int k) {
  uint64_t w = 0;
  for (int m = 0; m < 16; ++m) {
    const CaseCorners cc = case_corners(m);
    const int A = cc.c[0], B = cc.c[1], C = cc.c[2], D = cc.c[3];
    int e = 0;
    if (cc.n == 1) e = k == 0 ? edge_id(A, B) : k == 1 ? edge_id(A, C) : k == 2 ? edge_id(A, D) : 0;
    if (cc.n == 2) e = k == 0 ? edge_id(A, C) : k == 1 ? edge_id(A, D) : k == 2 ? edge_id(B, D) : edge_id(B, C);
    w |= (uint64_t)e << (3 * m);
  }
  return w;
}

constexpr int perm_sign(const int* c) {
  int s = 1;
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j)
      if (c[i] > c[j]) s = -s;
  return s;
}

// bit m: the triangles of case m in tetrahedron t are written with their second and third index swapped
constexpr uint32_t swap_bits(int t) {
  uint32_t w = 0;
  for (int m = 0; m < 16; ++m) {
    const CaseCorners cc = case_corners(m);
    if (!cc.n) continue;
    int s = TET_SIGN[t] * perm_sign(cc.c);
    if (!((m >> cc.c[0]) & 1)) s = -s;  // A outside (three corners inside)
    if (s < 0) w |= 1u << m;
  }
  return w;
}

constexpr uint64_t Q0 = case_edges(0), Q1 = case_edges(1), Q2 = case_edges(2), Q3 = case_edges(3);
constexpr uint32_t SWAP[6] = {swap_bits(0), swap_bits(1), swap_bits(2), swap_bits(3), swap_bits(4), swap_bits(5)};
static_assert(edge_id(0, 1) == 0 && edge_id(0, 3) == 2 && edge_id(1, 2) == 3 && edge_id(3, 2) == 5, "edge ids");
static_assert(SWAP[0] == (SWAP[1] ^ 0x7ffeu) && SWAP[0] == SWAP[3] && SWAP[1] == SWAP[5],
              "mirrored tetrahedra swap exactly the other cases");

struct Lattice {
  int nx, ny, nz;
  float iso;
  float lo[3], h[3];  // emit only
};

NERF_MESH_HD int popc(unsigned v) { return __builtin_popcount(v); }

// the 8 corner values of the cell at (ix,iy,iz); corners outside the lattice read as iso (outside, never used)
NERF_MESH_HD unsigned load_corners(const float* __restrict__ field, const Lattice& L, int ix, int iy, int iz, int64_t p,
                                   float f[8], unsigned& valid) {
  const bool bx = ix + 1 < L.nx, by = iy + 1 < L.ny, bz = iz + 1 < L.nz;
  const int64_t sx = (int64_t)L.ny * L.nz, sy = L.nz;
  unsigned in = 0;
  valid = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const bool ok = (!(c & 1) || bx) && (!(c & 2) || by) && (!(c & 4) || bz);
    f[c] = ok ? field[p + ((c & 1) ? sx : 0) + ((c & 2) ? sy : 0) + ((c & 4) ? 1 : 0)] : L.iso;
    in |= (f[c] > L.iso ? 1u : 0u) << c;
    valid |= (ok ? 1u : 0u) << c;
  }
  return in;
}

// inside bits of the four corners of tetrahedron T
template <int T>
NERF_MESH_HD unsigned tet_case(unsigned in) {
  return ((in >> TET[T][0]) & 1u) | (((in >> TET[T][1]) & 1u) << 1) | (((in >> TET[T][2]) & 1u) << 2) |
         (((in >> TET[T][3]) & 1u) << 3);
}

NERF_MESH_HD int case_tris(unsigned m) {
  const int n = popc(m);
  return n == 2 ? 2 : (n == 1 || n == 3) ? 1 : 0;
}

NERF_MESH_HD void classify_point(const float* __restrict__ field, const Lattice& L, int ix, int iy, int iz, int64_t p,
                                 uint8_t& edge_mask, int& face_count) {
  float f[8];
  unsigned valid;
  const unsigned in = load_corners(field, L, ix, iy, iz, p, f, valid);
  const unsigned differ = (in ^ ((in & 1u) ? 0xffu : 0u)) & valid;  // bit d: corner d differs from corner 0
  edge_mask = (uint8_t)(differ >> 1);
  int fc = 0;
  if (valid == 0xffu && in != 0u && in != 0xffu)
    fc = case_tris(tet_case<0>(in)) + case_tris(tet_case<1>(in)) + case_tris(tet_case<2>(in)) +
         case_tris(tet_case<3>(in)) + case_tris(tet_case<4>(in)) + case_tris(tet_case<5>(in));
  face_count = fc;
}

// d field / d world at lattice point (jx,jy,jz): central differences, one-sided on the border
NERF_MESH_HD void lattice_gradient(const float* __restrict__ field, const Lattice& L, int jx, int jy, int jz, float g[3]) {
  const int64_t sx = (int64_t)L.ny * L.nz, sy = L.nz;
  const int64_t q = ((int64_t)jx * L.ny + jy) * L.nz + jz;
  const int j[3] = {jx, jy, jz}, n[3] = {L.nx, L.ny, L.nz};
  const int64_t s[3] = {sx, sy, 1};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const bool up = j[a] + 1 < n[a], dn = j[a] > 0;
    const float fu = field[up ? q + s[a] : q], fd = field[dn ? q - s[a] : q];
    g[a] = (fu - fd) / (up && dn ? 2.0f * L.h[a] : L.h[a]);
  }
}

NERF_MESH_HD int pick6(const int e[6], unsigned k) {
  return k == 0 ? e[0] : k == 1 ? e[1] : k == 2 ? e[2] : k == 3 ? e[3] : k == 4 ? e[4] : e[5];
}

// vertex index of tetra edge K of tetrahedron T: the edge belongs to its lower corner `own` with class d
template <int T, int K>
NERF_MESH_HD int tet_vertex(const unsigned mk[7], const int vo[7]) {
  constexpr int own = TET[T][EI[K]], d = TET[T][EJ[K]] ^ own;
  return vo[own] + popc(mk[own] & ((1u << (d - 1)) - 1u));
}

// triangles of tetrahedron T of a cell; mk / vo: edge mask and first vertex of the cell's corners 0..6
template <int T>
NERF_MESH_HD void emit_tet(unsigned in, const unsigned mk[7], const int vo[7], int32_t* __restrict__ faces, int64_t F,
                           int64_t& fo) {
  const unsigned m = tet_case<T>(in);
  const int nt = case_tris(m);
  if (nt == 0) return;
  const int e[6] = {tet_vertex<T, 0>(mk, vo), tet_vertex<T, 1>(mk, vo), tet_vertex<T, 2>(mk, vo),
                    tet_vertex<T, 3>(mk, vo), tet_vertex<T, 4>(mk, vo), tet_vertex<T, 5>(mk, vo)};
  const unsigned sh = 3u * m;
  const int q0 = pick6(e, (unsigned)(Q0 >> sh) & 7u), q1 = pick6(e, (unsigned)(Q1 >> sh) & 7u),
            q2 = pick6(e, (unsigned)(Q2 >> sh) & 7u);
  const bool sw = (SWAP[T] >> m) & 1u;
  if (fo < F) {
    int32_t* o = faces + 3 * fo;
    o[0] = q0;
    o[1] = sw ? q2 : q1;
    o[2] = sw ? q1 : q2;
  }
  ++fo;
  if (nt == 2) {
    const int q3 = pick6(e, (unsigned)(Q3 >> sh) & 7u);
    if (fo < F) {
      int32_t* o = faces + 3 * fo;
      o[0] = q0;
      o[1] = sw ? q3 : q2;
      o[2] = sw ? q2 : q3;
    }
    ++fo;
  }
}

// the vertex (and grid normal) on the owned edge of class D, if it crosses; v = its index, advanced
template <int D>
NERF_MESH_HD void emit_vertex(const float* __restrict__ field, const Lattice& L, int ix, int iy, int iz, unsigned mask,
                              const float f[8], const float pa[3], const float ga[3], int64_t V,
                              float* __restrict__ verts, float* __restrict__ normals, int64_t& v) {
  if (!((mask >> (D - 1)) & 1u)) return;
  const float t = (f[0] - L.iso) / (f[0] - f[D]);
  if (v < V) {
    const float ib[3] = {(float)(ix + 1), (float)(iy + 1), (float)(iz + 1)};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float pb = ((D >> a) & 1) ? L.lo[a] + ib[a] * L.h[a] : pa[a];
      verts[3 * v + a] = pa[a] + t * (pb - pa[a]);
    }
    if (normals) {
      float gb[3], g[3];
      lattice_gradient(field, L, ix + (D & 1), iy + ((D >> 1) & 1), iz + ((D >> 2) & 1), gb);
#pragma unroll
      for (int a = 0; a < 3; ++a) g[a] = ga[a] + t * (gb[a] - ga[a]);
      const float den = fmaxf(sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]), 1e-12f);
#pragma unroll
      for (int a = 0; a < 3; ++a) normals[3 * v + a] = -g[a] / den;
    }
  }
  ++v;
}

// vertices (and grid normals) of the edges point p owns, and the triangles of the cell at p.  Every output slot has
// one writer; a slot index at or past V / F (offsets that do not belong to this field) is not written.
NERF_MESH_HD void emit_point(const float* __restrict__ field, const Lattice& L, int ix, int iy, int iz, int64_t p,
                             const uint8_t* __restrict__ edge_mask, const int32_t* __restrict__ vert_off,
                             const int32_t* __restrict__ face_off, int64_t V, int64_t F, float* __restrict__ verts,
                             int32_t* __restrict__ faces, float* __restrict__ normals) {
  float f[8];
  unsigned valid;
  const unsigned in = load_corners(field, L, ix, iy, iz, p, f, valid);
  const unsigned mask = edge_mask[p];
  if (mask) {
    int64_t v = vert_off[p];
    const int i[3] = {ix, iy, iz};
    float pa[3], ga[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int a = 0; a < 3; ++a) pa[a] = L.lo[a] + (float)i[a] * L.h[a];
    if (normals) lattice_gradient(field, L, ix, iy, iz, ga);
    emit_vertex<1>(field, L, ix, iy, iz, mask, f, pa, ga, V, verts, normals, v);
    emit_vertex<2>(field, L, ix, iy, iz, mask, f, pa, ga, V, verts, normals, v);
    emit_vertex<3>(field, L, ix, iy, iz, mask, f, pa, ga, V, verts, normals, v);
    emit_vertex<4>(field, L, ix, iy, iz, mask, f, pa, ga, V, verts, normals, v);
    emit_vertex<5>(field, L, ix, iy, iz, mask, f, pa, ga, V, verts, normals, v);
    emit_vertex<6>(field, L, ix, iy, iz, mask, f, pa, ga, V, verts, normals, v);
    emit_vertex<7>(field, L, ix, iy, iz, mask, f, pa, ga, V, verts, normals, v);
  }
  if (valid != 0xffu || in == 0u || in == 0xffu) return;
  const int64_t sx = (int64_t)L.ny * L.nz, sy = L.nz;
  unsigned mk[7];
  int vo[7];
#pragma unroll
  for (int c = 0; c < 7; ++c) {
    const int64_t q = p + ((c & 1) ? sx : 0) + ((c & 2) ? sy : 0) + ((c & 4) ? 1 : 0);
    mk[c] = edge_mask[q];
    vo[c] = vert_off[q];
  }
  int64_t fo = face_off[p];
  emit_tet<0>(in, mk, vo, faces, F, fo);
  emit_tet<1>(in, mk, vo, faces, F, fo);
  emit_tet<2>(in, mk, vo, faces, F, fo);
  emit_tet<3>(in, mk, vo, faces, F, fo);
  emit_tet<4>(in, mk, vo, faces, F, fo);
  emit_tet<5>(in, mk, vo, faces, F, fo);
}

}  // namespace nerf_mesh
