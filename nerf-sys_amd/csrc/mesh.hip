// Mesh extraction from a density lattice: marching tetrahedra over the Kuhn split.
//
//   nerf_mesh_classify  one thread per lattice point p: the crossing bits of the 7 edges p owns (edge_mask), their
//                       number (vert_count) and the triangles of the cell whose low corner is p (face_count).
//   nerf_exclusive_scan_i32 over both count arrays (occ.hip) gives every point its first vertex and first face.
//   nerf_mesh_emit      one thread per lattice point: the point's vertices (and grid normals), its cell's triangles.
//                       The vertex on edge (q, d) has index vert_off[q] + popcount(edge_mask[q] & ((1 << (d-1)) - 1)).
//
// The per-point work is csrc/mesh_core.hpp, shared with host builds.  Both kernels stream: consecutive lanes walk iz,
// so a thread's 8 corner loads are 4 row pairs that its neighbours along iz share through the vector cache, and a
// wave's vertex and face stores fall into one contiguous run each.  No LDS, no atomics: every output slot has one
// writer, so equal inputs give equal bits.  This file is compiled with -ffp-contract=off (Makefile): vertex positions
// are pa + t (pb - pa) with every product and sum rounded once, as the numpy reference rounds them.
#include "common.hpp"
#include "mesh_core.hpp"

namespace {

using nerf_mesh::Lattice;
constexpr int NTHREADS = 256;

// Linear map, consecutive lanes along iz.  Workgroups of 2x2x64, 1x4x64, 2x4x32, 4x1x64 and 1x2x128 points were
// measured against it and were 2-19 % slower at 512^3 (profiles/mesh_thread_map_ab.txt).
__device__ __forceinline__ bool point_of_thread(const Lattice& L, int64_t P, int64_t& p, int& ix, int& iy, int& iz) {
  p = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (p >= P) return false;
  const int q = (int)p;  // P < 2^31 / 12
  const int r = q / L.nz;
  iz = q - r * L.nz;
  ix = r / L.ny;
  iy = r - ix * L.ny;
  return true;
}

__global__ __launch_bounds__(NTHREADS) void mesh_classify_kernel(const float* __restrict__ field, Lattice L, int64_t P,
                                                                 uint8_t* __restrict__ edge_mask,
                                                                 int32_t* __restrict__ vert_count,
                                                                 int32_t* __restrict__ face_count) {
  int64_t p;
  int ix, iy, iz;
  if (!point_of_thread(L, P, p, ix, iy, iz)) return;
  uint8_t mask;
  int fc;
  nerf_mesh::classify_point(field, L, ix, iy, iz, p, mask, fc);
  edge_mask[p] = mask;
  vert_count[p] = nerf_mesh::popc(mask);
  face_count[p] = fc;
}

__global__ __launch_bounds__(NTHREADS) void mesh_emit_kernel(const float* __restrict__ field, Lattice L, int64_t P,
                                                             const uint8_t* __restrict__ edge_mask,
                                                             const int32_t* __restrict__ vert_off,
                                                             const int32_t* __restrict__ face_off, int64_t V, int64_t F,
                                                             float* __restrict__ verts, int32_t* __restrict__ faces,
                                                             float* __restrict__ normals) {
  int64_t p;
  int ix, iy, iz;
  if (!point_of_thread(L, P, p, ix, iy, iz)) return;
  nerf_mesh::emit_point(field, L, ix, iy, iz, p, edge_mask, vert_off, face_off, V, F, verts, faces, normals);
}

// dimensions >= 2 and 12 P < 2^31: vertex (<= 7 P) and face (<= 12 P) numbers and their int32 scans cannot overflow
bool lattice_ok(int nx, int ny, int nz, int64_t& P) {
  if (nx < 2 || ny < 2 || nz < 2) return false;
  P = (int64_t)nx * ny * nz;
  return 12 * P < (int64_t(1) << 31);
}

}  // namespace

extern "C" int nerf_mesh_classify(const float* field, int nx, int ny, int nz, float iso, uint8_t* edge_mask,
                                  int32_t* vert_count, int32_t* face_count, hipStream_t stream) {
  int64_t P = 0;
  NERF_CHECK_ARG(lattice_ok(nx, ny, nz, P));
  NERF_CHECK_ARG(field && edge_mask && vert_count && face_count);
  Lattice L{nx, ny, nz, iso, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
  mesh_classify_kernel<<<(unsigned)nerf_cdiv(P, NTHREADS), NTHREADS, 0, stream>>>(field, L, P, edge_mask, vert_count,
                                                                                  face_count);
  return nerf_launch_status();
}

extern "C" int nerf_mesh_emit(const float* field, int nx, int ny, int nz, float iso, const float* lo, const float* hi,
                              const uint8_t* edge_mask, const int32_t* vert_off, const int32_t* face_off, int64_t V,
                              int64_t F, float* verts, int32_t* faces, float* normals, hipStream_t stream) {
  int64_t P = 0;
  NERF_CHECK_ARG(lattice_ok(nx, ny, nz, P));
  NERF_CHECK_ARG(lo && hi && V >= 0 && F >= 0 && V <= 7 * P && F <= 12 * P);
  NERF_CHECK_ARG(lo[0] < hi[0] && lo[1] < hi[1] && lo[2] < hi[2]);
  if (V == 0 && F == 0) return NERF_OK;  // nothing crosses: no launch on empty outputs
  NERF_CHECK_ARG(field && edge_mask && vert_off && face_off && (V == 0 || verts) && (F == 0 || faces));
  Lattice L{nx, ny, nz, iso, {lo[0], lo[1], lo[2]}, {0.f, 0.f, 0.f}};
  const int n[3] = {nx, ny, nz};
  for (int a = 0; a < 3; ++a) L.h[a] = (hi[a] - lo[a]) / (float)(n[a] - 1);
  mesh_emit_kernel<<<(unsigned)nerf_cdiv(P, NTHREADS), NTHREADS, 0, stream>>>(field, L, P, edge_mask, vert_off, face_off,
                                                                              V, F, verts, faces, V ? normals : nullptr);
  return nerf_launch_status();
}
