// Mesh extraction from a density lattice by dual contouring.
//
//   nerf_mesh_dual_classify  one thread per lattice point p: the crossing bits of the 3 axis edges p owns (edge_mask),
//                            their number, whether the cell whose low corner is p is active, and 2 x the interior
//                            crossing edges of p (its triangles).
//   nerf_exclusive_scan_i32 over the three count arrays (occ.hip) gives every point its first edge, its cell's vertex
//                            and its first face.
//   nerf_mesh_dual_edges     one thread per lattice point: the Hermite data of its crossing edges (marching
//                            tetrahedra's vertex and grid normal on that edge, and the key 3 p + a).
//   nerf_mesh_dual_cells     one thread per lattice point: its cell's vertex from the Hermite data of the cell's up to
//                            12 crossing edges (their mean, or the minimiser of their plane quadric), and the quads of
//                            its interior crossing edges.  points / normals are plain inputs: the caller may replace
//                            what the second kernel wrote (refined crossings, normals of the field itself).
//
// The per-point work is csrc/mesh_dual_core.hpp, shared with host builds.  The launch shape is mesh.hip's: the linear
// map with consecutive lanes along iz, so corner loads are shared through the vector cache and a wave's stores fall into
// contiguous runs.  No LDS, no atomics: every output slot has one writer, so equal inputs give equal bits.  In the third
// kernel only the threads of active cells gather and solve; the others leave after their corner loads.  This file is
// compiled with -ffp-contract=off (Makefile): every fp32 and double operation rounds once, as the numpy reference
// rounds them.
#include "common.hpp"
#include "mesh_dual_core.hpp"

namespace {

using nerf_mesh::Lattice;
constexpr int NTHREADS = 256;

// the linear map of mesh.hip (measured there against five tiled workgroup shapes)
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

__global__ __launch_bounds__(NTHREADS) void mesh_dual_classify_kernel(const float* __restrict__ field, Lattice L,
                                                                      int64_t P, uint8_t* __restrict__ edge_mask,
                                                                      int32_t* __restrict__ edge_count,
                                                                      int32_t* __restrict__ cell_flag,
                                                                      int32_t* __restrict__ face_count) {
  int64_t p;
  int ix, iy, iz;
  if (!point_of_thread(L, P, p, ix, iy, iz)) return;
  uint8_t mask;
  int ec, cf, fc;
  nerf_dual::classify_point(field, L, ix, iy, iz, p, mask, ec, cf, fc);
  edge_mask[p] = mask;
  edge_count[p] = ec;
  cell_flag[p] = cf;
  face_count[p] = fc;
}

__global__ __launch_bounds__(NTHREADS) void mesh_dual_edges_kernel(const float* __restrict__ field, Lattice L, int64_t P,
                                                                   const uint8_t* __restrict__ edge_mask,
                                                                   const int32_t* __restrict__ edge_off, int64_t E,
                                                                   float* __restrict__ points,
                                                                   float* __restrict__ normals,
                                                                   int32_t* __restrict__ keys) {
  int64_t p;
  int ix, iy, iz;
  if (!point_of_thread(L, P, p, ix, iy, iz)) return;
  nerf_dual::edges_point(field, L, ix, iy, iz, p, edge_mask, edge_off, E, points, normals, keys);
}

__global__ __launch_bounds__(NTHREADS) void mesh_dual_cells_kernel(
    const float* __restrict__ field, Lattice L, int64_t P, const uint8_t* __restrict__ edge_mask,
    const int32_t* __restrict__ edge_off, const int32_t* __restrict__ cell_off, const int32_t* __restrict__ face_off,
    const float* __restrict__ points, const float* __restrict__ normals, int placement, double tol, int64_t V, int64_t F,
    float* __restrict__ verts, int32_t* __restrict__ faces, float* __restrict__ vertex_normals,
    uint8_t* __restrict__ fallback) {
  int64_t p;
  int ix, iy, iz;
  if (!point_of_thread(L, P, p, ix, iy, iz)) return;
  nerf_dual::cells_point(field, L, ix, iy, iz, p, P, edge_mask, edge_off, cell_off, face_off, points, normals, placement,
                         tol, V, F, verts, faces, vertex_normals, fallback);
}

// dimensions >= 2 and 12 P < 2^31, the bound of nerf_mesh_classify: edges (<= 3 P), cells (<= P), faces (<= 6 P), the
// keys 3 p + a and the int32 scans cannot overflow
bool lattice_ok(int nx, int ny, int nz, int64_t& P) {
  if (nx < 2 || ny < 2 || nz < 2) return false;
  P = (int64_t)nx * ny * nz;
  return 12 * P < (int64_t(1) << 31);
}

bool box_lattice(int nx, int ny, int nz, float iso, const float* lo, const float* hi, Lattice& L) {
  if (!lo || !hi || !(lo[0] < hi[0] && lo[1] < hi[1] && lo[2] < hi[2])) return false;
  L = Lattice{nx, ny, nz, iso, {lo[0], lo[1], lo[2]}, {0.f, 0.f, 0.f}};
  const int n[3] = {nx, ny, nz};
  for (int a = 0; a < 3; ++a) L.h[a] = (hi[a] - lo[a]) / (float)(n[a] - 1);
  return true;
}

}  // namespace

extern "C" int nerf_mesh_dual_classify(const float* field, int nx, int ny, int nz, float iso, uint8_t* edge_mask,
                                       int32_t* edge_count, int32_t* cell_flag, int32_t* face_count,
                                       hipStream_t stream) {
  int64_t P = 0;
  NERF_CHECK_ARG(lattice_ok(nx, ny, nz, P));
  NERF_CHECK_ARG(field && edge_mask && edge_count && cell_flag && face_count);
  Lattice L{nx, ny, nz, iso, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
  mesh_dual_classify_kernel<<<(unsigned)nerf_cdiv(P, NTHREADS), NTHREADS, 0, stream>>>(field, L, P, edge_mask,
                                                                                       edge_count, cell_flag, face_count);
  return nerf_launch_status();
}

extern "C" int nerf_mesh_dual_edges(const float* field, int nx, int ny, int nz, float iso, const float* lo,
                                    const float* hi, const uint8_t* edge_mask, const int32_t* edge_off, int64_t E,
                                    float* points, float* normals, int32_t* keys, hipStream_t stream) {
  int64_t P = 0;
  Lattice L;
  NERF_CHECK_ARG(lattice_ok(nx, ny, nz, P));
  NERF_CHECK_ARG(box_lattice(nx, ny, nz, iso, lo, hi, L));
  NERF_CHECK_ARG(E >= 0 && E <= 3 * P);
  if (E == 0) return NERF_OK;  // nothing crosses: no launch on empty outputs
  NERF_CHECK_ARG(field && edge_mask && edge_off && points);
  mesh_dual_edges_kernel<<<(unsigned)nerf_cdiv(P, NTHREADS), NTHREADS, 0, stream>>>(field, L, P, edge_mask, edge_off, E,
                                                                                    points, normals, keys);
  return nerf_launch_status();
}

extern "C" int nerf_mesh_dual_cells(const float* field, int nx, int ny, int nz, float iso, const float* lo,
                                    const float* hi, const uint8_t* edge_mask, const int32_t* edge_off,
                                    const int32_t* cell_off, const int32_t* face_off, const float* points,
                                    const float* normals, int placement, double tol, int64_t V, int64_t F, float* verts,
                                    int32_t* faces, float* vertex_normals, uint8_t* fallback, hipStream_t stream) {
  int64_t P = 0;
  Lattice L;
  NERF_CHECK_ARG(lattice_ok(nx, ny, nz, P));
  NERF_CHECK_ARG(box_lattice(nx, ny, nz, iso, lo, hi, L));
  NERF_CHECK_ARG(placement == nerf_dual::PLACE_MEAN || placement == nerf_dual::PLACE_QEF);
  NERF_CHECK_ARG(tol > 0.0 && tol < 1.0);  // a NaN fails both
  NERF_CHECK_ARG(V >= 0 && F >= 0 && V <= P && F <= 6 * P && (V > 0 || F == 0));
  NERF_CHECK_ARG(normals || (placement == nerf_dual::PLACE_MEAN && !vertex_normals));
  if (V == 0) return NERF_OK;  // no active cell, so no quad either: no launch on empty outputs
  NERF_CHECK_ARG(field && edge_mask && edge_off && cell_off && face_off && points && verts && (F == 0 || faces));
  mesh_dual_cells_kernel<<<(unsigned)nerf_cdiv(P, NTHREADS), NTHREADS, 0, stream>>>(
      field, L, P, edge_mask, edge_off, cell_off, face_off, points, normals, placement, tol, V, F, verts, faces,
      vertex_normals, fallback);
  return nerf_launch_status();
}
