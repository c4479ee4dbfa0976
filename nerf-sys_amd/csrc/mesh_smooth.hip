// Mesh smoothing on the device (the shared core is mesh_smooth_core.hpp).
//
//   The two adjacencies (vertex -> neighbouring vertices, vertex -> faces) are CSR lists built by sorting int64 keys:
//   nerf_mesh_pair_keys    one thread per key: the 6 F directed pairs (mode 0) or the 3 F (vertex, face) pairs (mode 1).
//   (the caller sorts the keys ascending)
//   nerf_mesh_csr_flags    one thread per key: flags[i] = first of its run and no sentinel; a run of exactly one
//                          directed pair marks its first vertex as a boundary vertex (a plain store of 1).
//   (the caller scans the flags: pos, E = pos[n])
//   nerf_mesh_csr_build    one thread per key scatters the flagged entries to col[pos[i]]; one thread per vertex finds
//                          its row start by a bounded binary search over the sorted keys.
//   nerf_mesh_smooth_pass  one thread per vertex: a Jacobi step over its row, summed in the row's order in double.
//   nerf_mesh_vertex_normals  one thread per vertex: the normalised sum of its faces' cross products, in the row's order.
//
// No atomics at all: every output element has one writer, or (the boundary flags) several writers of the same value.
// The kernels do not check indices or finiteness: that is the caller's duty (kernels.py validates before launching).
#include "common.hpp"
#include "mesh_grid_host.hpp"
#include "mesh_smooth_core.hpp"

namespace {

constexpr int NTHREADS = 256;

__global__ __launch_bounds__(NTHREADS) void pair_keys_kernel(const int32_t* __restrict__ faces, int64_t n, int mode,
                                                             int64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (i >= n) return;
  keys[i] = mode == 0 ? nerf_ms::pair_key(faces, i) : nerf_ms::vertex_face_key(faces, i);
}

__global__ __launch_bounds__(NTHREADS) void csr_flags_kernel(const int64_t* __restrict__ keys, int64_t n,
                                                             int32_t* __restrict__ flags, uint8_t* boundary) {
  const int64_t i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (i >= n) return;
  const int32_t f = nerf_ms::run_flag(keys, i);
  flags[i] = f;
  if (boundary && f && nerf_ms::run_is_single(keys, n, i)) boundary[nerf_ms::key_row(keys[i])] = 1;
}

// threads [0, n): the entries; threads [0, V]: the row starts
__global__ __launch_bounds__(NTHREADS) void csr_build_kernel(const int64_t* __restrict__ keys, int64_t n,
                                                             const int32_t* __restrict__ flags,
                                                             const int32_t* __restrict__ pos, int64_t V, int64_t E,
                                                             int32_t* __restrict__ row_off, int32_t* __restrict__ col) {
  const int64_t i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (i < n && flags[i]) {
    const int64_t at = pos[i];
    if (at < E) col[at] = nerf_ms::key_entry(keys[i]);  // at < E always holds for the caller's own flags / pos / E
  }
  if (i <= V) row_off[i] = nerf_ms::row_start(keys, n, pos, i);
}

__global__ __launch_bounds__(NTHREADS) void smooth_pass_kernel(const float* __restrict__ v_in,
                                                               const int32_t* __restrict__ row_off,
                                                               const int32_t* __restrict__ col,
                                                               const uint8_t* __restrict__ fixed, int64_t V, float s,
                                                               float* __restrict__ v_out) {
  const int64_t v = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (v >= V) return;
  nerf_ms::smooth_vertex(v_in, row_off, col, fixed, v, s, v_out);
}

__global__ __launch_bounds__(NTHREADS) void vertex_normals_kernel(const float* __restrict__ verts,
                                                                  const int32_t* __restrict__ faces,
                                                                  const int32_t* __restrict__ row_off,
                                                                  const int32_t* __restrict__ col, int64_t V,
                                                                  float* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (v >= V) return;
  nerf_ms::vertex_normal(verts, faces, row_off, col, v, out);
}

using nerf_grid::aligned8;
using nerf_grid::LIMIT;

}  // namespace

extern "C" int nerf_mesh_pair_keys(const int32_t* faces, int64_t F, int mode, int64_t* keys, hipStream_t stream) {
  NERF_CHECK_ARG(F >= 0 && 6 * F < LIMIT && (mode == 0 || mode == 1));
  if (F == 0) return NERF_OK;
  NERF_CHECK_ARG(faces && keys);
  if (!aligned8(keys)) return NERF_E_ALIGN;
  const int64_t n = (mode == 0 ? 6 : 3) * F;
  pair_keys_kernel<<<(unsigned)nerf_cdiv(n, NTHREADS), NTHREADS, 0, stream>>>(faces, n, mode, keys);
  return nerf_launch_status();
}

extern "C" int nerf_mesh_csr_flags(const int64_t* sorted_keys, int64_t n, int32_t* flags, uint8_t* boundary,
                                   hipStream_t stream) {
  NERF_CHECK_ARG(n >= 0 && n < LIMIT);
  if (n == 0) return NERF_OK;
  NERF_CHECK_ARG(sorted_keys && flags);
  if (!aligned8(sorted_keys)) return NERF_E_ALIGN;
  csr_flags_kernel<<<(unsigned)nerf_cdiv(n, NTHREADS), NTHREADS, 0, stream>>>(sorted_keys, n, flags, boundary);
  return nerf_launch_status();
}

extern "C" int nerf_mesh_csr_build(const int64_t* sorted_keys, int64_t n, const int32_t* flags, const int32_t* pos,
                                   int64_t V, int64_t E, int32_t* row_off, int32_t* col, hipStream_t stream) {
  NERF_CHECK_ARG(n >= 0 && n < LIMIT && V >= 0 && V < LIMIT && E >= 0 && E <= n);
  NERF_CHECK_ARG(row_off != nullptr);
  if (n == 0) return nerf_hip_status(hipMemsetAsync(row_off, 0, (size_t)(V + 1) * sizeof(int32_t), stream));
  NERF_CHECK_ARG(sorted_keys && flags && pos && (E == 0 || col));
  if (!aligned8(sorted_keys)) return NERF_E_ALIGN;
  const int64_t threads = n > V + 1 ? n : V + 1;
  csr_build_kernel<<<(unsigned)nerf_cdiv(threads, NTHREADS), NTHREADS, 0, stream>>>(sorted_keys, n, flags, pos, V, E,
                                                                                   row_off, col);
  return nerf_launch_status();
}

extern "C" int nerf_mesh_smooth_pass(const float* v_in, const int32_t* row_off, const int32_t* col,
                                     const uint8_t* fixed, int64_t V, float s, float* v_out, hipStream_t stream) {
  NERF_CHECK_ARG(V >= 0 && V < LIMIT);
  if (V == 0) return NERF_OK;
  NERF_CHECK_ARG(v_in && row_off && v_out && v_out != v_in);  // col may be NULL: a mesh without an edge
  smooth_pass_kernel<<<(unsigned)nerf_cdiv(V, NTHREADS), NTHREADS, 0, stream>>>(v_in, row_off, col, fixed, V, s, v_out);
  return nerf_launch_status();
}

extern "C" int nerf_mesh_vertex_normals(const float* vertices, const int32_t* faces, const int32_t* row_off,
                                        const int32_t* col, int64_t V, float* normals_out, hipStream_t stream) {
  NERF_CHECK_ARG(V >= 0 && V < LIMIT);
  if (V == 0) return NERF_OK;
  NERF_CHECK_ARG(vertices && row_off && normals_out && normals_out != vertices);  // faces / col NULL: no face at all
  vertex_normals_kernel<<<(unsigned)nerf_cdiv(V, NTHREADS), NTHREADS, 0, stream>>>(vertices, faces, row_off, col, V,
                                                                                  normals_out);
  return nerf_launch_status();
}
