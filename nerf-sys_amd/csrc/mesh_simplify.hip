// Mesh simplification by vertex clustering on the device (the shared core is mesh_simplify_core.hpp).
//
//   nerf_mesh_cluster_labels  labels[v] = smallest vertex index in v's grid cell.
//     1. keys      one thread per vertex: keys[v] = the int64 cell key.
//     2. insert    one thread per vertex: the hash set of vertex indices (slot key = keys[slot value]).
//     3. lookup    one thread per vertex: labels[v] = the value of the slot of v's key.  The kernel boundary makes
//                  every insert visible.
//   nerf_mesh_cluster_reduce  fixed-point sums per cluster at the row labels[v], then one thread per vertex finalizes.
//     1. init      the accumulator rows and counts to zero.
//     2. accumulate one thread per vertex: 64-bit integer atomicAdd of the quantised position / normal / colour, an
//                  int32 atomicAdd of the count.  Integer sums are associative: the order of arrival does not matter.
//     3. finalize  one thread per vertex: a representative's rows from the sums in double precision, zeros elsewhere.
//   nerf_mesh_cluster_faces   faces_out = labels[faces], keep = non-degenerate and first of its canonical form.
//     1. remap     one thread per face: writes faces_out.
//     2. insert    one thread per non-degenerate face: the hash set of face indices (slot key = the canonical triple
//                  of faces_out[slot value], written by the launch before).
//     3. lookup    one thread per face: keep[f] = non-degenerate && slot value == f.
//   nerf_mesh_cluster_quadric  the quadric-error position of every cluster (mesh_quadric_core.hpp).
//     1. place     one thread per vertex row: a representative sums the plane quadrics of its row of the
//                  vertex-to-face adjacency in the row's order, solves from the mean and stores its position and flag;
//                  every other row stores zeros.  No atomics, one writer per element.
//   status[0] != 0 reports a thread that exhausted its probe bound; status[1] is the longest probe chain.
//
// The kernels do not check indices or finiteness: that is the caller's duty (kernels.py validates before launching).
#include "common.hpp"
#include "mesh_grid_host.hpp"
#include "mesh_quadric_core.hpp"
#include "mesh_simplify_core.hpp"

namespace {

constexpr int NTHREADS = 256;
using nerf_hs::Grid;

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)v, d, 64);
    v = o > v ? o : v;
  }
  return v;
}

// every lane of the wave calls this (no early return before it)
__device__ __forceinline__ void report(int32_t* status, bool ok, uint32_t probes, int32_t bit) {
  if (!ok) atomicOr(status, bit);
  probes = wave_max_u32(probes);
  if (nerf_lane() == 0 && probes) atomicMax(status + 1, (int32_t)(probes > 0x7fffffffu ? 0x7fffffffu : probes));
}

struct SameKey {
  const int64_t* keys;
  __device__ __forceinline__ bool operator()(int32_t a, int32_t b) const { return keys[a] == keys[b]; }
};

__global__ __launch_bounds__(NTHREADS) void cluster_keys_kernel(const float* __restrict__ verts, int64_t V, Grid g,
                                                                int64_t* __restrict__ keys) {
  const int64_t v = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (v >= V) return;
  const float p[3] = {verts[3 * v], verts[3 * v + 1], verts[3 * v + 2]};
  keys[v] = nerf_hs::cell_key(g, p);
}

__global__ __launch_bounds__(NTHREADS) void cluster_insert_kernel(const int64_t* __restrict__ keys, int64_t V,
                                                                  int32_t* table, uint32_t mask,
                                                                  int32_t* __restrict__ status) {
  const int64_t v = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  uint32_t probes = 0;
  bool ok = true;
  if (v < V) ok = nerf_hs::insert(table, mask, nerf_hs::mix((uint64_t)keys[v]), (int32_t)v, SameKey{keys}, probes);
  report(status, ok, probes, 1);
}

__global__ __launch_bounds__(NTHREADS) void cluster_lookup_kernel(const int64_t* __restrict__ keys, int64_t V,
                                                                  const int32_t* __restrict__ table, uint32_t mask,
                                                                  int32_t* __restrict__ labels,
                                                                  int32_t* __restrict__ status) {
  const int64_t v = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  uint32_t probes = 0;
  bool ok = true;
  if (v < V) {
    const int32_t l = nerf_hs::lookup(table, mask, nerf_hs::mix((uint64_t)keys[v]), (int32_t)v, SameKey{keys}, probes);
    ok = l >= 0;
    labels[v] = ok ? l : (int32_t)v;  // a valid index even when the status word reports the failure
  }
  report(status, ok, probes, 2);
}

// ---------------------------------------------------------------- reduce

__global__ __launch_bounds__(NTHREADS) void reduce_init_kernel(unsigned long long* __restrict__ acc, int64_t n_words,
                                                               int32_t* __restrict__ count, int64_t V) {
  const int64_t i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (i < n_words) acc[i] = 0ull;
  if (i < V) count[i] = 0;
}

__global__ __launch_bounds__(NTHREADS) void reduce_accumulate_kernel(const float* __restrict__ verts,
                                                                     const int32_t* __restrict__ labels,
                                                                     const float* __restrict__ normals,
                                                                     const float* __restrict__ colors, int64_t V, Grid g,
                                                                     int words, unsigned long long* acc,
                                                                     int32_t* count) {
  const int64_t v = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (v >= V) return;
  unsigned long long* row = acc + (int64_t)labels[v] * words;
#pragma unroll
  for (int c = 0; c < 3; ++c) atomicAdd(row + c, (unsigned long long)nerf_hs::quant_pos(g, c, verts[3 * v + c]));
  int w = 3;
  if (normals) {
#pragma unroll
    for (int c = 0; c < 3; ++c)  // two's complement: the unsigned sum of the int64 bit patterns is the int64 sum
      atomicAdd(row + w + c, (unsigned long long)nerf_hs::quant_normal(normals[3 * v + c]));
    w += 3;
  }
  if (colors) {
#pragma unroll
    for (int c = 0; c < 3; ++c) atomicAdd(row + w + c, (unsigned long long)nerf_hs::quant_color(colors[3 * v + c]));
  }
  atomicAdd(count + labels[v], 1);
}

__global__ __launch_bounds__(NTHREADS) void reduce_finalize_kernel(const float* __restrict__ verts,
                                                                   const int32_t* __restrict__ labels, int64_t V, Grid g,
                                                                   int words, int has_normals, int has_colors,
                                                                   const unsigned long long* __restrict__ acc,
                                                                   const int32_t* __restrict__ count,
                                                                   float* __restrict__ out_v, float* __restrict__ out_n,
                                                                   float* __restrict__ out_c) {
  const int64_t v = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (v >= V) return;
  const bool rep = labels[v] == (int32_t)v;
  const unsigned long long* row = acc + v * words;
  const int32_t n = rep ? count[v] : 1;  // a representative counts itself: n >= 1
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int32_t i = nerf_hs::cell_index(g, c, verts[3 * v + c]);
    out_v[3 * v + c] = rep ? nerf_hs::mean_pos(g, c, i, row[c], n) : 0.0f;
  }
  int w = 3;
  if (has_normals) {
    float o[3] = {0.0f, 0.0f, 0.0f};
    if (rep) {
      const int64_t s[3] = {(int64_t)row[w], (int64_t)row[w + 1], (int64_t)row[w + 2]};
      nerf_hs::unit_normal(s, o);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out_n[3 * v + c] = o[c];
    w += 3;
  }
  if (has_colors) {
#pragma unroll
    for (int c = 0; c < 3; ++c) out_c[3 * v + c] = rep ? nerf_hs::mean_color(row[w + c], n) : 0.0f;
  }
}

// ---------------------------------------------------------------- faces

struct SameFace {
  const int32_t* faces;  // the remapped faces
  __device__ __forceinline__ bool operator()(int32_t a, int32_t b) const {
    int32_t ka[3], kb[3];
    nerf_hs::canonical(faces[3 * (int64_t)a], faces[3 * (int64_t)a + 1], faces[3 * (int64_t)a + 2], ka);
    nerf_hs::canonical(faces[3 * (int64_t)b], faces[3 * (int64_t)b + 1], faces[3 * (int64_t)b + 2], kb);
    return ka[0] == kb[0] && ka[1] == kb[1] && ka[2] == kb[2];
  }
};

__global__ __launch_bounds__(NTHREADS) void faces_remap_kernel(const int32_t* __restrict__ faces,
                                                               const int32_t* __restrict__ labels, int64_t F,
                                                               int32_t* __restrict__ out) {
  const int64_t f = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (f >= F) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[3 * f + c] = labels[faces[3 * f + c]];
}

__device__ __forceinline__ bool load_face(const int32_t* __restrict__ faces, int64_t f, int32_t k[3]) {
  const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
  nerf_hs::canonical(a, b, c, k);
  return a != b && b != c && a != c;
}

__global__ __launch_bounds__(NTHREADS) void faces_insert_kernel(const int32_t* __restrict__ faces, int64_t F,
                                                                int32_t* table, uint32_t mask,
                                                                int32_t* __restrict__ status) {
  const int64_t f = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  uint32_t probes = 0;
  bool ok = true;
  int32_t k[3];
  if (f < F && load_face(faces, f, k))
    ok = nerf_hs::insert(table, mask, nerf_hs::face_hash(k), (int32_t)f, SameFace{faces}, probes);
  report(status, ok, probes, 1);
}

__global__ __launch_bounds__(NTHREADS) void faces_lookup_kernel(const int32_t* __restrict__ faces, int64_t F,
                                                                const int32_t* __restrict__ table, uint32_t mask,
                                                                uint8_t* __restrict__ keep,
                                                                int32_t* __restrict__ status) {
  const int64_t f = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  uint32_t probes = 0;
  bool ok = true;
  int32_t k[3];
  if (f < F) {
    uint8_t kept = 0;
    if (load_face(faces, f, k)) {
      const int32_t first = nerf_hs::lookup(table, mask, nerf_hs::face_hash(k), (int32_t)f, SameFace{faces}, probes);
      ok = first >= 0;
      kept = first == (int32_t)f;
    }
    keep[f] = kept;
  }
  report(status, ok, probes, 2);
}

// ---------------------------------------------------------------- quadric placement

__global__ __launch_bounds__(NTHREADS) void cluster_quadric_kernel(
    const float* __restrict__ verts, const int32_t* __restrict__ faces, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ row_off, const int32_t* __restrict__ col, const float* __restrict__ mean, int64_t V,
    Grid g, double tol, float* __restrict__ out_pos, uint8_t* __restrict__ out_placed) {
  const int64_t v = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (v >= V) return;
  nerf_mq::place_vertex(verts, faces, labels, row_off, col, mean, g, tol, v, out_pos, out_placed);
}

bool sizes_ok(int64_t F, int64_t V) { return F >= 0 && V >= 0 && V < nerf_grid::LIMIT && 3 * F < nerf_grid::LIMIT; }

bool table_ok(int64_t items, int table_log2) {
  return table_log2 >= 0 && table_log2 <= 31 && (int64_t(1) << table_log2) > items;
}

int64_t round16(int64_t b) { return (b + 15) / 16 * 16; }

bool grid_ok(const float* lo, float cell, float inv, const int32_t* dims) {
  if (!lo || !dims || !(cell > 0.0f) || !(inv > 0.0f)) return false;
  for (int c = 0; c < 3; ++c)
    if (dims[c] < 1 || dims[c] > (1 << 20)) return false;
  return true;
}

int reduce_words(int has_normals, int has_colors) { return 3 * (1 + (has_normals ? 1 : 0) + (has_colors ? 1 : 0)); }

}  // namespace

extern "C" int64_t nerf_mesh_cluster_labels_workspace_bytes(int64_t V, int table_log2) {
  if (!sizes_ok(0, V) || !table_ok(V, table_log2)) return NERF_E_ARG;
  return round16(8 * V) + 4 * (int64_t(1) << table_log2);
}

extern "C" int nerf_mesh_cluster_labels(const float* vertices, int64_t V, const float* lo, float cell, float inv,
                                        const int32_t* dims, int table_log2, void* workspace, int64_t workspace_bytes,
                                        int32_t* labels, int32_t* status, hipStream_t stream) {
  NERF_CHECK_ARG(sizes_ok(0, V) && table_ok(V, table_log2) && grid_ok(lo, cell, inv, dims));
  NERF_CHECK_ARG(status != nullptr && (V == 0 || (vertices && labels && workspace)));
  if (V && !nerf_aligned16(workspace)) return NERF_E_ALIGN;
  if (V && workspace_bytes < nerf_mesh_cluster_labels_workspace_bytes(V, table_log2)) return NERF_E_WORKSPACE;
  hipError_t e = hipMemsetAsync(status, 0, 2 * sizeof(int32_t), stream);
  if (e != hipSuccess) return nerf_hip_status(e);
  if (V == 0) return NERF_OK;
  int64_t* keys = (int64_t*)workspace;
  int32_t* table = (int32_t*)((char*)workspace + round16(8 * V));
  const int64_t slots = int64_t(1) << table_log2;
  e = hipMemsetAsync(table, 0xff, 4 * slots, stream);  // EMPTY = -1
  if (e != hipSuccess) return nerf_hip_status(e);
  const Grid g = nerf_grid::fill_grid(lo, cell, inv, dims);
  const unsigned vb = (unsigned)nerf_cdiv(V, NTHREADS);
  const uint32_t mask = (uint32_t)(slots - 1);
  cluster_keys_kernel<<<vb, NTHREADS, 0, stream>>>(vertices, V, g, keys);
  cluster_insert_kernel<<<vb, NTHREADS, 0, stream>>>(keys, V, table, mask, status);
  cluster_lookup_kernel<<<vb, NTHREADS, 0, stream>>>(keys, V, table, mask, labels, status);
  return nerf_launch_status();
}

extern "C" int64_t nerf_mesh_cluster_reduce_workspace_bytes(int64_t V, int has_normals, int has_colors) {
  if (!sizes_ok(0, V)) return NERF_E_ARG;
  return round16(8 * V * reduce_words(has_normals, has_colors)) + round16(4 * V);
}

extern "C" int nerf_mesh_cluster_reduce(const float* vertices, const int32_t* labels, const float* normals,
                                        const float* colors, int64_t V, const float* lo, float cell, float inv,
                                        const int32_t* dims, void* workspace, int64_t workspace_bytes,
                                        float* out_vertices, float* out_normals, float* out_colors,
                                        hipStream_t stream) {
  NERF_CHECK_ARG(sizes_ok(0, V) && grid_ok(lo, cell, inv, dims));
  if (V == 0) return NERF_OK;
  NERF_CHECK_ARG(vertices && labels && workspace && out_vertices);
  NERF_CHECK_ARG((normals == nullptr) == (out_normals == nullptr) && (colors == nullptr) == (out_colors == nullptr));
  if (!nerf_aligned16(workspace)) return NERF_E_ALIGN;
  const int has_n = normals != nullptr, has_c = colors != nullptr;
  if (workspace_bytes < nerf_mesh_cluster_reduce_workspace_bytes(V, has_n, has_c)) return NERF_E_WORKSPACE;
  const int words = reduce_words(has_n, has_c);
  unsigned long long* acc = (unsigned long long*)workspace;
  int32_t* count = (int32_t*)((char*)workspace + round16(8 * V * words));
  const Grid g = nerf_grid::fill_grid(lo, cell, inv, dims);
  const unsigned vb = (unsigned)nerf_cdiv(V, NTHREADS);
  reduce_init_kernel<<<(unsigned)nerf_cdiv(V * words, NTHREADS), NTHREADS, 0, stream>>>(acc, V * words, count, V);
  reduce_accumulate_kernel<<<vb, NTHREADS, 0, stream>>>(vertices, labels, normals, colors, V, g, words, acc, count);
  reduce_finalize_kernel<<<vb, NTHREADS, 0, stream>>>(vertices, labels, V, g, words, has_n, has_c, acc, count,
                                                      out_vertices, out_normals, out_colors);
  return nerf_launch_status();
}

extern "C" int64_t nerf_mesh_cluster_faces_workspace_bytes(int64_t F, int table_log2) {
  if (!sizes_ok(F, 0) || !table_ok(F, table_log2)) return NERF_E_ARG;
  return 4 * (int64_t(1) << table_log2);
}

extern "C" int nerf_mesh_cluster_faces(const int32_t* faces, const int32_t* labels, int64_t F, int64_t V,
                                       int table_log2, void* workspace, int64_t workspace_bytes, int32_t* faces_out,
                                       uint8_t* keep, int32_t* status, hipStream_t stream) {
  NERF_CHECK_ARG(sizes_ok(F, V) && table_ok(F, table_log2));
  NERF_CHECK_ARG(status != nullptr && (F == 0 || (V > 0 && faces && labels && workspace && faces_out && keep)));
  NERF_CHECK_ARG(F == 0 || faces_out != faces);
  if (F && !nerf_aligned16(workspace)) return NERF_E_ALIGN;
  if (F && workspace_bytes < nerf_mesh_cluster_faces_workspace_bytes(F, table_log2)) return NERF_E_WORKSPACE;
  hipError_t e = hipMemsetAsync(status, 0, 2 * sizeof(int32_t), stream);
  if (e != hipSuccess) return nerf_hip_status(e);
  if (F == 0) return NERF_OK;
  int32_t* table = (int32_t*)workspace;
  const int64_t slots = int64_t(1) << table_log2;
  e = hipMemsetAsync(table, 0xff, 4 * slots, stream);  // EMPTY = -1
  if (e != hipSuccess) return nerf_hip_status(e);
  const unsigned fb = (unsigned)nerf_cdiv(F, NTHREADS);
  const uint32_t mask = (uint32_t)(slots - 1);
  faces_remap_kernel<<<fb, NTHREADS, 0, stream>>>(faces, labels, F, faces_out);
  faces_insert_kernel<<<fb, NTHREADS, 0, stream>>>(faces_out, F, table, mask, status);
  faces_lookup_kernel<<<fb, NTHREADS, 0, stream>>>(faces_out, F, table, mask, keep, status);
  return nerf_launch_status();
}

extern "C" int nerf_mesh_cluster_quadric(const float* vertices, const int32_t* faces, const int32_t* labels,
                                         const int32_t* row_off, const int32_t* col, const float* mean, int64_t V,
                                         int64_t F, const float* lo, float cell, float inv, const int32_t* dims,
                                         double tol, float* out_position, uint8_t* out_placed, hipStream_t stream) {
  NERF_CHECK_ARG(sizes_ok(F, V) && grid_ok(lo, cell, inv, dims));
  NERF_CHECK_ARG(tol > 0.0 && tol < 1.0);  // false for a NaN
  if (V == 0) return NERF_OK;
  NERF_CHECK_ARG(vertices && labels && row_off && mean && out_position && out_placed);  // col NULL: every row empty
  NERF_CHECK_ARG(F == 0 || faces);
  NERF_CHECK_ARG(out_position != mean && out_position != vertices);
  const Grid g = nerf_grid::fill_grid(lo, cell, inv, dims);
  cluster_quadric_kernel<<<(unsigned)nerf_cdiv(V, NTHREADS), NTHREADS, 0, stream>>>(
      vertices, faces, labels, row_off, col, mean, V, g, tol, out_position, out_placed);
  return nerf_launch_status();
}
