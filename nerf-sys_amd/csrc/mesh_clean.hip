// Mesh clean-up on the device: connected components of an indexed triangle list, and the compaction
// of a mesh to a subset of its faces.
//
//   nerf_mesh_components  labels[v] = smallest vertex index of v's component, face_count[l] = faces of component l.
//     1. init      one thread per vertex: parent[v] = v, face_count[v] = 0.
//     2. unite     one thread per face: lock-free union-find (mesh_clean_core.hpp), compare-and-swap on roots only.
//     3. flatten   one thread per vertex: parent[v] = root(v), in place (a vertex's word has this one writer now; a
//                  reader meets the old ancestor or the root, and both lead to the root).  parent is now `labels`.
//     4. count     face_count[labels[face[0]]] += 1 for every face, aggregated per wave before the integer atomic (a
//                  one-component mesh would otherwise send every face of the mesh to one word).
//   The labels are a function of the input alone, so equal inputs give equal bits although the kernels use atomics;
//   integer atomics only.  status[0] != 0 reports a thread that exhausted a loop bound (the labels are then not to be
//   used); status[1] is the largest number of find steps one face's two unions took.
//
//   nerf_mesh_mark_used   one thread per face: keep32[f] = keep[f] != 0 (or keep[labels[face[0]]], a flag per
//                         component), and used[v] = 1 for the vertices of a kept face (many threads store the same 1;
//                         nothing else is written to `used`, zeroed by the caller).
//   nerf_mesh_remap_faces one thread per face: a kept face goes to row face_pos[f] with its indices renumbered by
//                         vert_pos (the exclusive scans of keep32 and used), so faces and vertices keep their order.
//   The vertex rows and attributes follow by nerf_flag_compact + nerf_gather_rows.  Every output slot has one writer.
//
// The kernels do not check indices: 0 <= index < V is the caller's duty (kernels.py validates before launching).
#include "common.hpp"
#include "mesh_clean_core.hpp"

namespace {

constexpr int NTHREADS = 256;
constexpr int COUNT_ITERS = 16;  // runs of 64 faces per wave of the count pass

__global__ __launch_bounds__(NTHREADS) void uf_init_kernel(int32_t* __restrict__ parent,
                                                           int32_t* __restrict__ face_count, int32_t V) {
  const int64_t v = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (v >= V) return;
  parent[v] = (int32_t)v;
  face_count[v] = 0;
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)v, d, 64);
    v = o > v ? o : v;
  }
  return v;
}

__global__ __launch_bounds__(NTHREADS) void uf_unite_kernel(const int32_t* __restrict__ faces, int64_t F, int32_t V,
                                                            int32_t* parent, int32_t* __restrict__ status) {
  const int64_t f = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  uint32_t steps = 0;
  bool ok = true;
  if (f < F) {
    const int32_t face[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
    ok = nerf_uf::unite_face(parent, face, V, steps);
  }
  if (!ok) atomicOr(status, 1);
  steps = wave_max_u32(steps);  // every lane of the wave is here: no early return above
  if (nerf_lane() == 0 && steps) atomicMax(status + 1, (int32_t)(steps > 0x7fffffffu ? 0x7fffffffu : steps));
}

__global__ __launch_bounds__(NTHREADS) void uf_flatten_kernel(int32_t* parent, int32_t V,
                                                              int32_t* __restrict__ status) {
  const int64_t v = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (v >= V) return;
  uint32_t steps = 0;
  // at most v steps down a strictly descending chain; the budget V can only be spent on a broken invariant
  const int32_t r = nerf_uf::find<false>(parent, (int32_t)v, (uint32_t)V, steps);
  if (r < 0) {
    atomicOr(status, 2);
    return;
  }
  nerf_uf::store(parent + v, r);
}

__global__ __launch_bounds__(NTHREADS) void face_count_kernel(const int32_t* __restrict__ faces, int64_t F,
                                                              const int32_t* __restrict__ labels,
                                                              int32_t* __restrict__ face_count) {
  // A wave walks COUNT_ITERS runs of 64 consecutive faces and keeps one running (label, count) pair, wave-uniform: a
  // run whose faces all carry one label only grows the pair, and the extractor's face order keeps a component's faces
  // together, so a large component costs one add per 64 COUNT_ITERS faces, not one per wave instruction.
  const int64_t wave = ((int64_t)blockIdx.x * NTHREADS + threadIdx.x) / NERF_WAVE;
  const int lane = nerf_lane();
  int32_t cur = -1, run = 0;
  for (int it = 0; it < COUNT_ITERS; ++it) {
    const int64_t f = (wave * COUNT_ITERS + it) * NERF_WAVE + lane;
    bool todo = f < F;
    const int32_t l = todo ? labels[faces[3 * f]] : -1;
    unsigned long long pending = __ballot(todo);
    if (!pending) break;  // wave-uniform: the face list ended
    const int32_t first = __shfl(l, __ffsll((long long)pending) - 1, 64);
    if (__ballot(todo && l == first) == pending) {
      if (first != cur) {
        if (lane == 0 && run) atomicAdd(face_count + cur, run);
        cur = first;
        run = 0;
      }
      run += (int32_t)__popcll(pending);
      continue;
    }
    // mixed labels: one add per distinct label; every pass retires the first pending lane's group, so at most 64 passes
    for (int pass = 0; pass < NERF_WAVE && pending; ++pass) {
      const int leader = __ffsll((long long)pending) - 1;
      const int32_t ll = __shfl(l, leader, 64);
      const bool mine = todo && l == ll;
      const unsigned long long group = __ballot(mine);
      if (lane == leader) atomicAdd(face_count + ll, (int32_t)__popcll(group));
      if (mine) todo = false;
      pending = __ballot(todo);
    }
  }
  if (lane == 0 && run) atomicAdd(face_count + cur, run);
}

__global__ __launch_bounds__(NTHREADS) void mark_used_kernel(const int32_t* __restrict__ faces,
                                                             const uint8_t* __restrict__ keep,
                                                             const int32_t* __restrict__ labels, int64_t F,
                                                             int32_t* __restrict__ keep32, int32_t* __restrict__ used) {
  const int64_t f = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (f >= F) return;
  const bool k = keep[labels ? (int64_t)labels[faces[3 * f]] : f] != 0;  // per face, or per component label
  keep32[f] = k ? 1 : 0;
  if (k) {
    used[faces[3 * f]] = 1;
    used[faces[3 * f + 1]] = 1;
    used[faces[3 * f + 2]] = 1;
  }
}

__global__ __launch_bounds__(NTHREADS) void remap_faces_kernel(const int32_t* __restrict__ faces,
                                                               const int32_t* __restrict__ keep32,
                                                               const int32_t* __restrict__ face_pos,
                                                               const int32_t* __restrict__ vert_pos, int64_t F,
                                                               int64_t F_out, int32_t* __restrict__ out) {
  const int64_t f = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (f >= F || !keep32[f]) return;
  const int64_t o = face_pos[f];
  if (o >= F_out) return;  // F_out is the scan's total, so this never holds; it keeps a wrong total from writing past the output
  out[3 * o] = vert_pos[faces[3 * f]];
  out[3 * o + 1] = vert_pos[faces[3 * f + 1]];
  out[3 * o + 2] = vert_pos[faces[3 * f + 2]];
}

bool sizes_ok(int64_t F, int64_t V) { return F >= 0 && V >= 0 && V < (int64_t(1) << 31) && 3 * F < (int64_t(1) << 31); }

}  // namespace

extern "C" int nerf_mesh_components(const int32_t* faces, int64_t F, int64_t V, int32_t* labels, int32_t* face_count,
                                    int32_t* status, hipStream_t stream) {
  NERF_CHECK_ARG(sizes_ok(F, V));
  NERF_CHECK_ARG(status != nullptr);
  NERF_CHECK_ARG(F == 0 || V > 0);
  hipError_t e = hipMemsetAsync(status, 0, 2 * sizeof(int32_t), stream);
  if (e != hipSuccess) return nerf_hip_status(e);
  if (V == 0) return NERF_OK;
  NERF_CHECK_ARG(labels && face_count && (F == 0 || faces));
  const unsigned vb = (unsigned)nerf_cdiv(V, NTHREADS), fb = (unsigned)nerf_cdiv(F, NTHREADS);
  uf_init_kernel<<<vb, NTHREADS, 0, stream>>>(labels, face_count, (int32_t)V);
  if (F == 0) return nerf_launch_status();  // every vertex is its own component
  uf_unite_kernel<<<fb, NTHREADS, 0, stream>>>(faces, F, (int32_t)V, labels, status);
  uf_flatten_kernel<<<vb, NTHREADS, 0, stream>>>(labels, (int32_t)V, status);
  face_count_kernel<<<(unsigned)nerf_cdiv(F, (int64_t)NTHREADS * COUNT_ITERS), NTHREADS, 0, stream>>>(faces, F, labels,
                                                                                                       face_count);
  return nerf_launch_status();
}

extern "C" int nerf_mesh_mark_used(const int32_t* faces, const uint8_t* keep, const int32_t* labels, int64_t F,
                                   int64_t V, int32_t* keep32, int32_t* used, hipStream_t stream) {
  NERF_CHECK_ARG(sizes_ok(F, V));
  if (F == 0) return NERF_OK;
  NERF_CHECK_ARG(V > 0 && faces && keep && keep32 && used);
  mark_used_kernel<<<(unsigned)nerf_cdiv(F, NTHREADS), NTHREADS, 0, stream>>>(faces, keep, labels, F, keep32, used);
  return nerf_launch_status();
}

extern "C" int nerf_mesh_remap_faces(const int32_t* faces, const int32_t* keep32, const int32_t* face_pos,
                                     const int32_t* vert_pos, int64_t F, int64_t F_out, int32_t* out,
                                     hipStream_t stream) {
  NERF_CHECK_ARG(sizes_ok(F, 0) && F_out >= 0 && F_out <= F);
  if (F == 0 || F_out == 0) return NERF_OK;
  NERF_CHECK_ARG(faces && keep32 && face_pos && vert_pos && out);
  remap_faces_kernel<<<(unsigned)nerf_cdiv(F, NTHREADS), NTHREADS, 0, stream>>>(faces, keep32, face_pos, vert_pos, F,
                                                                                F_out, out);
  return nerf_launch_status();
}
