// Texture baking for meshes on the device (the shared core is mesh_texture_core.hpp).
//
//   nerf_mesh_atlas_texels    one thread per texel of the T x T atlas, x fastest: the owning face, the barycentric
//                             pair, the surface point and (optionally) the normal the texel stands for.
//   nerf_mesh_texture_lookup  one thread per (face, barycentric pair): the bilinear fetch of a (T,T,C) texture at the
//                             face's own UV, C channels.
//
// The atlas is a function of (F, S): there is no UV array, both kernels compute the layout.  Neighbouring threads of
// the texel kernel write neighbouring texels, so each of its four store streams is contiguous per wave; the three
// corners of a face are read by the S^2 / 2 threads of its half cell, from the caches after the first.  No LDS, no
// atomics: every output element has one writer and is a function of the input alone.  The kernels do not check the
// vertex indices: that is the caller's duty (kernels.py validates before launching); the lookup's reads stay inside the
// texture for any face and pair.
#include "common.hpp"
#include "mesh_texture_core.hpp"

namespace {

constexpr int NTHREADS = 256;
constexpr int64_t LIMIT = (int64_t)1 << 31;

__global__ __launch_bounds__(NTHREADS) void atlas_texels_kernel(nerf_mt::Atlas A, const float* __restrict__ verts,
                                                                const int32_t* __restrict__ faces,
                                                                const float* __restrict__ vertex_normals,
                                                                int32_t* __restrict__ face, float* __restrict__ bary,
                                                                float* __restrict__ position,
                                                                float* __restrict__ normal) {
  const int64_t p = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (p >= (int64_t)A.T * A.T) return;
  nerf_mt::texel(A, verts, faces, vertex_normals, p, face, bary, position, normal);
}

template <int C>
__global__ __launch_bounds__(NTHREADS) void texture_lookup_kernel(nerf_mt::Atlas A, const float* __restrict__ texture,
                                                                  const int32_t* __restrict__ face,
                                                                  const float* __restrict__ bary, int64_t N,
                                                                  float* __restrict__ out) {
  const int64_t n = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (n >= N) return;
  nerf_mt::lookup(A, texture, C, face, bary, n, out);
}

}  // namespace

extern "C" int nerf_mesh_atlas_texels(const float* vertices, const int32_t* faces, int64_t F, int texels, int T,
                                      const float* vertex_normals, int32_t* face, float* bary, float* position,
                                      float* normal, hipStream_t stream) {
  nerf_mt::Atlas A;
  NERF_CHECK_ARG(F >= 0 && 3 * F < LIMIT && nerf_mt::make_atlas(F, texels, A) && A.T == T);
  NERF_CHECK_ARG(face && bary && position && (F == 0 || (vertices && faces)) && (normal || !vertex_normals));
  const int64_t P = (int64_t)A.T * A.T;  // at most 2^28
  atlas_texels_kernel<<<(unsigned)nerf_cdiv(P, NTHREADS), NTHREADS, 0, stream>>>(A, vertices, faces, vertex_normals,
                                                                                 face, bary, position, normal);
  return nerf_launch_status();
}

extern "C" int nerf_mesh_texture_lookup(const float* texture, int T, int C, int64_t F, int texels, const int32_t* face,
                                        const float* bary, int64_t N, float* out, hipStream_t stream) {
  nerf_mt::Atlas A;
  NERF_CHECK_ARG(F >= 0 && 3 * F < LIMIT && nerf_mt::make_atlas(F, texels, A) && A.T == T && C >= 1 && C <= 4 &&
                 N >= 0 && N < LIMIT);
  if (N == 0) return NERF_OK;
  NERF_CHECK_ARG(texture && face && bary && out);
  const unsigned blocks = (unsigned)nerf_cdiv(N, NTHREADS);
  switch (C) {
    case 1: texture_lookup_kernel<1><<<blocks, NTHREADS, 0, stream>>>(A, texture, face, bary, N, out); break;
    case 2: texture_lookup_kernel<2><<<blocks, NTHREADS, 0, stream>>>(A, texture, face, bary, N, out); break;
    case 3: texture_lookup_kernel<3><<<blocks, NTHREADS, 0, stream>>>(A, texture, face, bary, N, out); break;
    default: texture_lookup_kernel<4><<<blocks, NTHREADS, 0, stream>>>(A, texture, face, bary, N, out); break;
  }
  return nerf_launch_status();
}
