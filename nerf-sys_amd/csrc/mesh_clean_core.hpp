// Lock-free union-find over a parent array: the per-face work of nerf_mesh_components
// (mesh_clean.hip), written once for the device and for a host compiler so that the loops can be run and checked under
// a host sanitizer without a GPU.
//
// Invariant, at every instant and for every interleaving: parent[v] <= v, and parent[v] is v itself (v is a root) or a
// vertex that was an ancestor of v when it was stored, so a vertex of v's set.  The links strictly decrease, so there
// are no cycles and a root is the smallest vertex of its tree.  A root stops being one only through a successful
// compare-and-swap, and never becomes one again.
//
// Every access to parent is a relaxed agent-scope atomic (sc1 loads and stores on gfx950: they bypass the vector L1,
// which another CU's stores never refresh).  Correctness does not need a load to be fresh: an old value is still an
// ancestor.  Only the compare-and-swap decides, and its return value is the word's true content.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NERF_UF_HD __host__ __device__ __forceinline__
#else
#define NERF_UF_HD inline
#endif

namespace nerf_uf {

NERF_UF_HD int32_t load(const int32_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return __atomic_load_n(p, __ATOMIC_RELAXED);
#endif
}

NERF_UF_HD void store(int32_t* p, int32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  __atomic_store_n(p, v, __ATOMIC_RELAXED);
#endif
}

// compare-and-swap; returns the value found (== expected iff it stored)
NERF_UF_HD int32_t cas(int32_t* p, int32_t expected, int32_t desired) {
#if defined(__HIP_DEVICE_COMPILE__)
  __hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
#else
  __atomic_compare_exchange_n(p, &expected, desired, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
#endif
  return expected;
}

// The root of v, shortening the path by halving: parent[v] = grandparent, a value that is already an ancestor, stored
// only over a non-root word (parent[v] != v was read, and a non-root never becomes a root again), so it never undoes a
// union.  Bound: every step moves to a strictly smaller vertex, whatever other threads store, so the loop body runs
// at most v times; `steps` counts them against `budget` and the function returns -1 when the budget
// is spent, which only a broken invariant can cause.
template <bool SHORTEN>
NERF_UF_HD int32_t find(int32_t* parent, int32_t v, uint32_t budget, uint32_t& steps) {
  int32_t p = load(parent + v);
  while (p != v) {
    if (++steps > budget) return -1;
    const int32_t g = load(parent + p);
    if (SHORTEN && g != p) store(parent + v, g);
    v = p;
    p = g;
  }
  return v;
}

// Unite the sets of a and b; returns a vertex of the united set (the root it found, or a common ancestor), or -1 when
// a bound is exhausted.  First a shortcut: equal parent words mean a common ancestor, so the two are united already,
// and the root's own word, which every thread of a large component would read, is not touched.  Then the loop: find
// both roots; equal -> done; else compare-and-swap the larger root's word from itself to the smaller root; it fails
// only when another thread's compare-and-swap on that word succeeded in between (that root was hooked elsewhere), and
// then the search goes on from the value the failed operation returned.  No thread waits for another thread's store.
// Bound: a failed compare-and-swap proves one successful union by another thread, and V vertices allow at most V - 1
// successful unions, so the loop body runs at most V times; the finds inside share one step budget of 2 V per call
// (each of the two walks is a descending chain of at most V vertices in total, because a retry continues downwards
// from where the last walk ended).
NERF_UF_HD int32_t unite(int32_t* parent, int32_t a, int32_t b, int32_t V, uint32_t& total_steps) {
  if (a == b) return a;
  {
    const int32_t pa = load(parent + a), pb = load(parent + b);
    if (pa == pb) return pa;
  }
  const uint32_t budget = 2u * (uint32_t)V;  // V < 2^31
  uint32_t steps = 0;
  for (int32_t tries = 0; tries < V; ++tries) {
    a = find<true>(parent, a, budget, steps);
    b = find<true>(parent, b, budget, steps);
    if (a < 0 || b < 0) return -1;
    if (a == b) {
      total_steps += steps;
      return a;
    }
    if (a < b) {
      const int32_t t = a;
      a = b;
      b = t;
    }
    const int32_t seen = cas(parent + a, a, b);  // a > b
    if (seen == a) {
      total_steps += steps;
      return b;
    }
    a = seen;  // a's true parent: an ancestor, so the next find continues from there
  }
  return -1;
}

// One face: two unions join its three vertices (the third pair follows); the second starts from the vertex the first
// returned, which is as far up the tree as this thread has been.  Repeated indices unite a vertex with itself.
NERF_UF_HD bool unite_face(int32_t* parent, const int32_t* face, int32_t V, uint32_t& steps) {
  const int32_t r = unite(parent, face[0], face[1], V, steps);
  if (r < 0) return false;
  return unite(parent, r, face[2], V, steps) >= 0;
}

}  // namespace nerf_uf
