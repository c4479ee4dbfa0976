// Vertex clustering: the cell of a vertex, the fixed-point quantisation of positions, normals and
// colours, and the lock-free hash set that finds the smallest item of every key, written once for the device and for
// a host compiler so that the loops can be run and checked under a host sanitizer without a GPU.
//
// The hash set: 2^k int32 slots, EMPTY = -1, linear probing with a mask.  A slot holds an item index (a vertex or a
// face); the slot's key is the key of that item, which the caller's `same(a, b)` compares through the indices.
// Invariants, at every instant and for every interleaving: a slot leaves EMPTY once, through a successful
// compare-and-swap, and never returns to it; afterwards only atomicMin writes to it, with items of the key it already
// holds, so a slot's key never changes and its value only decreases.  A key sits in at most one slot: a thread
// advances past a slot only after it has read a value of another key there, and never past an empty one.  Every
// access during the insert is a relaxed agent-scope atomic; the lookup runs in a later launch.
#pragma once
#include "mesh_grid_core.hpp"

#define NERF_HS_HD NERF_GRID_HD

namespace nerf_hs {

using nerf_grid::cell_index;
using nerf_grid::clampf;
using nerf_grid::Grid;

constexpr int32_t EMPTY = -1;

NERF_HS_HD int32_t load(const int32_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return __atomic_load_n(p, __ATOMIC_RELAXED);
#endif
}

// compare-and-swap; returns the value found (== expected iff it stored)
NERF_HS_HD int32_t cas(int32_t* p, int32_t expected, int32_t desired) {
#if defined(__HIP_DEVICE_COMPILE__)
  __hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
#else
  __atomic_compare_exchange_n(p, &expected, desired, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
#endif
  return expected;
}

NERF_HS_HD void fetch_min(int32_t* p, int32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  // a host compiler has no fetch-min: at most one round per smaller value stored in between, and those are finite
  int32_t cur = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (cur > v && !__atomic_compare_exchange_n(p, &cur, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
  }
#endif
}

// splitmix64 finaliser: the start slot of a key is its low bits
NERF_HS_HD uint64_t mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}

// Insert item v (>= 0) with hash h.  Returns false when `mask + 1` slots were probed without an end, which only a
// full table can cause (the callers keep 2^k > items, so one slot always stays empty).  A failed compare-and-swap
// returns the value that took the slot, and that very slot is examined with it: advancing instead would put one key
// into two slots.  atomicMin is applied only to a slot that was read non-empty.  Bound: mask + 1 probes.
template <class Same>
NERF_HS_HD bool insert(int32_t* table, uint32_t mask, uint64_t h, int32_t v, Same same, uint32_t& probes) {
  uint32_t s = (uint32_t)h & mask;
  for (uint32_t n = 0; n <= mask; ++n, s = (s + 1) & mask) {
    int32_t cur = load(table + s);
    if (cur == EMPTY) {
      cur = cas(table + s, EMPTY, v);
      if (cur == EMPTY) {
        probes = n + 1;
        return true;
      }
    }
    if (same(cur, v)) {  // cur may be stale under a racing atomicMin: it is still an item of the slot's key
      fetch_min(table + s, v);
      probes = n + 1;
      return true;
    }
  }
  probes = mask + 1;
  return false;
}

// The value of the slot that holds v's key, after every insert has finished (a later launch): the smallest item of
// that key.  Returns -1 when the key is not found (an empty slot on the way, or mask + 1 probes): v was not inserted.
template <class Same>
NERF_HS_HD int32_t lookup(const int32_t* table, uint32_t mask, uint64_t h, int32_t v, Same same, uint32_t& probes) {
  uint32_t s = (uint32_t)h & mask;
  for (uint32_t n = 0; n <= mask; ++n, s = (s + 1) & mask) {
    const int32_t cur = table[s];
    probes = n + 1;
    if (cur == EMPTY) return -1;
    if (same(cur, v)) return cur;
  }
  return -1;
}

// ---------------------------------------------------------------- the contract's arithmetic (build with
// -ffp-contract=off: every fp32 and fp64 operation below rounds on its own)

// the cell key of vertex v: nerf_grid::cell_id of its three cell indices (dims up to 2^20 here, so up to 2^60)
NERF_HS_HD int64_t cell_key(const Grid& g, const float* v) {
  return nerf_grid::cell_id(g, cell_index(g, 0, v[0]), cell_index(g, 1, v[1]), cell_index(g, 2, v[2]));
}

// the position inside the cell in 24-bit fixed point, 0 .. 2^24
NERF_HS_HD uint32_t quant_pos(const Grid& g, int c, float x) {
  const float t = nerf_grid::cell_coord(g, c, x);
  return (uint32_t)(clampf(t - (float)cell_index(g, c, x), 0.0f, 1.0f) * 16777216.0f);
}

NERF_HS_HD int64_t quant_normal(float n) { return (int64_t)rintf(clampf(n, -1.0f, 1.0f) * 1048576.0f); }

NERF_HS_HD uint32_t quant_color(float c) { return (uint32_t)rintf(clampf(c, 0.0f, 1.0f) * 16777216.0f); }

NERF_HS_HD float mean_pos(const Grid& g, int c, int32_t i, uint64_t sum, int32_t n) {
  const double frac = (double)sum / ((double)n * 16777216.0);
  const double cells = (double)i + frac;
  const double off = cells * (double)g.cell;
  return (float)((double)g.lo[c] + off);
}

NERF_HS_HD float mean_color(uint64_t sum, int32_t n) { return (float)((double)sum / ((double)n * 16777216.0)); }

NERF_HS_HD void unit_normal(const int64_t sum[3], float out[3]) {
  const double gx = (double)sum[0] / 1048576.0, gy = (double)sum[1] / 1048576.0, gz = (double)sum[2] / 1048576.0;
  const double xx = gx * gx, yy = gy * gy, zz = gz * gz;
  const double len = sqrt((xx + yy) + zz);
  const double d = len > 1e-12 ? len : 1e-12;
  out[0] = (float)(gx / d);
  out[1] = (float)(gy / d);
  out[2] = (float)(gz / d);
}

// ---------------------------------------------------------------- faces

// the rotation of (a, b, c) with the smallest index first; the cyclic order is kept
NERF_HS_HD void canonical(int32_t a, int32_t b, int32_t c, int32_t out[3]) {
  if (a <= b && a <= c) {
    out[0] = a, out[1] = b, out[2] = c;
  } else if (b <= a && b <= c) {
    out[0] = b, out[1] = c, out[2] = a;
  } else {
    out[0] = c, out[1] = a, out[2] = b;
  }
}

NERF_HS_HD uint64_t face_hash(const int32_t k[3]) {
  return mix(mix(((uint64_t)(uint32_t)k[0] << 32) | (uint32_t)k[1]) + (uint32_t)k[2]);
}

}  // namespace nerf_hs
