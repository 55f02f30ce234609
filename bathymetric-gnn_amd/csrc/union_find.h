// Label equivalence by union-find over int32 cell indices, shared by the connected-component kernels of noise_analysis.hip and
// review_regions.hip: parent[i] = -1 off the mask, else the index of another cell of the same component or i itself (a root).
//
// Termination, by construction.  Invariant: parent[i] <= i for every cell of the mask, at all times.  It holds after
// initialisation (parent[i] = i, or the tile-local root, the smallest index of the component in the tile, in row-major order both
// locally and globally), and the only later writes are atomicMin(&parent[a], b) with b < a and, in the flatten kernels,
// parent[i] = root <= i.
//   find(x)   follows parent while parent[x] != x: each step strictly lowers x, so it ends after at most x steps whatever other
//             threads write meanwhile (a stale read only makes it stop at an older ancestor; the atomicMin below detects that).
//   unite(a, b)   a = find(a), b = find(b); equal: done.  Otherwise, with a > b: old = atomicMin(&parent[a], b).  old == a: a was
//             still a root and now points at b: done.  Otherwise another thread lowered parent[a] to old < a first; whichever of
//             old and b stayed in parent[a], the pair (old, b) still has to be united: continue with a = old.  Every iteration
//             replaces the larger of two non-negative indices by a strictly smaller one, so a + b strictly decreases: the loop ends.
// No thread waits for another: there is no spin-wait on a flag or a workgroup, no grid-wide barrier and no persistent kernel; a
// workgroup's progress never depends on another workgroup being scheduled.
//
// A consequence both users rely on: the root of a finished component is its smallest cell index, its first cell in row-major order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bgnn {

// GLOBAL: the parent array is in global memory and other workgroups lower it meanwhile: device-scope loads.  Else: LDS.
template <bool GLOBAL>
__device__ __forceinline__ int32_t load_parent(const int32_t *p, int32_t x) {
  return GLOBAL ? __hip_atomic_load(p + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                : __hip_atomic_load(p + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <bool GLOBAL>
__device__ __forceinline__ int32_t find_root(const int32_t *p, int32_t x) {
  for (;;) {                                                    // parent[x] <= x: every step strictly lowers x
    const int32_t q = load_parent<GLOBAL>(p, x);
    if (q == x) return x;
    x = q;
  }
}
template <bool GLOBAL>
__device__ __forceinline__ void unite(int32_t *p, int32_t a, int32_t b) {
  for (;;) {                                                    // a + b strictly decreases: see the head of the file
    a = find_root<GLOBAL>(p, a);
    b = find_root<GLOBAL>(p, b);
    if (a == b) return;
    if (a < b) { const int32_t s = a; a = b; b = s; }
    const int32_t old = atomicMin(p + a, b);
    if (old == a) return;
    a = old;
  }
}

}  // namespace bgnn
