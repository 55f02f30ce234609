// Connected-component labelling (4-connectivity, scipy.ndimage.label's default structure) of a mask over a survey-sized plane, for
// noise_analysis.hip, review_regions.hip and slope_features.hip.  Label equivalence by union-find over int32 cell indices:
// parent[i] = -1 off the mask, else the index of another cell of the same component or i itself (a root).  Three launches:
//
//   the caller's own local kernel   a 16 x 64 tile in LDS: the caller computes its mask, then tile_label() unites every cell of the
//                   mask with its left and upper neighbour inside the tile and counts the cells per tile-local root, and
//                   tile_write() stores every cell's parent (the global index of its tile-local root, -1 off the mask) and size
//                   (0 but at tile-local roots).  What else rides along (sums, bounds, column counts) is the caller's
//   label_merge     every cell of the mask in the first row / column of a tile unites with its neighbour across the border
//   label_flatten   every tile-local root that is not a global root points at its root and adds its aggregate to the root's: integer
//                   atomics, at most one set per tile-local component, not per cell; the components of up to 64 tiles that hang under
//                   one root are combined in a wave first
// launch_merge_flatten() enqueues the last two.  Afterwards parent[i] is at most two hops from the root and the aggregates at the
// roots (parent[i] == i) are complete.
//
// Termination, by construction.  Invariant: parent[i] <= i for every cell of the mask, at all times.  It holds after
// initialisation (parent[i] = i, or the tile-local root, the smallest index of the component in the tile, in row-major order both
// locally and globally), and the only later writes are atomicMin(&parent[a], b) with b < a and, in label_flatten,
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
// A consequence every user relies on: the root of a finished component is its smallest cell index, its first cell in row-major
// order, so "ascending by root" is the order scipy.ndimage.label numbers the components.
//
// What label_flatten needs.  (1) Merges complete: it is a launch of its own after label_merge on the same stream.  (2) Roots stable:
// it unites nothing, and its only write to parent re-points a cell that is not a root at its root, so find_root gives the same
// answer throughout.  (3) One writer class: only global roots' aggregates are added to, only other tile-local roots' aggregates are
// read, and a cell is one or the other for the whole launch.  Every aggregate is an integer add, minimum or maximum: the result
// does not depend on the order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "plane_util.h"

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

// ---- geometry ------------------------------------------------------------------------------------------------------------------
constexpr int TILE_R = 16, TILE_C = 64;               // the tile of a local kernel: 1024 cells, four per thread
constexpr int TILE_CELLS = TILE_R * TILE_C, TILE_PER = TILE_CELLS / BLOCK_THREADS;

struct TileGrid {
  int32_t rows, cols, tiles_r, tiles_c;
  TileGrid(int64_t r, int64_t c)
      : rows((int32_t)r), cols((int32_t)c), tiles_r((int32_t)((r + TILE_R - 1) / TILE_R)), tiles_c((int32_t)((c + TILE_C - 1) / TILE_C)) {}
  __host__ __device__ int64_t tiles() const { return (int64_t)tiles_r * tiles_c; }
  // The cells that have a neighbour across a tile border: (tiles_r - 1) * cols in the first rows of the lower tiles (upper
  // neighbour), then (tiles_c - 1) * rows in the first columns of the right-hand tiles (left neighbour).
  __host__ __device__ int64_t border_rows() const { return (int64_t)(tiles_r - 1) * cols; }
  __host__ __device__ int64_t borders() const { return border_rows() + (int64_t)(tiles_c - 1) * rows; }
  int local_grid() const { return capped_grid(tiles(), PLANE_MAX_GRID); }          // of a kernel that strides over the tiles
};

// ---- a tile in LDS ---------------------------------------------------------------------------------------------------------------
// Every thread of the workgroup calls these with the same tile.  Thread t has the cells l = k * BLOCK_THREADS + t, k < TILE_PER, of
// the tile in row-major order: one column, BLOCK_THREADS / TILE_C rows apart.
__device__ __forceinline__ int tile_cell(int k) { return k * BLOCK_THREADS + (int)threadIdx.x; }
__device__ __forceinline__ int64_t tile_to_global(const TileGrid &tg, int r0, int c0, int l) {
  return (int64_t)(r0 + l / TILE_C) * tg.cols + c0 + l % TILE_C;
}

// lp, lsize: TILE_CELLS words of LDS each that nobody reads any more (the caller's barrier after the previous tile).  in_mask[k]:
// the thread's cell k is on the mask (false outside the plane).  Returns root[k], the tile-local root of the thread's cell k (-1 off
// the mask), and leaves in lsize[r] the cells of every tile-local root r once the workgroup has passed its next barrier.
__device__ __forceinline__ void tile_label(const bool (&in_mask)[TILE_PER], int32_t *lp, int32_t *lsize, int32_t (&root)[TILE_PER]) {
#pragma unroll
  for (int k = 0; k < TILE_PER; ++k) {
    const int l = tile_cell(k);
    lp[l] = in_mask[k] ? l : -1;
    lsize[l] = 0;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < TILE_PER; ++k) {
    const int l = tile_cell(k);
    if (!in_mask[k]) continue;
    if (l % TILE_C > 0 && load_parent<false>(lp, l - 1) >= 0) unite<false>(lp, l, l - 1);
    if (l >= TILE_C && load_parent<false>(lp, l - TILE_C) >= 0) unite<false>(lp, l, l - TILE_C);
  }
  __syncthreads();
  // The thread's cells that share its first one's root go to LDS as one add, the others cell by cell.
  int32_t r_first = -1, n_first = 0;
#pragma unroll
  for (int k = 0; k < TILE_PER; ++k) {
    root[k] = in_mask[k] ? find_root<false>(lp, tile_cell(k)) : -1;
    if (!in_mask[k]) continue;
    if (r_first < 0) r_first = root[k];
    if (root[k] == r_first) n_first += 1;
    else atomicAdd(&lsize[root[k]], 1);
  }
  if (r_first >= 0) atomicAdd(&lsize[r_first], n_first);
}

// The barrier that completes lsize (and whatever the caller added to LDS arrays of its own since tile_label), then parent and size
// of the thread's cells inside the plane.  (r0, c0): the tile's first cell.
__device__ __forceinline__ void tile_write(const TileGrid &tg, int r0, int c0, const bool (&in_mask)[TILE_PER], const int32_t (&root)[TILE_PER],
                                           const int32_t *lsize, int32_t *__restrict__ parent, int32_t *__restrict__ size) {
  __syncthreads();
#pragma unroll
  for (int k = 0; k < TILE_PER; ++k) {
    const int l = tile_cell(k);
    if (r0 + l / TILE_C >= tg.rows || c0 + l % TILE_C >= tg.cols) continue;
    const int64_t i = tile_to_global(tg, r0, c0, l);
    parent[i] = in_mask[k] ? (int32_t)tile_to_global(tg, r0, c0, root[k]) : -1;
    size[i] = in_mask[k] && root[k] == l ? lsize[l] : 0;
  }
}

// ---- across the tiles --------------------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(BLOCK_THREADS) void label_merge(TileGrid tg, int32_t *parent) {
  const int64_t nh = tg.border_rows(), total = tg.borders();
  for (int64_t j = (int64_t)blockIdx.x * BLOCK_THREADS + threadIdx.x; j < total; j += (int64_t)gridDim.x * BLOCK_THREADS) {
    int64_t i, other;
    if (j < nh) {
      const int64_t r = (j / tg.cols + 1) * TILE_R, c = j % tg.cols;
      i = r * tg.cols + c;
      other = i - tg.cols;
    } else {
      const int64_t k = j - nh, c = (k / tg.rows + 1) * TILE_C, r = k % tg.rows;
      i = r * tg.cols + c;
      other = i - 1;
    }
    if (load_parent<true>(parent, (int32_t)i) >= 0 && load_parent<true>(parent, (int32_t)other) >= 0) unite<true>(parent, (int32_t)i, (int32_t)other);
  }
}

// What rides along with a component, indexed by cell: valid at tile-local roots after the local kernel, complete at global roots
// after label_flatten.  An aggregate is a struct of pointers with a member `int32_t *size` (positive at tile-local roots, 0
// elsewhere) and
//   Piece                  what one lane carries: the aggregate of one tile-local root
//   identity()             the piece that changes nothing
//   load(i)                the piece at the tile-local root i
//   combine(g, w)          g = g with the piece of lane ^ w (one level of the __shfl_xor tree; every lane of the wave calls it)
//   add_to_root(r, g)      integer atomics onto the global root r
struct SizeOnly {
  int32_t *size;
  using Piece = int32_t;
  __device__ static Piece identity() { return 0; }
  __device__ Piece load(int32_t i) const { return size[i]; }
  __device__ static void combine(Piece &g, int w) { g += __shfl_xor(g, w); }
  __device__ void add_to_root(int32_t r, Piece g) const { atomicAdd(size + r, g); }
};

// A workgroup takes 4096 consecutive cells at a time -- in a tile's first row that is the first cells of 64 tiles -- and lists the
// tile-local roots among them in LDS (in any order: every later step is an integer add, minimum or maximum).  Then a wave takes 64
// of the list: the pieces that hang under one root are combined in the wave (shuffles) and one lane adds them to that root.  Where a
// component covers many tiles this is one set of global atomics per 64 tiles, not 64 on one address.  After FL_GROUPS roots the
// lanes still left add their own piece.  Preconditions: the head of the file.
constexpr int FL_ITEMS = 16, FL_CHUNK = BLOCK_THREADS * FL_ITEMS, FL_GROUPS = 4;

template <typename Agg>
static __global__ __launch_bounds__(BLOCK_THREADS) void label_flatten(int64_t cells, int32_t *parent, Agg ag) {
  using Piece = typename Agg::Piece;
  __shared__ int32_t cand[FL_CHUNK];
  __shared__ int32_t n_cand;
  const int t = threadIdx.x, lane = t & 63;
  const int64_t chunks = (cells + FL_CHUNK - 1) / FL_CHUNK;
  for (int64_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
    __syncthreads();                                            // (the previous list is consumed)
    if (t == 0) n_cand = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < FL_ITEMS; ++k) {
      const int64_t i = chunk * FL_CHUNK + k * BLOCK_THREADS + t;
      // size > 0: a tile-local root.  At a global root the load races with other workgroups' atomicAdd, hence the atomic load;
      // the value there is positive and only grows, so the test comes out the same whichever value it sees.
      if (i < cells && __hip_atomic_load(ag.size + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > 0) cand[atomicAdd(&n_cand, 1)] = (int32_t)i;
    }
    __syncthreads();
    const int n = n_cand;
    for (int j0 = 0; j0 < n; j0 += BLOCK_THREADS) {             // (the same trips for every thread of the workgroup)
      const int j = j0 + t;
      int32_t root = -1;
      Piece piece = Agg::identity();
      bool todo = false;
      if (j < n) {
        const int32_t i = cand[j];
        root = find_root<true>(parent, i);
        todo = root != i;
        if (todo) {
          __hip_atomic_store(parent + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          piece = ag.load(i);                                   // (not a global root: nobody adds to it)
        }
      }
      for (int group = 0;; ++group) {                           // (the same trips for every lane of the wave)
        const unsigned long long left = __ballot(todo);
        if (left == 0ull) break;
        const bool own = group == FL_GROUPS;                    // every lane for itself
        const int leader = __ffsll((long long)left) - 1;
        const int32_t r = own ? root : __shfl(root, leader);
        const bool mine = todo && root == r;
        Piece g = mine ? piece : Agg::identity();
        if (!own) {
#pragma unroll
          for (int w = 32; w > 0; w >>= 1) Agg::combine(g, w);
        }
        if (own ? todo : lane == leader) ag.add_to_root(r, g);
        if (own) break;
        todo = todo && !mine;
      }
    }
  }
}

// label_merge and label_flatten on the stream, after the caller's local kernel
template <typename Agg>
inline void launch_merge_flatten(hipStream_t stream, const TileGrid &tg, int32_t *parent, Agg ag) {
  const int64_t cells = (int64_t)tg.rows * tg.cols;
  const int g_merge = capped_grid((tg.borders() + BLOCK_THREADS - 1) / BLOCK_THREADS, PLANE_MAX_GRID);
  const int g_flatten = capped_grid((cells + FL_CHUNK - 1) / FL_CHUNK, PLANE_MAX_GRID);
  hipLaunchKernelGGL(label_merge, dim3(g_merge), dim3(BLOCK_THREADS), 0, stream, tg, parent);
  hipLaunchKernelGGL(label_flatten<Agg>, dim3(g_flatten), dim3(BLOCK_THREADS), 0, stream, cells, parent, ag);
}

}  // namespace bgnn
