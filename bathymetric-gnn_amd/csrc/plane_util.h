// Helpers shared by the translation units that work on survey-sized planes and by the kernels that need a reproducible
// workgroup reduction: one definition each.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace bgnn {

constexpr int BLOCK_THREADS = 256;                    // the workgroup of block_reduce and of radix_select.h
constexpr int PLANE_MAX_GRID = 2048;                  // 256 CUs x 8 workgroups: the grid cap of the plane kernels that stride

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// the grid of a grid-stride pass over work_items chunks: at least one workgroup, at most cap
inline int capped_grid(int64_t work_items, int cap) { return (int)(work_items < 1 ? 1 : (work_items > cap ? cap : work_items)); }

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// A fixed halving tree over the 256 threads of a workgroup: s[t] = op(s[t], s[t + w]) for w = 128 .. 1.  The association is the
// contract: a float64 sum formed here has the same bits on every run.  Every thread calls it, every thread gets the result.
// scratch: 256 x sizeof(T) bytes of LDS.  LEAD: the barrier that lets the previous call's readers of scratch finish; only a
// caller whose scratch nobody has read yet may drop it.
template <bool LEAD = true, typename T, typename Op>
__device__ __forceinline__ T block_reduce(T v, void *scratch, Op op) {
  T *s = static_cast<T *>(scratch);
  const int t = threadIdx.x;
  if (LEAD) __syncthreads();
  s[t] = v;
  __syncthreads();
  for (int w = BLOCK_THREADS / 2; w > 0; w >>= 1) {
    if (t < w) s[t] = op(s[t], s[t + w]);
    __syncthreads();
  }
  return s[0];
}
struct SumOp {
  template <typename T>
  __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};

// The exclusive scan of one integer per thread over the workgroup; *total: the sum.  scratch: BLOCK_THREADS / 64 values of LDS,
// free again on return.  Every thread calls it.
template <typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T *scratch, T *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T up = __shfl_up(incl, o);
    if (lane >= o) incl += up;
  }
  __syncthreads();
  if (lane == 63) scratch[wave] = incl;
  __syncthreads();
  T before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < BLOCK_THREADS / 64; ++w) {
    const T c = scratch[w];
    before += w < wave ? c : 0;
    all += c;
  }
  *total = all;
  return before + incl - v;
}

// One workgroup: sums[] (one sum per tile of some tiled scan) becomes its own exclusive scan; the sum of it all goes to *total.
template <typename T, typename Total>
__global__ __launch_bounds__(BLOCK_THREADS) void scan_tile_sums(T *__restrict__ sums, int64_t n_tiles, Total *__restrict__ total) {
  __shared__ T scratch[BLOCK_THREADS / 64];
  T running = 0;
  for (int64_t base = 0; base < n_tiles; base += BLOCK_THREADS) {
    const int64_t i = base + threadIdx.x;
    const T v = i < n_tiles ? sums[i] : 0;
    T all;
    const T before = block_exclusive_scan(v, scratch, &all);
    if (i < n_tiles) sums[i] = running + before;
    running += all;
  }
  if (threadIdx.x == 0) *total = (Total)running;
}

}  // namespace bgnn
