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

}  // namespace bgnn
