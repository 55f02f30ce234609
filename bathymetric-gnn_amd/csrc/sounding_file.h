// Filing a sounding under a cell of a sounding state (include/bgnn_soundings.h), and which counter a sounding enters: one
// definition for the uniform gridders (sounding_grid.hip, sounding_robust.hip) and the variable-resolution ones (sounding_vr.hip).
#pragma once
#include "plane_util.h"
#include "../../include/bgnn_soundings.h"

namespace bgnn {

struct SoundingCell {
  long long s1;                                       // sum q
  unsigned long long s2_lo, s2_hi;                    // sum (q^2 & 0xFFFFFFFF), sum (q^2 >> 32): S2 = s2_hi * 2^32 + s2_lo
  uint32_t n, min_inv, max_key, pad;                  // min_inv: the largest ~key, the key of the minimum inverted
};
static_assert(sizeof(SoundingCell) == BGNN_SOUNDINGS_CELL_BYTES, "the cell the header documents");

__device__ __forceinline__ bool finite_bits64(double v) {
  return (__double_as_longlong(v) & 0x7FF0000000000000LL) != 0x7FF0000000000000LL;
}

// float32 onto uint32, order-preserving for every non-NaN value (-0.0 below +0.0)
__device__ __forceinline__ uint32_t order_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float order_value(uint32_t key) {
  return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}

// Which counter a sounding enters: the first four in the order of the state's header, SOUNDING_UNREFINED beside them (a layout
// with refinement grids only; the uniform grids pass refined = true).
enum SoundingKind { SOUNDING_ACCEPTED = 0, SOUNDING_NONFINITE = 1, SOUNDING_OUTSIDE = 2, SOUNDING_OUT_OF_RANGE = 3, SOUNDING_UNREFINED = 4 };
constexpr int SOUNDING_KINDS = 5;

// checked in this order, exactly one each: nonfinite, outside, unrefined, out of range, accepted
__device__ __forceinline__ int sounding_kind(double x, double y, float z, bool on_grid, bool refined) {
  if (!(finite_bits64(x) && finite_bits64(y) && finite_bits(z))) return SOUNDING_NONFINITE;
  if (!on_grid) return SOUNDING_OUTSIDE;
  if (!refined) return SOUNDING_UNREFINED;
  if (!(fabsf(z) < (float)BGNN_SOUNDINGS_Z_CAP)) return SOUNDING_OUT_OF_RANGE;
  return SOUNDING_ACCEPTED;
}

__device__ __forceinline__ long long sounding_q(float z) {
  return llrint((double)z * (double)BGNN_SOUNDINGS_SCALE);                           // |q| < 2^31 for an accepted sounding
}

// One sounding per lane into its cell; every lane of the wave calls this.
__device__ __forceinline__ void file_sounding(SoundingCell *cells, bool ok, int64_t cell, float z) {
  const long long q = ok ? sounding_q(z) : 0;
  const unsigned long long q2 = (unsigned long long)(q * q);                         // < 2^62
  const uint32_t key = order_key(z);
  uint32_t cnt = 1, lo_inv = ~key, hi_key = key;
  unsigned long long s1 = (unsigned long long)q, s2_lo = q2 & 0xFFFFFFFFull, s2_hi = q2 >> 32;
  // a run of neighbouring lanes on one cell is summed towards its first lane, which alone goes to memory
  const int lane = threadIdx.x & 63;
  const int64_t mine = ok ? cell : (int64_t)-1 - lane;                               // (a rejected lane merges with nobody)
  const int64_t prev = __shfl_up(mine, 1);
  const bool head = ok && (lane == 0 || prev != mine);
  const unsigned long long starts = __ballot(lane == 0 || prev != mine);             // every run start, rejected lanes included
  if (starts != ~0ull) {                                                             // (wave-uniform) some run is longer than one lane
    const unsigned long long after = lane == 63 ? 0ull : starts >> (lane + 1);
    const int room = after ? __ffsll((long long)after) : 64 - lane;                  // lanes from this one to the end of its run
    int longest = room;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) longest = max(longest, __shfl_xor(longest, o));
    for (int d = 1; d < longest; d <<= 1) {                                          // (wave-uniform trip count)
      const uint32_t c2 = __shfl_down(cnt, d), l2 = __shfl_down(lo_inv, d), h2 = __shfl_down(hi_key, d);
      const unsigned long long a2 = __shfl_down(s1, d), b2 = __shfl_down(s2_lo, d), e2 = __shfl_down(s2_hi, d);
      if (d < room) {                                                                // lane + d lies in this lane's run
        cnt += c2; s1 += a2; s2_lo += b2; s2_hi += e2;
        lo_inv = max(lo_inv, l2); hi_key = max(hi_key, h2);
      }
    }
  }
  if (head) {
    SoundingCell *c = cells + cell;
    atomicAdd(&c->n, cnt);
    atomicAdd(reinterpret_cast<unsigned long long *>(&c->s1), s1);
    atomicAdd(&c->s2_lo, s2_lo);
    atomicAdd(&c->s2_hi, s2_hi);
    atomicMax(&c->min_inv, lo_inv);
    atomicMax(&c->max_key, hi_key);
  }
}

}  // namespace bgnn
