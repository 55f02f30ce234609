// The mean and the standard deviation of n quantised soundings from their exact integer sums (include/bgnn_soundings.h): one
// definition for the streaming gridder (sounding_grid.hip) and for the kept soundings of the robust one (sounding_robust.hip).
// Device code, compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bgnn {

// the exact integer v rounded once, half to even, to float64
__device__ __forceinline__ double u128_to_double(unsigned __int128 v) {
  const unsigned long long hi = (unsigned long long)(v >> 64), lo = (unsigned long long)v;
  if (hi == 0) return (double)lo;
  const int shift = 64 - __clzll((long long)hi);                                     // 1 .. 64: the bits above the top 64
  unsigned long long top = (unsigned long long)(v >> shift);
  const unsigned long long below = shift == 64 ? lo : (lo & ((1ull << shift) - 1));
  top |= below != 0;                                  // sticky: bit 0 lies under the rounding position of a 64-bit value
  return ldexp((double)top, shift);
}

// (float)((double)S1 / (double)n * 2^-16)
__device__ __forceinline__ float sounding_mean(uint32_t n, long long s1) {
  const double unscale = 1.0 / 65536.0;                                              // exact
  return (float)((double)s1 / (double)n * unscale);
}

// (float)(sqrt((double)(n * S2 - S1^2) / ((double)n * (double)n)) * 2^-16), S2 = s2_hi * 2^32 + s2_lo: the numerator is formed
// exactly in 128 bits and rounded once to float64
__device__ __forceinline__ float sounding_std(uint32_t n, long long s1, unsigned long long s2_lo, unsigned long long s2_hi) {
  const double unscale = 1.0 / 65536.0, dn = (double)n;
  const unsigned __int128 s2 = ((unsigned __int128)s2_hi << 32) + s2_lo;
  const unsigned long long a1 = (unsigned long long)(s1 < 0 ? -s1 : s1);
  const unsigned __int128 num = (unsigned __int128)n * s2 - (unsigned __int128)a1 * a1;            // >= 0 (Cauchy-Schwarz), < 2^124
  return (float)(sqrt(u128_to_double(num) / (dn * dn)) * unscale);
}

}  // namespace bgnn
