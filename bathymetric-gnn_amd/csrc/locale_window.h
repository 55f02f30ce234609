// The locale estimate of one cell (include/bgnn_locale.h): the two middle order statistics of the witness values inside a window of
// a halo image, by counting.  One definition for the device pass (locale_guide.hip calls it on LDS) and for the host check
// (tests/locale_host_check.cpp compiles this header alone, with a host compiler).  Integers only but for the one conversion of
// locale_guide_bits.
//
// The image holds one int64 per cell: a witness's value (twice its median in units of 2^-17 m, |v| < 2^32) or LOCALE_NO_WITNESS.
// The window is the rows r0 .. r1 and the columns c0 .. c1 of the image (both ends inside) without the entry at `self`.  With
// w[0 .. k) the witness values of the window in ascending order, med2 = w[(k - 1) / 2] + w[k / 2]:
//   - one pass counts k and takes the least and the greatest value;
//   - a bisection between the two finds a = w[(k - 1) / 2], the least x with (k - 1) / 2 + 1 values <= x: one counting pass per
//     step, 33 steps at the most for values of the contract (64 for any int64: the midpoint is formed without overflow, so the
//     loop ends whatever the image holds);
//   - one pass more counts the values <= a and takes the least value above a: w[k / 2] is a where the count reaches k / 2 + 1.
// No per-thread array, no order of the entries shows in the result.
#pragma once
#include <stdint.h>

#ifndef BGNN_SOUNDING_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define BGNN_SOUNDING_HD __host__ __device__
#else
#define BGNN_SOUNDING_HD
#endif
#endif

namespace bgnn {

constexpr int64_t LOCALE_NO_WITNESS = INT64_MAX;
constexpr uint32_t LOCALE_NAN_BITS = 0x7FC00000u;

// a cell is a witness iff it has exactly one hypothesis and that one was chosen
BGNN_SOUNDING_HD inline int64_t locale_witness_value(int32_t n_hyp, int32_t chosen, int64_t center2) {
  return n_hyp == 1 && chosen == 0 ? center2 : LOCALE_NO_WITNESS;
}

// the values <= x in the window (no witness mark is: x is a witness value or lies between two)
BGNN_SOUNDING_HD inline int32_t locale_count_le(const int64_t *image, int stride, int r0, int r1, int c0, int c1, int self, int64_t x) {
  int32_t n = 0;
  for (int r = r0; r <= r1; ++r)
    for (int c = c0; c <= c1; ++c) {
      const int i = r * stride + c;
      n += i != self && image[i] <= x;
    }
  return n;
}

// The support k of the window; *med2 where k >= min_support (min_support >= 1), untouched otherwise.
BGNN_SOUNDING_HD inline int32_t locale_window(const int64_t *image, int stride, int r0, int r1, int c0, int c1, int self,
                                              int32_t min_support, int64_t *med2) {
  int32_t k = 0;
  int64_t lo = INT64_MAX, hi = INT64_MIN;
  for (int r = r0; r <= r1; ++r)
    for (int c = c0; c <= c1; ++c) {
      const int i = r * stride + c;
      const int64_t v = image[i];
      if (i == self || v == LOCALE_NO_WITNESS) continue;
      ++k;
      lo = v < lo ? v : lo;
      hi = v > hi ? v : hi;
    }
  if (k < min_support) return k;
  const int32_t need = (k - 1) / 2 + 1;
  while (lo < hi) {
    const int64_t mid = lo + (int64_t)(((uint64_t)hi - (uint64_t)lo) >> 1);
    if (locale_count_le(image, stride, r0, r1, c0, c1, self, mid) >= need) hi = mid;
    else lo = mid + 1;
  }
  const int64_t a = lo;
  int32_t le = 0;
  int64_t above = INT64_MAX;
  for (int r = r0; r <= r1; ++r)
    for (int c = c0; c <= c1; ++c) {
      const int i = r * stride + c;
      const int64_t v = image[i];
      if (i == self || v == LOCALE_NO_WITNESS) continue;
      le += v <= a;
      above = v > a && v < above ? v : above;
    }
  const int64_t b = le >= k / 2 + 1 ? a : above;
  *med2 = (int64_t)((uint64_t)a + (uint64_t)b);        // |med2| < 2^33 for values of the contract
  return k;
}

// the bits of the guide: (float)((double)med2 * 2^-18), one rounding, or the quiet NaN where the support falls short
BGNN_SOUNDING_HD inline uint32_t locale_guide_bits(int32_t k, int32_t min_support, int64_t med2) {
  if (k < min_support) return LOCALE_NAN_BITS;
  const float g = (float)((double)med2 * (1.0 / 262144.0));
  uint32_t bits;
  __builtin_memcpy(&bits, &g, 4);
  return bits;
}

}  // namespace bgnn
