// Reading the robust statistics off one sorted segment of quantised soundings (include/bgnn_soundings_robust.h): one definition
// for the device passes and for the host check (tests/robust_host_check.cpp compiles this header alone, with a host compiler).
// Everything is an integer but the rejection limit, which is float64 operation by operation (-ffp-contract=off).
//
// s[0 .. n) is ascending, n >= 1, |s_i| < 2^31.  m2 = s[(n-1)/2] + s[n/2] is twice the median; d_i = |2 s_i - m2| < 2^33.
// The d of a sorted segment fall into two sorted runs, the ones left of the median read backwards and the ones right of it, so
//   - a rank of d is the head of a merge walked outwards from the median (seg_mad2_walk: n / 2 + 1 steps, for short segments), or
//   - the smallest t with count(d <= t) above the rank, the count being two binary searches (seg_mad2_bisect: 34 halvings of t).
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef BGNN_SOUNDING_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define BGNN_SOUNDING_HD __host__ __device__
#else
#define BGNN_SOUNDING_HD
#endif
#endif

namespace bgnn {

// floor(v / 2) and ceil(v / 2), also below zero
BGNN_SOUNDING_HD inline int64_t floor_half(int64_t v) { return (v - (v & 1)) / 2; }
BGNN_SOUNDING_HD inline int64_t ceil_half(int64_t v) { return (v + (v & 1)) / 2; }

// the first index whose value is >= v (lower) or > v (upper); n where there is none
BGNN_SOUNDING_HD inline int64_t seg_lower_bound(const int32_t *s, int64_t n, int64_t v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if ((int64_t)s[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}
BGNN_SOUNDING_HD inline int64_t seg_upper_bound(const int32_t *s, int64_t n, int64_t v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if ((int64_t)s[mid] <= v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

BGNN_SOUNDING_HD inline int64_t seg_center2(const int32_t *s, int64_t n) { return (int64_t)s[(n - 1) / 2] + (int64_t)s[n / 2]; }

BGNN_SOUNDING_HD inline int64_t seg_dist(int32_t q, int64_t m2) {
  const int64_t d = 2 * (int64_t)q - m2;
  return d < 0 ? -d : d;
}

// the soundings with d <= t: [*lo, *hi) of the segment (t >= 0; t < 0 gives an empty range)
BGNN_SOUNDING_HD inline void seg_within(const int32_t *s, int64_t n, int64_t m2, int64_t t, int64_t *lo, int64_t *hi) {
  *lo = seg_lower_bound(s, n, ceil_half(m2 - t));
  *hi = seg_upper_bound(s, n, floor_half(m2 + t));
  if (*hi < *lo) *hi = *lo;
}

// the k-th smallest d (k from 0): the smallest t at which k + 1 soundings lie within t
BGNN_SOUNDING_HD inline int64_t seg_dist_rank(const int32_t *s, int64_t n, int64_t m2, int64_t k) {
  const int64_t d0 = seg_dist(s[0], m2), d1 = seg_dist(s[n - 1], m2);
  int64_t lo = 0, hi = d0 > d1 ? d0 : d1;             // the largest d: every sounding lies within it
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    int64_t a, b;
    seg_within(s, n, m2, mid, &a, &b);
    if (b - a >= k + 1) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// D = d_((n-1)/2) + d_(n/2) over the sorted d: twice the MAD of the doubled distances
BGNN_SOUNDING_HD inline int64_t seg_mad2_bisect(const int32_t *s, int64_t n, int64_t m2) {
  const int64_t a = seg_dist_rank(s, n, m2, (n - 1) / 2);
  return (n & 1) ? 2 * a : a + seg_dist_rank(s, n, m2, n / 2);
}
BGNN_SOUNDING_HD inline int64_t seg_mad2_walk(const int32_t *s, int64_t n, int64_t m2) {
  const int64_t k1 = (n - 1) / 2, k2 = n / 2, never = INT64_MAX;
  int64_t l = (n - 1) / 2, r = l + 1, D = 0;          // the next candidate on either side of the median
  for (int64_t step = 0; step <= k2; ++step) {        // (k2 <= n - 1: one side always has a candidate)
    const int64_t dl = l >= 0 ? m2 - 2 * (int64_t)s[l] : never, dr = r < n ? 2 * (int64_t)s[r] - m2 : never;
    int64_t d;
    if (dl <= dr) { d = dl; --l; } else { d = dr; ++r; }
    if (step == k1) D += d;
    if (step == k2) D += d;
  }
  return D;
}

// L = floor(min(max(k * (D / 2), floor_m * 2^17), 2^34)): a sounding is kept iff d <= L
BGNN_SOUNDING_HD inline int64_t robust_limit(int64_t D, double k, double floor_m) {
  const double a = k * ((double)D * 0.5), b = floor_m * 131072.0;
  const double td = a > b ? a : b;
  const double cap = 17179869184.0;                   // 2^34, above every d
  return (int64_t)floor(td < cap ? td : cap);
}

// what the mean and the standard deviation of a range are formed from: S1 = sum q, S2 = s2_hi * 2^32 + s2_lo = sum q^2
struct SegSums {
  int64_t s1;
  uint64_t s2_lo, s2_hi;
};
BGNN_SOUNDING_HD inline void seg_sums_add(SegSums *a, int32_t q) {
  const uint64_t q2 = (uint64_t)((int64_t)q * (int64_t)q);
  a->s1 += q;
  a->s2_lo += q2 & 0xFFFFFFFFull;
  a->s2_hi += q2 >> 32;
}

}  // namespace bgnn
