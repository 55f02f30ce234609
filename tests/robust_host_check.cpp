// The rank functions of the robust sounding gridder (csrc/sounding_rank.h) on the host, without HIP, against brute force: the MAD
// by bisection and by the merge walk, the ranks of the distances, the kept range and the sums over it, on segments of length 1 .. 4,
// of every length up to 200, all-equal, two-valued, at +-(2^31 - 65536) and random.  tests/test_host_soundings_rank.py compiles
// this with -fsanitize=address,undefined and runs it; it prints "ok <segments checked>" and returns 0, or says what differs.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../bathymetric-gnn_amd/csrc/sounding_rank.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t next_u64() {                                  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

const int64_t TOP = 2147483648ll - 65536;              // the widest quantised soundings
long long checked = 0;

int fail(const char *what, const std::vector<int32_t> &s, long long got, long long want) {
  std::fprintf(stderr, "%s: got %lld, want %lld on a segment of %zu:", what, got, want, s.size());
  for (size_t i = 0; i < s.size() && i < 12; ++i) std::fprintf(stderr, " %d", (int)s[i]);
  std::fprintf(stderr, "\n");
  return 1;
}

// one segment (sorted here) under the multipliers and floors below
int check(std::vector<int32_t> s) {
  std::sort(s.begin(), s.end());
  // the exact-size copy puts the sanitizer's red zones right at both ends of what the header may read
  std::vector<int32_t> exact(s);
  exact.shrink_to_fit();
  const int32_t *p = exact.data();
  const int64_t n = (int64_t)exact.size();
  const int64_t m2 = bgnn::seg_center2(p, n);
  if (m2 != (int64_t)s[(n - 1) / 2] + (int64_t)s[n / 2]) return fail("center2", s, m2, 0);
  std::vector<int64_t> d(n);
  for (int64_t i = 0; i < n; ++i) {
    d[i] = 2 * (int64_t)s[i] - m2;
    if (d[i] < 0) d[i] = -d[i];
    if (bgnn::seg_dist(s[i], m2) != d[i]) return fail("dist", s, bgnn::seg_dist(s[i], m2), d[i]);
  }
  std::vector<int64_t> ds(d);
  std::sort(ds.begin(), ds.end());
  const int64_t D = ds[(n - 1) / 2] + ds[n / 2];
  for (int64_t k : {(int64_t)0, (n - 1) / 2, n / 2, n - 1})
    if (bgnn::seg_dist_rank(p, n, m2, k) != ds[k]) return fail("dist_rank", s, bgnn::seg_dist_rank(p, n, m2, k), ds[k]);
  if (bgnn::seg_mad2_bisect(p, n, m2) != D) return fail("mad2_bisect", s, bgnn::seg_mad2_bisect(p, n, m2), D);
  if (bgnn::seg_mad2_walk(p, n, m2) != D) return fail("mad2_walk", s, bgnn::seg_mad2_walk(p, n, m2), D);
  const double ks[] = {1.0, 1.4826, 3 * 1.4826, 1e300};
  const double floors[] = {0.0, 0.05, 65536.0};
  for (double k : ks)
    for (double floor_m : floors) {
      const int64_t L = bgnn::robust_limit(D, k, floor_m);
      if (L < D / 2 || L > ((int64_t)1 << 34)) return fail("limit", s, L, D / 2);
      int64_t lo, hi;
      bgnn::seg_within(p, n, m2, L, &lo, &hi);
      int64_t kept = 0, first = -1, last = -1;
      bgnn::SegSums want = {0, 0, 0};
      for (int64_t i = 0; i < n; ++i)
        if (d[i] <= L) {
          if (first < 0) first = i;
          last = i;
          ++kept;
          const uint64_t q2 = (uint64_t)((int64_t)s[i] * (int64_t)s[i]);
          want.s1 += s[i]; want.s2_lo += q2 & 0xFFFFFFFFull; want.s2_hi += q2 >> 32;
        }
      if (kept != last - first + 1) return fail("kept soundings not contiguous", s, kept, last - first + 1);
      if (lo != first || hi != last + 1) return fail("kept range", s, lo * 1000000 + hi, first * 1000000 + last + 1);
      if (kept < (n - 1) / 2 + 1) return fail("kept below (n - 1) / 2 + 1", s, kept, (n - 1) / 2 + 1);
      if (floor_m >= 65536.0 && kept != n) return fail("a floor of 65536 m keeps all", s, kept, n);
      bgnn::SegSums got = {0, 0, 0};
      for (int64_t i = lo; i < hi; ++i) bgnn::seg_sums_add(&got, p[i]);
      if (got.s1 != want.s1 || got.s2_lo != want.s2_lo || got.s2_hi != want.s2_hi) return fail("sums", s, got.s1, want.s1);
    }
  ++checked;
  return 0;
}

int32_t draw(int kind) {
  const uint64_t r = next_u64();
  switch (kind) {
    case 0: return 12345;                                                      // all equal
    case 1: return (r & 1) ? -700000 : 900001;                                 // two values
    case 2: return (int32_t)((r & 1) ? TOP : -TOP);                            // the widest values
    case 3: return (int32_t)((int64_t)(r % (uint64_t)(2 * TOP + 1)) - TOP);    // anything
    case 4: return (int32_t)((int64_t)(r % 2001) - 1000 - 1638400);            // a seabed with ties
    default: return (int32_t)((r % 16 == 0) ? (int64_t)(r >> 8) % TOP : (int64_t)((r >> 8) % 5000) - 2500);   // a seabed with outliers
  }
}

}  // namespace

int main() {
  if (bgnn::floor_half(-3) != -2 || bgnn::ceil_half(-3) != -1 || bgnn::floor_half(3) != 1 || bgnn::ceil_half(3) != 2 ||
      bgnn::floor_half(-4) != -2 || bgnn::ceil_half(4) != 2)
    return 2;
  if (check({5}) || check({3, 4}) || check({-1, 0, 1}) || check({9, 9, 9, 10})) return 1;
  if (check({(int32_t)-TOP}) || check({(int32_t)-TOP, (int32_t)TOP}) || check({(int32_t)-TOP, (int32_t)-TOP, (int32_t)TOP})) return 1;
  for (int kind = 0; kind < 6; ++kind)
    for (int n = 1; n <= 200; ++n)
      for (int rep = 0; rep < (n <= 8 ? 40 : 2); ++rep) {
        std::vector<int32_t> s(n);
        for (int32_t &v : s) v = draw(kind);
        if (check(s)) return 1;
      }
  for (int n : {1000, 4097, 20001}) {
    std::vector<int32_t> s(n);
    for (int32_t &v : s) v = draw(5);
    if (check(s)) return 1;
  }
  std::printf("ok %lld\n", checked);
  return 0;
}
