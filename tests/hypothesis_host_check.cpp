// The segment logic of the depth hypotheses (csrc/sounding_hypothesis.h) on the host, without HIP, against brute force: the walk,
// and the share summaries stitched in order (256, 7, 4 and 1 shares), with their records, on segments of every length 1 .. 600,
// with breaks at every position for lengths up to 12, with breaks exactly on, one before and one after every share boundary, all
// one run, every sounding its own run, values at +-(2^31 - 65536), and every tie of both keys, under both rules.
// tests/test_host_hypothesis_walk.py compiles this with -fsanitize=address,undefined and runs it; it prints
// "ok <segments checked>" and returns 0, or says what differs.
#include <algorithm>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../bathymetric-gnn_amd/csrc/sounding_hypothesis.h"

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

struct Want {
  int64_t n_hyp, h, a, b;
  std::vector<int64_t> first, count;
};

// the contract, written out: the runs, then the smallest (k0, k1, h)
Want brute(const std::vector<int32_t> &s, int64_t gap_q, int64_t min_count, bool by_guide, int64_t ref2) {
  Want w;
  const int64_t n = (int64_t)s.size();
  int64_t a = 0;
  for (int64_t i = 1; i <= n; ++i)
    if (i == n || (int64_t)s[i] - (int64_t)s[i - 1] > gap_q) {
      w.first.push_back(a);
      w.count.push_back(i - a);
      a = i;
    }
  w.n_hyp = (int64_t)w.first.size();
  w.h = -1; w.a = w.b = 0;
  int64_t b0 = 0, b1 = 0;
  for (int64_t h = 0; h < w.n_hyp; ++h) {
    const int64_t nh = w.count[h], f = w.first[h];
    if (nh < min_count) continue;
    const int64_t m2 = (int64_t)s[f + (nh - 1) / 2] + (int64_t)s[f + nh / 2];
    const int64_t d = std::llabs(m2 - ref2);
    const int64_t k0 = by_guide ? d : -nh, k1 = by_guide ? -nh : d;
    if (w.h < 0 || k0 < b0 || (k0 == b0 && k1 < b1)) {             // (ascending h: a tie keeps the lower index)
      w.h = h; w.a = f; w.b = f + nh; b0 = k0; b1 = k1;
    }
  }
  return w;
}

int fail(const char *what, const std::vector<int32_t> &s, long long got, long long want, long long extra) {
  std::fprintf(stderr, "%s (%lld): got %lld, want %lld on a segment of %zu:", what, extra, got, want, s.size());
  for (size_t i = 0; i < s.size() && i < 16; ++i) std::fprintf(stderr, " %d", (int)s[i]);
  std::fprintf(stderr, "\n");
  return 1;
}

int compare(const char *what, const std::vector<int32_t> &s, const Want &w, int64_t n_hyp, const bgnn::HypPick &p,
            const std::vector<uint32_t> &first, const std::vector<int32_t> &count, uint32_t base, long long extra) {
  if (n_hyp != w.n_hyp) return fail(what, s, n_hyp, w.n_hyp, extra);
  if (p.h != w.h) return fail(what, s, p.h, w.h, extra);
  if (w.h >= 0 && (p.a != w.a || p.b != w.b)) return fail(what, s, p.a * 100000 + p.b, w.a * 100000 + w.b, extra);
  for (int64_t h = 0; h < w.n_hyp; ++h)
    if ((int64_t)first[h] != w.first[h] + base || count[h] != w.count[h]) return fail(what, s, first[h], w.first[h] + base, h);
  return 0;
}

// one ascending segment under one gap: both rules, several min_count, the walk and the stitched shares
int check(std::vector<int32_t> s, int64_t gap_q, float guide = 0.0f) {
  std::sort(s.begin(), s.end());
  std::vector<int32_t> exact(s);                       // (an exact-size copy: the sanitizer's red zones sit at both ends)
  exact.shrink_to_fit();
  const int32_t *p = exact.data();
  const int64_t n = (int64_t)exact.size();
  const uint32_t base = 1000;
  for (int by_guide = 0; by_guide < 2; ++by_guide)
    for (int64_t min_count : {(int64_t)1, (int64_t)2, (int64_t)3, n, n + 1}) {
      const bgnn::HypRule r = bgnn::hyp_rule_of(p, n, gap_q, min_count, by_guide != 0, guide);
      int64_t g2 = 0;
      const bool usable = by_guide && bgnn::hyp_guide2(guide, &g2);
      const int64_t ref2 = usable ? g2 : (int64_t)s[(n - 1) / 2] + (int64_t)s[n / 2];
      if (r.ref2 != ref2 || (r.by_guide != 0) != usable) return fail("rule", s, r.ref2, ref2, by_guide);
      const Want w = brute(s, gap_q, min_count, usable, ref2);
      if (bgnn::hyp_count_breaks(p, 1, n, 1, gap_q) + 1 != w.n_hyp) return fail("count_breaks", s, 0, w.n_hyp, 1);
      int64_t strided = 0;
      for (int t = 0; t < 256; ++t) strided += bgnn::hyp_count_breaks(p, 1 + t, n, 256, gap_q);
      if (strided + 1 != w.n_hyp) return fail("count_breaks strided", s, strided + 1, w.n_hyp, 256);
      {
        std::vector<uint32_t> first((size_t)n);
        std::vector<int32_t> count((size_t)n);
        bgnn::HypPick pick;
        const int64_t got = bgnn::hyp_walk(p, n, r, &pick, first.data(), count.data(), base);
        if (compare("walk", s, w, got, pick, first, count, base, min_count)) return 1;
        bgnn::HypPick bare;
        if (bgnn::hyp_walk(p, n, r, &bare, nullptr, nullptr, 0) != got || bare.h != pick.h) return fail("walk, no records", s, bare.h, pick.h, 0);
      }
      for (int n_chunks : {256, 7, 4, 1}) {
        const int64_t len = (n + n_chunks - 1) / n_chunks;
        std::vector<bgnn::HypChunk> chunks((size_t)n_chunks);
        for (int t = 0; t < n_chunks; ++t) chunks[t] = bgnn::hyp_chunk_scan(p, t * len, std::min(n, t * len + len), r);
        std::vector<uint32_t> first((size_t)n, 0xFFFFFFFFu);
        std::vector<int32_t> count((size_t)n, -1);
        bgnn::HypPick pick;
        const int64_t got = bgnn::hyp_stitch(p, n, chunks.data(), n_chunks, r, &pick, first.data(), count.data(), base);
        for (int t = 0; t < n_chunks; ++t) bgnn::hyp_chunk_records(p, gap_q, chunks[t], first.data(), count.data(), base);
        if (compare("stitch", s, w, got, pick, first, count, base, n_chunks)) return 1;
        for (int64_t h = w.n_hyp; h < n; ++h)
          if (first[h] != 0xFFFFFFFFu || count[h] != -1) return fail("a record past the last run", s, h, w.n_hyp, n_chunks);
      }
    }
  ++checked;
  return 0;
}

int32_t draw(int kind) {
  const uint64_t r = next_u64();
  switch (kind) {
    case 0: return 12345;                                                      // all equal: one run at any gap
    case 1: return (r & 1) ? -700000 : 900001;                                 // two values
    case 2: return (int32_t)((r & 1) ? TOP : -TOP);                            // the widest values: a difference of 2^32 - 2^17
    case 3: return (int32_t)((int64_t)(r % (uint64_t)(2 * TOP + 1)) - TOP);    // anything
    case 4: return (int32_t)((int64_t)(r % 2001) - 1000 - 1638400);            // a seabed with ties
    default: return (int32_t)((r % 3 == 0) ? -1310720 + (int64_t)((r >> 8) % 9000) : -2293760 + (int64_t)((r >> 8) % 9000));   // two surfaces
  }
}

// a segment of n with a break (under a gap of 5) before exactly the positions given
std::vector<int32_t> with_breaks(int64_t n, const std::vector<int64_t> &at) {
  std::vector<int32_t> s((size_t)n);
  int32_t v = -5000;
  for (int64_t i = 0; i < n; ++i) {
    if (i > 0) v += std::find(at.begin(), at.end(), i) != at.end() ? 10 : (int32_t)(next_u64() % 6);     // steps of 0 .. 5 inside a run
    s[(size_t)i] = v;
  }
  return s;
}

}  // namespace

int main() {
  int64_t g2 = 0;
  if (bgnn::hyp_guide2(std::nanf(""), &g2) || bgnn::hyp_guide2(INFINITY, &g2) || bgnn::hyp_guide2(-INFINITY, &g2) ||
      bgnn::hyp_guide2(32768.0f, &g2) || bgnn::hyp_guide2(-32768.0f, &g2) || bgnn::hyp_guide2(1.0e6f, &g2))
    return 2;
  if (!bgnn::hyp_guide2(-32767.998f, &g2) || g2 != 2 * (int64_t)std::llrint((double)-32767.998f * 65536.0)) return 2;
  if (!bgnn::hyp_guide2(0.5f, &g2) || g2 != 65536) return 2;

  // the ties, written out: -2, -1 | 1, 2 m is symmetric about the cell's median, both keys tie and the lower index wins
  const int32_t M = 65536;
  if (check({-2 * M, -1 * M, 1 * M, 2 * M}, M)) return 1;
  {
    const std::vector<int32_t> s = {-2 * M, -1 * M, 1 * M, 2 * M};
    const Want w = brute(s, M, 1, false, 0);
    if (w.n_hyp != 2 || w.h != 0 || w.a != 0 || w.b != 2) return fail("symmetric cell", s, w.h, 0, 0);
  }
  // equal counts, the second run nearer to the cell's median
  if (check({-40 * M, -39 * M, -10 * M, -9 * M, -8 * M, 20 * M, 21 * M, 22 * M, 23 * M, 30 * M, 31 * M, 32 * M, 33 * M}, 2 * M)) return 1;
  // a guide exactly halfway between two runs: the larger count wins, whichever side it is on
  if (check({-30 * M, -30 * M, -30 * M, -20 * M, -20 * M}, M, -25.0f) || check({-30 * M, -30 * M, -20 * M, -20 * M, -20 * M}, M, -25.0f)) return 1;
  if (check({-30 * M, -30 * M, -20 * M, -20 * M}, M, -25.0f)) return 1;                   // and with equal counts the lower index
  // both signs at the widest values: one run at 2^32, two below the difference
  for (int64_t gap : {(int64_t)4294967296ll, 2 * TOP, 2 * TOP - 1, (int64_t)0})
    if (check({(int32_t)-TOP, (int32_t)-TOP, (int32_t)TOP}, gap) || check({(int32_t)-TOP, (int32_t)TOP}, gap, 40000.0f)) return 1;
  if (check({5}, 0) || check({5, 5}, 0) || check({5, 6}, 0) || check({5, 6}, 1)) return 1;

  // every length 1 .. 600: each kind at a gap that cuts it somewhere and at the two ends of the range
  for (int kind = 0; kind < 6; ++kind)
    for (int n = 1; n <= 600; ++n) {
      std::vector<int32_t> s((size_t)n);
      for (int32_t &v : s) v = draw(kind);
      const int64_t gaps[] = {0, 3, 4000, 4294967296ll};
      if (check(s, gaps[(n + kind) % 4], kind == 5 ? -20.3f : -25.0f)) return 1;
    }
  // every sounding its own run (distinct values, gap 0) and all one run
  for (int n : {1, 2, 255, 256, 257, 511, 512, 513, 600}) {
    std::vector<int32_t> s((size_t)n);
    for (int i = 0; i < n; ++i) s[(size_t)i] = -1000 + 3 * i;
    if (check(s, 0) || check(s, 2) || check(s, 3) || check(s, 4294967296ll)) return 1;
  }
  // breaks at every set of positions for lengths up to 12
  for (int n = 1; n <= 12; ++n)
    for (uint32_t mask = 0; mask < (1u << (n - 1)); ++mask) {
      std::vector<int64_t> at;
      for (int i = 1; i < n; ++i)
        if (mask & (1u << (i - 1))) at.push_back(i);
      if (check(with_breaks(n, at), 5, -0.07f)) return 1;
    }
  // breaks exactly on, one before and one after every share boundary, alone and with a second break elsewhere
  for (int n : {257, 300, 512, 513, 600})
    for (int n_chunks : {256, 7, 4}) {
      const int64_t len = (n + n_chunks - 1) / n_chunks;
      for (int64_t edge = len; edge < n; edge += len)
        for (int64_t d = -1; d <= 1; ++d) {
          const int64_t at = edge + d;
          if (at < 1 || at >= n) continue;
          if (n_chunks == 256 && n > 300 && edge % (7 * len) != 0) continue;              // (a seventh of them is enough there)
          if (check(with_breaks(n, {at}), 5) || check(with_breaks(n, {at, 1}), 5) || check(with_breaks(n, {at, (int64_t)n - 1}), 5) ||
              check(with_breaks(n, {at, at + len}), 5))
            return 1;
        }
    }
  std::printf("ok %lld\n", checked);
  return 0;
}
