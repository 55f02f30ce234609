// Depth hypotheses of one sorted segment of quantised soundings (include/bgnn_hypotheses.h): one definition for the device passes
// (sounding_hypotheses.hip) and for the host check (tests/hypothesis_host_check.cpp compiles this header alone, with a host
// compiler).  Integers only.
//
// s[0 .. n) is ascending.  A break sits before i (1 <= i < n) iff (int64)s[i] - (int64)s[i - 1] > gap_q; hypothesis h is the h-th
// maximal run [a, b) without a break, m2 = s[a + (nh - 1) / 2] + s[a + nh / 2] twice its median, nh = b - a.  Among the runs with
// nh >= min_count the smallest key wins, (-nh, |m2 - ref2|, h) by count and (|m2 - ref2|, -nh, h) by guide; the runs are always
// offered in ascending h, so the comparison of the first two parts is strict and h needs no place in the key.
//   - hyp_walk: one pass over a segment, for the short class (one thread) and as the plain statement of the rule;
//   - hyp_chunk_scan / hyp_stitch / hyp_chunk_records: the same result from contiguous shares of the segment, one summary per
//     share and one stitch of the summaries in order, for the long class (one workgroup).
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

struct HypRule {
  int64_t gap_q, min_count, ref2;                      // ref2: twice the cell's median (by count) or twice the guide (by guide)
  int32_t by_guide;
};
struct HypKey {
  int64_t k0, k1;
};
struct HypPick {                                       // the best run so far: h = -1 where there is none
  int64_t h, a, b;
  HypKey key;
};
// what one contiguous share [lo, hi) of the break positions holds
struct HypChunk {
  int64_t first, last, breaks;                         // its first and last break (-1: none) and how many it has
  HypPick inner;                                       // the best run between two of its breaks; h counts from its first break
  int64_t open_at, h_at;                               // from the stitch: where the run begins that is open at lo, and its index
};

BGNN_SOUNDING_HD inline bool hyp_break(const int32_t *s, int64_t i, int64_t gap_q) { return (int64_t)s[i] - (int64_t)s[i - 1] > gap_q; }

// twice the guide in units of 2^-17 m; false where the guide cannot be used (not finite, or |g| >= 32768) and the count rule holds
BGNN_SOUNDING_HD inline bool hyp_guide2(float g, int64_t *g2) {
  const double d = (double)g;
  if (!(fabs(d) < 32768.0)) return false;
  *g2 = 2 * (int64_t)llrint(d * 65536.0);
  return true;
}

// the rule of one cell: s its segment, n >= 1; guide: whether the call is by guide, g the cell's value then
BGNN_SOUNDING_HD inline HypRule hyp_rule_of(const int32_t *s, int64_t n, int64_t gap_q, int64_t min_count, bool guide, float g) {
  HypRule r;
  r.gap_q = gap_q;
  r.min_count = min_count;
  r.by_guide = guide && hyp_guide2(g, &r.ref2);
  if (!r.by_guide) r.ref2 = (int64_t)s[(n - 1) / 2] + (int64_t)s[n / 2];
  return r;
}

BGNN_SOUNDING_HD inline int64_t hyp_m2(const int32_t *s, int64_t a, int64_t b) {
  const int64_t nh = b - a;
  return (int64_t)s[a + (nh - 1) / 2] + (int64_t)s[a + nh / 2];
}

// run [a, b) with index h against the best so far
BGNN_SOUNDING_HD inline void hyp_offer(HypPick *p, const HypRule &r, const int32_t *s, int64_t a, int64_t b, int64_t h) {
  const int64_t nh = b - a;
  if (nh < r.min_count) return;
  int64_t d = hyp_m2(s, a, b) - r.ref2;                // below 2^34 either way
  if (d < 0) d = -d;
  HypKey k;
  k.k0 = r.by_guide ? d : -nh;
  k.k1 = r.by_guide ? -nh : d;
  if (p->h < 0 || k.k0 < p->key.k0 || (k.k0 == p->key.k0 && k.k1 < p->key.k1)) {
    p->h = h; p->a = a; p->b = b; p->key = k;
  }
}

// the breaks at lo, lo + step, .. below hi (lo >= 1)
BGNN_SOUNDING_HD inline int64_t hyp_count_breaks(const int32_t *s, int64_t lo, int64_t hi, int64_t step, int64_t gap_q) {
  int64_t breaks = 0;
  for (int64_t i = lo; i < hi; i += step) breaks += hyp_break(s, i, gap_q);
  return breaks;
}

// One pass over s[0 .. n), n >= 1: the number of runs; *pick the chosen one; where rec_first is given, run h goes into
// rec_first[h] = base + a and rec_count[h] = b - a.
BGNN_SOUNDING_HD inline int64_t hyp_walk(const int32_t *s, int64_t n, const HypRule &r, HypPick *pick, uint32_t *rec_first,
                                         int32_t *rec_count, uint32_t base) {
  pick->h = -1; pick->a = pick->b = 0; pick->key.k0 = pick->key.k1 = 0;
  int64_t a = 0, h = 0;
  for (int64_t i = 1; i <= n; ++i) {
    if (i < n && !hyp_break(s, i, r.gap_q)) continue;
    hyp_offer(pick, r, s, a, i, h);
    if (rec_first) {
      rec_first[h] = base + (uint32_t)a;
      rec_count[h] = (int32_t)(i - a);
    }
    a = i;
    ++h;
  }
  return h;
}

// the share [lo, hi) of the positions 0 .. n - 1 (position 0 is never a break)
BGNN_SOUNDING_HD inline HypChunk hyp_chunk_scan(const int32_t *s, int64_t lo, int64_t hi, const HypRule &r) {
  HypChunk c;
  c.first = c.last = -1; c.breaks = 0; c.open_at = c.h_at = 0;
  c.inner.h = -1; c.inner.a = c.inner.b = 0; c.inner.key.k0 = c.inner.key.k1 = 0;
  for (int64_t i = lo < 1 ? 1 : lo; i < hi; ++i) {
    if (!hyp_break(s, i, r.gap_q)) continue;
    if (c.first < 0) c.first = i;
    else hyp_offer(&c.inner, r, s, c.last, i, c.breaks - 1);
    c.last = i;
    ++c.breaks;
  }
  return c;
}

// The summaries of the shares in order, over s[0 .. n), n >= 1: the number of runs, *pick the chosen one; every share learns the
// run that is open where it begins (open_at, h_at).  The last run goes into the records where they are given.
BGNN_SOUNDING_HD inline int64_t hyp_stitch(const int32_t *s, int64_t n, HypChunk *chunks, int n_chunks, const HypRule &r, HypPick *pick,
                                           uint32_t *rec_first, int32_t *rec_count, uint32_t base) {
  pick->h = -1; pick->a = pick->b = 0; pick->key.k0 = pick->key.k1 = 0;
  int64_t open = 0, h = 0;
  for (int t = 0; t < n_chunks; ++t) {
    HypChunk &c = chunks[t];
    c.open_at = open;
    c.h_at = h;
    if (c.breaks == 0) continue;
    hyp_offer(pick, r, s, open, c.first, h);
    ++h;
    if (c.inner.h >= 0) {                              // (one comparison stands for all of the share's inner runs, the lowest index first)
      HypPick in = c.inner;
      const HypKey k = in.key;
      if (pick->h < 0 || k.k0 < pick->key.k0 || (k.k0 == pick->key.k0 && k.k1 < pick->key.k1)) {
        in.h += h;
        *pick = in;
      }
    }
    h += c.breaks - 1;
    open = c.last;
  }
  hyp_offer(pick, r, s, open, n, h);
  if (rec_first) {
    rec_first[h] = base + (uint32_t)open;
    rec_count[h] = (int32_t)(n - open);
  }
  return h + 1;
}

// the records of the runs that end at a break of a share, after the stitch
BGNN_SOUNDING_HD inline void hyp_chunk_records(const int32_t *s, int64_t gap_q, const HypChunk &c, uint32_t *rec_first,
                                               int32_t *rec_count, uint32_t base) {
  if (c.breaks == 0) return;
  int64_t a = c.open_at, h = c.h_at;
  for (int64_t i = c.first; i <= c.last; ++i) {        // (the first and the last are breaks: nothing to ask)
    if (i > c.first && i < c.last && !hyp_break(s, i, gap_q)) continue;
    rec_first[h] = base + (uint32_t)a;
    rec_count[h] = (int32_t)(i - a);
    a = i;
    ++h;
  }
}

}  // namespace bgnn
