// Exact multi-rank radix selection over integer histograms: the one implementation behind the ground truth's median
// (ground_truth.hip: two ranks of a 32-bit key, int64 counts) and the analysis's order statistics (noise_analysis.hip: up to
// six ranks of a 32- or 64-bit key, uint32 counts).
//
// A key is cut into digits, most significant first (Digits<11, 11, 10>).  One level = one streaming pass that counts the level's
// digit of every key under a prefix fixed so far (DigitCounter, inside the caller's own streaming kernel), then one workgroup
// that walks the counts and narrows prefix and rank of every rank (select_digit, inside the caller's own kernel).  Ranks whose
// keys share the prefix fixed so far share one histogram, a "group": a level's pass compares each key with the at most RANKS
// group prefixes, and ranks part ways when they fall into different bins.  After the last level the prefixes are the keys.
// The first level has a single group with the empty prefix: the caller counts the top digit in a pass it makes anyway, and
// gives select_digit the rule that sets the ranks from the totals.
//
// Histograms are integer LDS atomics merged with integer global atomics: counts do not depend on scheduling.
#pragma once
#include "plane_util.h"

namespace bgnn {

// The digit widths of a key, most significant first.  Level l counts width(l) bits above shift(l) low bits.
template <int... W>
struct Digits {
  static constexpr int N = sizeof...(W);
  static constexpr int width(int level) {
    const int w[] = {W...};
    return w[level];
  }
  static constexpr int shift(int level) {
    const int w[] = {W...};
    int s = 0;
    for (int k = level + 1; k < N; ++k) s += w[k];
    return s;
  }
  template <typename Key>
  static constexpr bool covers() { return shift(0) + width(0) == 8 * (int)sizeof(Key); }
};

template <int RANKS, typename Key>
struct SelectState {
  Key prefix[RANKS];               // the key bits fixed so far, per rank (NONE: the rank does not exist)
  Key gprefix[RANKS];              // the same per group: the distinct prefixes
  int64_t rank[RANKS];             // the rank among the keys under the prefix (-1: the rank does not exist)
  int64_t rank0[RANKS];            // the rank among all keys
  int32_t group[RANKS];            // the histogram the rank reads at the next level (-1: none)
  int32_t ngroups, nranks;
  static constexpr Key NONE = ~(Key)0;       // matches no key: a prefix below the last level has fewer bits than the key
};

// the order-preserving uint32 image of a float32 (no NaN), and back
__device__ __forceinline__ uint32_t order_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// One count per active lane into an LDS histogram.  Called by whole waves (the ballots need every lane).  Real differences
// cluster around the offset, so most lanes of a wave hit one or two bins: two rounds take the bin of the first lane still
// waiting and add all its lanes at once; a clustered plane is done after them, a uniform one pays two ballots and goes on lane
// by lane.
__device__ __forceinline__ void hist_add(int32_t *hist, bool active, uint32_t bin) {
  const int lane = threadIdx.x & 63;
  unsigned long long waiting = __ballot(active);
#pragma unroll
  for (int round = 0; round < 2; ++round) {
    if (waiting == 0) break;                                    // (uniform)
    const int leader = __ffsll(waiting) - 1;
    const uint32_t lb = (uint32_t)__builtin_amdgcn_readlane((int)bin, leader);
    const bool mine = active && bin == lb;
    const unsigned long long m = __ballot(mine);
    if (lane == leader) atomicAdd(&hist[lb], (int32_t)__popcll(m));
    if (mine) active = false;
    waiting &= ~m;
  }
  if (active) atomicAdd(&hist[bin], 1);
}

// Count: uint32_t where the keys are fewer than 2^32, int64_t where they may be more
__device__ __forceinline__ void count_add(uint32_t *g, int32_t c) { atomicAdd(g, (uint32_t)c); }
__device__ __forceinline__ void count_add(int64_t *g, int32_t c) {
  atomicAdd(reinterpret_cast<unsigned long long *>(g), (unsigned long long)c);
}
template <typename Count>
__device__ __forceinline__ void hist_flush(const int32_t *lds, int bins, Count *global) {
  for (int b = threadIdx.x; b < bins; b += BLOCK_THREADS) {
    const int32_t c = lds[b];
    if (c != 0) count_add(global + b, c);
  }
}

// The digit of one level, counted per live group by a workgroup of a streaming pass.  SHIFT: the bits below this level's digit;
// BITS: the digit's width; the bits above the digit are the prefix.  LDS: RANKS << BITS counters; group g's histogram is
// [g << BITS, (g + 1) << BITS) in LDS and in the level's global histograms alike.
template <int RANKS, typename Key, int SHIFT, int BITS>
struct DigitCounter {
  static_assert(BITS >= 1 && SHIFT >= 0 && SHIFT + BITS < 8 * (int)sizeof(Key), "a level below the first: the prefix is not empty");
  static constexpr int BINS = 1 << BITS;
  int32_t *lds;
  int ng;                                                        // (uniform; 0 without a key)
  Key gp[RANKS];

  // every thread; clears the live groups' counters
  __device__ __forceinline__ void init(const SelectState<RANKS, Key> *__restrict__ sel, int32_t *counters) {
    lds = counters;
    ng = sel->ngroups;
#pragma unroll
    for (int g = 0; g < RANKS; ++g) gp[g] = sel->gprefix[g];
    for (int b = threadIdx.x; b < (ng << BITS); b += BLOCK_THREADS) lds[b] = 0;
    __syncthreads();
  }
  // whole waves; one key into every group whose prefix it has
  __device__ __forceinline__ void add(bool ok, Key key) {
    const Key top = key >> (SHIFT + BITS);
    const uint32_t bin = (uint32_t)(key >> SHIFT) & (BINS - 1);
#pragma unroll
    for (int g = 0; g < RANKS; ++g)
      if (g < ng) hist_add(lds + (g << BITS), ok && top == gp[g], bin);      // (uniform condition)
  }
  // every thread, after the last add
  template <typename Count>
  __device__ __forceinline__ void flush(Count *__restrict__ global) {
    __syncthreads();
    hist_flush(lds, ng << BITS, global);
  }
};

template <int RANKS, typename Key>
struct SelectScratch {             // LDS of select_digit
  int64_t part[BLOCK_THREADS + 1];
  SelectState<RANKS, Key> in, out;
};

// One workgroup of 256 threads walks a level's histograms (`hist`: group g at g << BITS) and narrows prefix and rank of every
// live rank, regroups, and stores the new state to *sel.  On return thread 0 may read sh.out (the new state) at once.
// FIRST: the single histogram of the top digit.  The state starts empty with `nranks` ranks, and thread 0 calls
//   rule(part, rank): part[k] = the keys in the bins below k * (BINS / 256), part[256] = all keys; it sets rank[r] of every
//   rank that exists (the others stay -1).
template <bool FIRST, int BITS, int RANKS, typename Key, typename Count, typename Rule>
__device__ __forceinline__ void select_digit(const Count *__restrict__ hist, SelectState<RANKS, Key> *sel, SelectScratch<RANKS, Key> &sh,
                                             int nranks, Rule rule) {
  constexpr int BINS = 1 << BITS, PER = BINS / BLOCK_THREADS;
  static_assert(PER >= 1, "a digit has at least 8 bits");
  constexpr Key NONE = SelectState<RANKS, Key>::NONE;
  SelectState<RANKS, Key> &in = sh.in, &out = sh.out;
  int64_t *part = sh.part;
  const int t = threadIdx.x;
  if (t == 0) {
    if (FIRST) {
      for (int r = 0; r < RANKS; ++r) { in.prefix[r] = 0; in.gprefix[r] = 0; in.rank[r] = -1; in.rank0[r] = -1; in.group[r] = 0; }
      in.ngroups = 1;
      in.nranks = nranks;
    } else {
      in = *sel;
    }
    for (int r = 0; r < RANKS; ++r) { out.prefix[r] = NONE; out.gprefix[r] = NONE; out.rank[r] = -1; out.group[r] = -1; }
  }
  __syncthreads();
  const int ng = in.ngroups;
  for (int g = 0; g < ng; ++g) {
    const Count *h = hist + ((size_t)g << BITS);
    Count local[PER];
    int64_t sum = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) { local[k] = h[t * PER + k]; sum += (int64_t)local[k]; }
    __syncthreads();                       // (the previous round's readers of part[] are done)
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
      int64_t run = 0;
#pragma unroll 8                           // (one thread's serial chain: eight LDS reads in flight, not sixteen register pairs)
      for (int k = 0; k < BLOCK_THREADS; ++k) { const int64_t v = part[k]; part[k] = run; run += v; }
      part[BLOCK_THREADS] = run;
      if (FIRST) {                         // the ranks, from the totals
        rule(part, in.rank);
        for (int r = 0; r < RANKS; ++r) {
          in.rank0[r] = in.rank[r];
          if (in.rank[r] < 0) in.group[r] = -1;
        }
      }
    }
    __syncthreads();
    const int64_t start = part[t];
    for (int r = 0; r < in.nranks; ++r) {
      const int64_t rank = in.rank[r];
      if (in.group[r] != g || rank < 0) continue;
      if (rank >= start && rank < start + sum) {                // exactly one thread: rank < the count under the prefix
        int64_t below = start;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
          if (rank >= below && rank < below + (int64_t)local[k]) {
            out.prefix[r] = (Key)(in.prefix[r] << BITS) | (Key)(t * PER + k);
            out.rank[r] = rank - below;
          }
          below += (int64_t)local[k];
        }
      }
    }
  }
  __syncthreads();
  if (t == 0) {                            // ranks under one prefix share a group
    int groups = 0;
    for (int r = 0; r < in.nranks; ++r) {
      out.rank0[r] = in.rank0[r];
      if (out.rank[r] < 0) continue;
      int g = -1;
      for (int q = 0; q < r; ++q)
        if (out.rank[q] >= 0 && out.prefix[q] == out.prefix[r]) { g = out.group[q]; break; }
      if (g < 0) { g = groups++; out.gprefix[g] = out.prefix[r]; }
      out.group[r] = g;
    }
    for (int r = in.nranks; r < RANKS; ++r) out.rank0[r] = -1;
    out.ngroups = groups;
    out.nranks = in.nranks;
    *sel = out;
  }
}

}  // namespace bgnn
