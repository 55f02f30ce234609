// Synthetic training noise on the device (include/bgnn_noise.h): SyntheticNoiseGenerator.generate of the reference
// (data/synthetic_noise.py:98-408) for a batch of clean tiles resident in HBM.  The arithmetic restates numpy's operation by
// operation (this file is compiled with -ffp-contract=off); tests/_noise_cpu.py is the same in numpy.
//
// Five launches per batch, every reduction in float64 in a fixed order (no float atomics):
//   noise_stats1     per tile 64 workgroups: sum / count of the non-NaN cells, sum / count / min / max of the valid ones
//   noise_stats2     the same grid: sum of squared deviations from the valid mean (two-pass, as np.std); nanmean, range
//   noise_local_std  16 x 16 cells per workgroup from a 26 x 26 LDS tile (edge mode nearest, invalid cells = nanmean): the
//                    11 x 11 population std, two passes over the window in float64, stored float32; min / max per workgroup
//   noise_finalize   one workgroup per tile: depth_std, min / max of local_std; blob centres drawn as "the k-th valid cell" by a
//                    rank-select over the mask (valid counts per run of 256 cells from noise_stats1, a prefix, a walk of one run)
//   noise_apply      one thread per cell: Gaussian, spike, blob (walks the tile's blob list in order: the float32 running sum
//                    rounds after every blob) and systematic terms, the four outputs
// Only noise_local_std has arithmetic weight (242 LDS reads and float64 operations per cell); the rest moves 5 .. 55 B per cell.
#include "bgnn_internal.h"
#include "plane_util.h"
#include "../../include/bgnn_noise.h"

#include <math.h>
#include <string.h>

namespace bgnn {

constexpr int NOISE_NB1 = 64;        // workgroups per tile of the two statistics passes
constexpr int NOISE_R = BGNN_NOISE_WINDOW / 2;
constexpr int NOISE_TB = 16;         // cells per side of a stencil workgroup
constexpr int NOISE_HALO = NOISE_TB + 2 * NOISE_R;
constexpr int NOISE_MAX_SIDE = 32768;

struct NoiseTile {          // 32 B
  int64_t cell_off;
  int32_t h, w;
  int32_t sbx, sblk_n;      // stencil workgroups per row of workgroups, and in all
  int32_t ablk_n, pad;      // apply workgroups (256 cells each)
};

struct NoiseScalars {       // written by noise_stats2 (nanmean, n_valid, depth_range) and noise_finalize (the rest)
  int64_t n_valid;
  float nanmean, depth_std, depth_range;
  float lmin, lden;         // complexity = (local_std - lmin) / lden
  int32_t cx_on;            // 0: complexity is 0 everywhere (max == min, or a NaN in local_std)
};

struct NoiseLmm { float mn, mx; int32_t nan; };

struct NoiseArgs {
  const NoiseTile *tiles;
  const bgnn_noise_plan *plans;
  bgnn_noise_blob *blobs;
  NoiseScalars *scal;
  double *p1;               // [T][NB1][6]
  double *p2;               // [T][NB1]
  NoiseLmm *lmm;            // [T][max_sblk]
  float *lstd;              // [cells]
  int32_t *segcnt;          // [T][max_ablk]: valid cells of every run of 256 cells of a tile
  int32_t max_sblk, max_ablk;
  const float *depth;
  const uint8_t *mask;
  bgnn_noise_params prm;
  bgnn_noise_fields fld;
  float *noisy;
  uint8_t *nmask;
  float *mag;
  int64_t *cls;
};

// ---- the counter-based generator (bgnn_noise.h) -------------------------------------------------------------------------------
__host__ __device__ inline uint64_t noise_fin(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__host__ __device__ inline uint64_t noise_key(uint64_t seed, uint64_t sample) {
  return noise_fin(seed + 0x9E3779B97F4A7C15ull * (sample + 1ull));
}
__device__ __forceinline__ uint64_t noise_bits(uint64_t key, uint32_t stream, uint64_t cell) {
  return noise_fin(key + 0x9E3779B97F4A7C15ull * ((uint64_t)stream + 1ull) + 0xD1B54A32D192ED03ull * cell);
}
__device__ __forceinline__ double noise_uniform(uint64_t key, uint32_t stream, uint64_t cell) {
  return (double)(noise_bits(key, stream, cell) >> 11) * 0x1.0p-53;
}

// fixed-order trees over the 256 threads of a workgroup (plane_util.h); every thread gets the result
__device__ __forceinline__ double block_sum(double v, double *sh) { return block_reduce(v, sh, SumOp()); }
__device__ __forceinline__ float block_min(float v, float *sh) { return block_reduce(v, sh, [](float a, float b) { return fminf(a, b); }); }
__device__ __forceinline__ float block_max(float v, float *sh) { return block_reduce(v, sh, [](float a, float b) { return fmaxf(a, b); }); }

__global__ __launch_bounds__(256) void noise_stats1(NoiseArgs a) {
  __shared__ double shd[256];
  __shared__ float shf[256];
  const int t = blockIdx.y;
  const NoiseTile tl = a.tiles[t];
  const int64_t n = (int64_t)tl.h * tl.w;
  double s_nn = 0, c_nn = 0, s_v = 0, c_v = 0;
  float mn = INFINITY, mx = -INFINITY;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += (int64_t)NOISE_NB1 * 256) {      // (uniform trip count)
    const int64_t i = base + threadIdx.x;
    bool v = false;
    if (i < n) {
      const float d = a.depth[tl.cell_off + i];
      v = a.mask[tl.cell_off + i] != 0;
      if (!isnan(d)) { s_nn += (double)d; c_nn += 1.0; }
      if (v) { s_v += (double)d; c_v += 1.0; mn = fminf(mn, d); mx = fmaxf(mx, d); }
    }
    const int seg_valid = __syncthreads_count(v);          // valid cells of this run of 256 cells, for the rank-select
    if (threadIdx.x == 0) a.segcnt[(size_t)t * a.max_ablk + (base >> 8)] = seg_valid;
  }
  s_nn = block_sum(s_nn, shd); c_nn = block_sum(c_nn, shd);
  s_v = block_sum(s_v, shd); c_v = block_sum(c_v, shd);
  mn = block_min(mn, shf); mx = block_max(mx, shf);
  if (threadIdx.x == 0) {
    double *p = a.p1 + ((size_t)t * NOISE_NB1 + blockIdx.x) * 6;
    p[0] = s_nn; p[1] = c_nn; p[2] = s_v; p[3] = c_v; p[4] = (double)mn; p[5] = (double)mx;
  }
}

__global__ __launch_bounds__(256) void noise_stats2(NoiseArgs a) {
  __shared__ double shd[256];
  __shared__ double tot[6];
  const int t = blockIdx.y;
  const NoiseTile tl = a.tiles[t];
  const int64_t n = (int64_t)tl.h * tl.w;
  if (threadIdx.x == 0) {      // every workgroup of the tile adds the 64 partials in the same order
    double s_nn = 0, c_nn = 0, s_v = 0, c_v = 0, mn = INFINITY, mx = -INFINITY;
    for (int b = 0; b < NOISE_NB1; ++b) {
      const double *p = a.p1 + ((size_t)t * NOISE_NB1 + b) * 6;
      s_nn += p[0]; c_nn += p[1]; s_v += p[2]; c_v += p[3]; mn = fmin(mn, p[4]); mx = fmax(mx, p[5]);
    }
    tot[0] = s_nn; tot[1] = c_nn; tot[2] = s_v; tot[3] = c_v; tot[4] = mn; tot[5] = mx;
    if (blockIdx.x == 0) {
      NoiseScalars &s = a.scal[t];
      s.n_valid = (int64_t)c_v;
      s.nanmean = (float)(s_nn / c_nn);                   // 0 / 0 = NaN for a tile of NaNs, as np.nanmean
      s.depth_range = c_v > 0 ? (float)mx - (float)mn : 0.0f;
    }
  }
  __syncthreads();
  const double mean = tot[2] / tot[3];
  double q = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)NOISE_NB1 * 256)
    if (a.mask[tl.cell_off + i]) { const double d = (double)a.depth[tl.cell_off + i] - mean; q += d * d; }
  q = block_sum(q, shd);
  if (threadIdx.x == 0) a.p2[(size_t)t * NOISE_NB1 + blockIdx.x] = q;
}

__global__ __launch_bounds__(256) void noise_local_std(NoiseArgs a) {
  __shared__ float tile[NOISE_HALO][NOISE_HALO + 1];
  __shared__ float shf[256];
  const int t = blockIdx.y;
  const NoiseTile tl = a.tiles[t];
  if ((int)blockIdx.x >= tl.sblk_n) return;                 // (uniform per workgroup)
  const int r0 = ((int)blockIdx.x / tl.sbx) * NOISE_TB, c0 = ((int)blockIdx.x % tl.sbx) * NOISE_TB;
  const float fill = a.scal[t].nanmean;
  for (int idx = threadIdx.x; idx < NOISE_HALO * NOISE_HALO; idx += 256) {
    const int rr = idx / NOISE_HALO, cc = idx - rr * NOISE_HALO;
    int r = r0 + rr - NOISE_R, c = c0 + cc - NOISE_R;
    r = r < 0 ? 0 : (r > tl.h - 1 ? tl.h - 1 : r);          // edge mode nearest
    c = c < 0 ? 0 : (c > tl.w - 1 ? tl.w - 1 : c);
    const int64_t g = tl.cell_off + (int64_t)r * tl.w + c;
    tile[rr][cc] = a.mask[g] ? a.depth[g] : fill;
  }
  __syncthreads();
  const int lr = threadIdx.x / NOISE_TB, lc = threadIdx.x % NOISE_TB;
  const int r = r0 + lr, c = c0 + lc;
  const bool in = r < tl.h && c < tl.w;
  float v = 0.0f;
  if (in) {
    double s = 0;
    for (int i = 0; i < BGNN_NOISE_WINDOW; ++i)
      for (int j = 0; j < BGNN_NOISE_WINDOW; ++j) s += (double)tile[lr + i][lc + j];
    const double mean = s / (double)(BGNN_NOISE_WINDOW * BGNN_NOISE_WINDOW);
    double q = 0;
    for (int i = 0; i < BGNN_NOISE_WINDOW; ++i)
      for (int j = 0; j < BGNN_NOISE_WINDOW; ++j) { const double d = (double)tile[lr + i][lc + j] - mean; q += d * d; }
    v = (float)sqrt(q / (double)(BGNN_NOISE_WINDOW * BGNN_NOISE_WINDOW));
    a.lstd[tl.cell_off + (int64_t)r * tl.w + c] = v;
  }
  const int any_nan = __syncthreads_or(in && isnan(v));
  const float mn = block_min(in ? v : INFINITY, shf), mx = block_max(in ? v : -INFINITY, shf);
  if (threadIdx.x == 0) a.lmm[(size_t)t * a.max_sblk + blockIdx.x] = NoiseLmm{mn, mx, any_nan};
}

__global__ __launch_bounds__(256) void noise_finalize(NoiseArgs a) {
  __shared__ float shf[256];
  __shared__ int64_t pre[257];
  const int t = blockIdx.x;
  const NoiseTile tl = a.tiles[t];
  const bgnn_noise_plan pl = a.plans[t];
  const int64_t n = (int64_t)tl.h * tl.w;
  float mn = INFINITY, mx = -INFINITY;
  int nan = 0;
  for (int b = threadIdx.x; b < tl.sblk_n; b += 256) {
    const NoiseLmm m = a.lmm[(size_t)t * a.max_sblk + b];
    mn = fminf(mn, m.mn); mx = fmaxf(mx, m.mx); nan |= m.nan;
  }
  nan = __syncthreads_or(nan);
  mn = block_min(mn, shf); mx = block_max(mx, shf);
  // rank-select over the mask: the valid counts of the runs of 256 cells (noise_stats1), a strip of runs per thread, their prefix
  const int32_t *seg = a.segcnt + (size_t)t * a.max_ablk;
  const int per = (tl.ablk_n + 255) / 256;
  const int s_lo = (int)threadIdx.x * per, s_hi = s_lo + per < tl.ablk_n ? s_lo + per : tl.ablk_n;
  int64_t cnt = 0;
  for (int sg = s_lo; sg < s_hi; ++sg) cnt += seg[sg];
  pre[threadIdx.x + 1] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    pre[0] = 0;
    for (int i = 0; i < 256; ++i) pre[i + 1] += pre[i];
    double q = 0;
    for (int b = 0; b < NOISE_NB1; ++b) q += a.p2[(size_t)t * NOISE_NB1 + b];
    NoiseScalars &s = a.scal[t];
    s.depth_std = s.n_valid > 0 ? (float)sqrt(q / (double)s.n_valid) : 0.0f;
    s.cx_on = (!nan && mx > mn) ? 1 : 0;
    s.lmin = mn; s.lden = mx - mn;
  }
  __syncthreads();
  const int64_t nv = pre[256];
  if (nv <= 0) return;
  for (int b = threadIdx.x; b < pl.blob_count; b += 256) {
    bgnn_noise_blob &bl = a.blobs[pl.blob_first + b];
    if (bl.row >= 0) continue;
    int64_t k = (int64_t)(bl.centre_u * (double)nv);
    k = k < 0 ? 0 : (k > nv - 1 ? nv - 1 : k);
    int j = 0;
    while (j < 255 && pre[j + 1] <= k) ++j;                 // pre[j] <= k < pre[j + 1]: the strip, then the run, then the cell
    int64_t left = k - pre[j];
    int sg = j * per;
    const int sg_end = sg + per < tl.ablk_n ? sg + per : tl.ablk_n;
    while (sg < sg_end - 1 && left >= seg[sg]) { left -= seg[sg]; ++sg; }
    int64_t i = (int64_t)sg * 256, end = i + 256 < n ? i + 256 : n, found = -1;
    for (; i < end; ++i)
      if (a.mask[tl.cell_off + i]) { if (left == 0) { found = i; break; } --left; }
    if (found >= 0) { bl.row = (int32_t)(found / tl.w); bl.col = (int32_t)(found % tl.w); }
  }
}

__device__ __forceinline__ float noise_scale32(double factor, float base, double intensity) {
  return ((float)factor * base) * (float)intensity;
}
__device__ __forceinline__ double noise_linspace(int i, int n) {      // np.linspace(-1, 1, n)[i]
  if (n == 1) return (double)i * 2.0 + -1.0;
  if (i == n - 1) return 1.0;
  return (double)i * (2.0 / (double)(n - 1)) + -1.0;
}

__global__ __launch_bounds__(256) void noise_apply(NoiseArgs a) {
  const int t = blockIdx.y;
  const NoiseTile tl = a.tiles[t];
  if ((int)blockIdx.x >= tl.ablk_n) return;
  const int64_t n = (int64_t)tl.h * tl.w;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t g = tl.cell_off + i;
  const uint32_t in_bits = __float_as_uint(a.depth[g]);
  const bool valid = a.mask[g] != 0;
  float depth = __uint_as_float(in_bits), mag = 0.0f;
  bool marked = false;
  if (valid) {
    const bgnn_noise_plan pl = a.plans[t];
    const NoiseScalars sc = a.scal[t];
    const int row = (int)(i / tl.w), col = (int)(i - (int64_t)row * tl.w);
    const uint64_t key = noise_key(a.prm.seed, pl.sample);
    if (a.prm.enable_gaussian) {
      const float ns = noise_scale32(pl.gaussian_std_factor, sc.depth_std, pl.intensity);
      double g64;
      if (a.fld.gaussian) g64 = a.fld.gaussian[g];
      else {
        const double u1 = ((double)(noise_bits(key, 1, (uint64_t)i) >> 11) + 1.0) * 0x1.0p-53;
        const double u2 = noise_uniform(key, 2, (uint64_t)i);
        g64 = 0.0 + (double)ns * (sqrt(-2.0 * log(u1)) * cos((2.0 * M_PI) * u2));
      }
      const float g32 = (float)g64;
      depth += g32;
      if (fabsf(g32) > 2.0f * ns) marked = true;
      mag = fmaxf(mag, fabsf(g32));
    }
    if (a.prm.enable_spikes) {
      const float cx = sc.cx_on ? (a.lstd[g] - sc.lmin) / sc.lden : 0.0f;
      const float dens = (float)pl.spike_density * (1.0f + (float)a.prm.complexity_correlation * (cx - 0.5f));
      const double u = a.fld.uniform ? a.fld.uniform[g] : noise_uniform(key, 3, (uint64_t)i);
      if (u < (double)dens) {
        const double sg = a.fld.sign ? (double)a.fld.sign[g] : ((noise_bits(key, 4, (uint64_t)i) >> 63) ? 1.0 : -1.0);
        const double m = a.fld.magnitude ? a.fld.magnitude[g]
                                         : a.prm.spike_mag_min + (a.prm.spike_mag_max - a.prm.spike_mag_min) * noise_uniform(key, 5, (uint64_t)i);
        const double v = sg * ((m * (double)sc.depth_range) * pl.intensity);
        depth = (float)((double)depth + v);
        marked = true;
        mag = (float)fabs(v);
      }
    }
    if (a.prm.enable_blobs) {
      for (int b = 0; b < pl.blob_count; ++b) {
        const bgnn_noise_blob bl = a.blobs[pl.blob_first + b];      // (one address per wave)
        if (bl.row < 0) continue;
        const int64_t dr = row - bl.row, dc = col - bl.col, d2 = dr * dr + dc * dc;
        if (d2 >= (int64_t)bl.size * bl.size) continue;
        const double dist = sqrt((double)d2), half = (double)bl.size / 2.0;
        const double c = exp(-(dist * dist) / (2.0 * (half * half))) * (double)noise_scale32(bl.magnitude, sc.depth_range, pl.intensity);
        depth = (float)((double)depth + c);
        marked = true;
        mag = fmaxf(mag, (float)fabs(c));
      }
    }
    if (a.prm.enable_systematic && pl.artifact != BGNN_NOISE_ARTIFACT_NONE) {
      const float amp = noise_scale32(pl.amplitude_factor, sc.depth_std, pl.intensity);
      const double a64 = (double)amp;
      double art;
      switch (pl.artifact) {
        case BGNN_NOISE_STRIPE_HORIZONTAL: art = a64 * sin(((2.0 * M_PI) * pl.freq_a) * (double)row); break;
        case BGNN_NOISE_STRIPE_VERTICAL: art = a64 * sin(((2.0 * M_PI) * pl.freq_a) * (double)col); break;
        case BGNN_NOISE_WAVE: art = a64 * sin((2.0 * M_PI) * (pl.freq_a * (double)col + pl.freq_b * (double)row) + pl.phase); break;
        case BGNN_NOISE_GRADIENT_X: art = a64 * noise_linspace(col, tl.w); break;
        case BGNN_NOISE_GRADIENT_Y: art = a64 * noise_linspace(row, tl.h); break;
        default: art = a64 * (noise_linspace(col, tl.w) + noise_linspace(row, tl.h)) / 2.0; break;
      }
      const float a32 = (float)art;
      depth += a32;
      if (fabsf(a32) > amp * 0.5f) marked = true;
      mag = fmaxf(mag, fabsf(a32));
    }
  }
  a.noisy[g] = valid ? depth : __uint_as_float(in_bits);
  a.nmask[g] = marked ? 1 : 0;
  a.mag[g] = mag;
  a.cls[g] = marked ? 2 : 0;
}

struct NoiseLayout {
  size_t tiles, plans, blobs, host_bytes, scal, p1, p2, lmm, segcnt, lstd, total;
  int64_t cells;
  int32_t max_sblk, max_ablk;
};


// false: arguments bgnn_noise_generate refuses (`why`, `code` say which way)
static bool noise_layout(int32_t n_tiles, const int32_t *hw, int32_t n_blobs, NoiseLayout &L, const char **why, int *code) {
  *code = BGNN_ERR_INVALID;
  if (n_tiles < 1 || !hw || n_blobs < 0) { *why = "no tiles, a NULL tile table or a negative blob count"; return false; }
  if (n_tiles > 65535) { *why = "more than 65535 tiles in one batch"; *code = BGNN_ERR_UNSUPPORTED; return false; }
  L.cells = 0; L.max_sblk = 0; L.max_ablk = 0;
  for (int32_t t = 0; t < n_tiles; ++t) {
    const int64_t h = hw[2 * t], w = hw[2 * t + 1];
    if (h < 1 || w < 1) { *why = "a tile with rows or cols < 1"; return false; }
    if (h > NOISE_MAX_SIDE || w > NOISE_MAX_SIDE) { *why = "a tile with more than 32768 rows or columns"; *code = BGNN_ERR_UNSUPPORTED; return false; }
    L.cells += h * w;
    if (L.cells >= (1ll << 31)) { *why = "a batch of 2^31 cells or more"; *code = BGNN_ERR_UNSUPPORTED; return false; }
    const int64_t sb = ((h + NOISE_TB - 1) / NOISE_TB) * ((w + NOISE_TB - 1) / NOISE_TB), ab = (h * w + 255) / 256;
    if (sb > L.max_sblk) L.max_sblk = (int32_t)sb;
    if (ab > L.max_ablk) L.max_ablk = (int32_t)ab;
  }
  size_t o = 0;
  L.tiles = o; o += (size_t)n_tiles * sizeof(NoiseTile);
  L.plans = o; o += (size_t)n_tiles * sizeof(bgnn_noise_plan);
  L.blobs = o; o += (size_t)n_blobs * sizeof(bgnn_noise_blob);
  L.host_bytes = o; o = align256(o);
  L.scal = o; o = align256(o + (size_t)n_tiles * sizeof(NoiseScalars));
  L.p1 = o; o = align256(o + (size_t)n_tiles * NOISE_NB1 * 6 * sizeof(double));
  L.p2 = o; o = align256(o + (size_t)n_tiles * NOISE_NB1 * sizeof(double));
  L.lmm = o; o = align256(o + (size_t)n_tiles * L.max_sblk * sizeof(NoiseLmm));
  L.segcnt = o; o = align256(o + (size_t)n_tiles * L.max_ablk * sizeof(int32_t));
  L.lstd = o; o = align256(o + (size_t)L.cells * sizeof(float));
  L.total = o;
  return true;
}

}  // namespace bgnn

using namespace bgnn;

static_assert(sizeof(NoiseTile) == 32 && sizeof(bgnn_noise_plan) == 80 && sizeof(bgnn_noise_blob) == 32, "table layout");

extern "C" size_t bgnn_noise_workspace_bytes(int32_t n_tiles, const int32_t *hw, int32_t n_blobs) {
  NoiseLayout L;
  const char *why;
  int code;
  return noise_layout(n_tiles, hw, n_blobs, L, &why, &code) ? L.total : 0;
}

extern "C" int bgnn_noise_generate(bgnn_ctx *ctx, int32_t n_tiles, const int32_t *hw, const float *depth, const uint8_t *mask,
                                   const bgnn_noise_params *params, const bgnn_noise_plan *plans, const bgnn_noise_blob *blobs,
                                   int32_t n_blobs, const bgnn_noise_fields *fields, void *workspace, size_t workspace_bytes,
                                   float *noisy, uint8_t *noise_mask, float *magnitude, int64_t *classification) {
  BGNN_REQUIRE(ctx && depth && mask && params && plans && workspace && noisy && noise_mask && magnitude && classification,
               "bgnn_noise_generate: NULL argument");
  BGNN_REQUIRE(n_blobs == 0 || blobs, "bgnn_noise_generate: NULL blob list");
  BGNN_REQUIRE(noisy != depth, "bgnn_noise_generate: noisy must not alias depth");
  NoiseLayout L;
  const char *why = "";
  int code = BGNN_ERR_INVALID;
  if (!noise_layout(n_tiles, hw, n_blobs, L, &why, &code)) {
    set_error("bgnn_noise_generate: %s", why);
    return code;
  }
  BGNN_REQUIRE(workspace_bytes >= L.total, "bgnn_noise_generate: workspace of %zu bytes, %zu needed", workspace_bytes, L.total);
  BGNN_REQUIRE(((uintptr_t)workspace & 15) == 0, "bgnn_noise_generate: workspace not 16-byte aligned");
  int32_t blob_end = 0;
  for (int32_t t = 0; t < n_tiles; ++t) {
    const bgnn_noise_plan &p = plans[t];
    if (p.artifact < BGNN_NOISE_ARTIFACT_NONE || p.artifact > BGNN_NOISE_GRADIENT_DIAGONAL) {
      set_error("bgnn_noise_generate: tile %d: artifact code %d is not supported", t, p.artifact);
      return BGNN_ERR_UNSUPPORTED;
    }
    BGNN_REQUIRE(p.blob_count >= 0 && p.blob_first >= blob_end && (int64_t)p.blob_first + p.blob_count <= n_blobs,
                 "bgnn_noise_generate: tile %d: blobs [%d, %d + %d) outside the list of %d or overlapping an earlier tile's", t,
                 p.blob_first, p.blob_first, p.blob_count, n_blobs);
    if (p.blob_count > 0) blob_end = p.blob_first + p.blob_count;
  }
  for (int32_t b = 0; b < n_blobs; ++b)
    BGNN_REQUIRE(blobs[b].size >= 0 && blobs[b].size <= 2 * NOISE_MAX_SIDE, "bgnn_noise_generate: blob %d has size %d", b, blobs[b].size);
  BGNN_HIP_CHECK(hipSetDevice(ctx->device));
  // the host tables, in one copy
  std::vector<char> host(L.host_bytes);
  NoiseTile *ht = reinterpret_cast<NoiseTile *>(host.data() + L.tiles);
  int64_t off = 0;
  for (int32_t t = 0; t < n_tiles; ++t) {
    const int32_t h = hw[2 * t], w = hw[2 * t + 1];
    const int32_t sbx = (w + NOISE_TB - 1) / NOISE_TB;
    ht[t] = NoiseTile{off, h, w, sbx, sbx * ((h + NOISE_TB - 1) / NOISE_TB), (int32_t)(((int64_t)h * w + 255) / 256), 0};
    off += (int64_t)h * w;
  }
  memcpy(host.data() + L.plans, plans, (size_t)n_tiles * sizeof(bgnn_noise_plan));
  if (n_blobs) memcpy(host.data() + L.blobs, blobs, (size_t)n_blobs * sizeof(bgnn_noise_blob));
  char *ws = static_cast<char *>(workspace);
  BGNN_TRY(ctx_upload(ctx, host.data(), L.host_bytes, ws));
  NoiseArgs a{};
  a.tiles = reinterpret_cast<const NoiseTile *>(ws + L.tiles);
  a.plans = reinterpret_cast<const bgnn_noise_plan *>(ws + L.plans);
  a.blobs = reinterpret_cast<bgnn_noise_blob *>(ws + L.blobs);
  a.scal = reinterpret_cast<NoiseScalars *>(ws + L.scal);
  a.p1 = reinterpret_cast<double *>(ws + L.p1);
  a.p2 = reinterpret_cast<double *>(ws + L.p2);
  a.lmm = reinterpret_cast<NoiseLmm *>(ws + L.lmm);
  a.lstd = reinterpret_cast<float *>(ws + L.lstd);
  a.segcnt = reinterpret_cast<int32_t *>(ws + L.segcnt);
  a.max_sblk = L.max_sblk; a.max_ablk = L.max_ablk;
  a.depth = depth; a.mask = mask;
  a.prm = *params;
  a.fld = fields ? *fields : bgnn_noise_fields{nullptr, nullptr, nullptr, nullptr};
  a.noisy = noisy; a.nmask = noise_mask; a.mag = magnitude; a.cls = classification;
  {
    ProfScope ps(ctx, BGNN_K_STATS);
    hipLaunchKernelGGL(noise_stats1, dim3(NOISE_NB1, n_tiles), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(noise_stats2, dim3(NOISE_NB1, n_tiles), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(noise_local_std, dim3(L.max_sblk, n_tiles), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(noise_finalize, dim3(n_tiles), dim3(256), 0, ctx->stream, a);
  }
  {
    ProfScope ps(ctx, BGNN_K_SCATTER);
    hipLaunchKernelGGL(noise_apply, dim3(L.max_ablk, n_tiles), dim3(256), 0, ctx->stream, a);
  }
  BGNN_HIP_CHECK(hipGetLastError());
  return BGNN_OK;
}
