/*
 * bgnn_noise.h -- C ABI of libbgnn_hip.so, synthetic training noise (ABI 7, additive).
 *
 * The conventions of bgnn.h hold (DEVICE / HOST pointers, return codes, bgnn_last_error(), the context's stream).  This header
 * adds the generator behind data/synthetic_noise.py's SyntheticNoiseGenerator (reference data/synthetic_noise.py:98-408,
 * generate and its four _add_*_noise steps) for a batch of clean tiles resident in HBM, in the flat concatenated row-major
 * layout of bgnn_tiles (hw table, depth, mask).  The Python mirror binds the entry points in bathymetric_gnn_amd/runtime.py
 * (_NOISE_SIGNATURES).
 *
 * Every formula is the reference's, with numpy 2's promotion of its float32 / float64 / Python-float mix; "f32(x)" below is a
 * rounding to float32, everything else is float64.  Per tile, with valid = mask != 0:
 *   nanmean      f32(sum / count over the cells that are not NaN)        depth_std   f32(population std of the valid depths)
 *   depth_range  f32(max) - f32(min) of the valid depths, in float32     local_std   f32(population std over the 11 x 11 window,
 *   edge mode nearest, of the tile with its invalid cells replaced by nanmean);  complexity = (local_std - min) / (max - min) in
 *   float32, 0 everywhere when max == min.  Sums run in float64 in a fixed order (no float atomics): two runs give equal bits.
 *   scale32(f, b) = f32(f32(f32(f) * b) * f32(intensity))    (a Python float times a float32 scalar times a Python float)
 * Terms, in this order, each applied to valid cells only:
 *   Gaussian    noise_std = scale32(gaussian_std_factor, depth_std); g = f32(noise_std * z); depth += g (float32); marked where
 *               |g| > f32(2 noise_std); magnitude = max(magnitude, |g|)
 *   spikes      density = f32(spike_density) * (1 + f32(complexity_correlation) * (complexity - 0.5)) in float32; where
 *               u < density: v = sign * ((m * depth_range) * intensity); depth = f32(depth + v); marked; magnitude = f32(|v|)
 *               (a spike OVERWRITES the magnitude), m = spike_mag_min + (spike_mag_max - spike_mag_min) * u'
 *   blobs       in list order, for the cells with dr^2 + dc^2 < size^2 (integers): c = exp(-d^2 / (2 (size / 2)^2)) *
 *               scale32(magnitude, depth_range), d = sqrt(dr^2 + dc^2); depth = f32(depth + c); marked; magnitude = max(., f32(|c|))
 *   systematic  a = f32(amplitude * s), amplitude = scale32(amplitude_factor, depth_std), s by artifact:
 *               stripes sin(((2 pi) freq_a) * row | col); wave sin((2 pi) * (freq_a * col + freq_b * row) + phase); gradients
 *               linspace(-1, 1, w)[col], linspace(-1, 1, h)[row], or their sum, times amplitude, halved;
 *               depth += a (float32); marked where |a| > f32(amplitude * 0.5); magnitude = max(., |a|)
 * classification = marked ? 2 : 0.  Invalid cells keep their input bits (NaN payloads included), are never marked and have
 * magnitude 0; a tile without a valid cell comes back as it went in.
 *
 * Random draws.  The scalar draws (the plan) are made by the caller.  The per-cell draws are either supplied
 * (bgnn_noise_fields) or made on the device by a counter-based generator on splitmix64's finaliser (the one of bgnn_dropout),
 * a pure function of (seed, sample, stream, cell) -- reproducible, independent of launch geometry and of the batch a sample is
 * generated in; numpy's own stream cannot be followed on the device:
 *   fin(z):  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  z ^= z >> 31
 *   key  = fin(seed + 0x9E3779B97F4A7C15 * (sample + 1))                                                     (mod 2^64)
 *   bits(stream, cell) = fin(key + 0x9E3779B97F4A7C15 * (stream + 1) + 0xD1B54A32D192ED03 * cell),   cell = row * w + col
 *   uniform = (bits >> 11) * 2^-53  in [0, 1)
 *   z (normal) = sqrt(-2 ln u1) * cos((2 pi) u2),  u1 = ((bits(1, cell) >> 11) + 1) * 2^-53 in (0, 1],  u2 = uniform(2, cell)
 *   u = uniform(3, cell);  sign = bit 63 of bits(4, cell) ? +1 : -1;  u' = uniform(5, cell)
 * tests/_noise_cpu.py restates the generator and the kernels in numpy.
 */
#ifndef BGNN_NOISE_H
#define BGNN_NOISE_H

#include "bgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BGNN_NOISE_WINDOW 11 /* side of the complexity window */

/* artifact of the systematic term */
#define BGNN_NOISE_ARTIFACT_NONE 0
#define BGNN_NOISE_STRIPE_HORIZONTAL 1
#define BGNN_NOISE_STRIPE_VERTICAL 2
#define BGNN_NOISE_WAVE 3
#define BGNN_NOISE_GRADIENT_X 4
#define BGNN_NOISE_GRADIENT_Y 5
#define BGNN_NOISE_GRADIENT_DIAGONAL 6

/* What the generator object holds: which terms run and the parameters that are not drawn. */
typedef struct bgnn_noise_params {
  int32_t enable_gaussian, enable_spikes, enable_blobs, enable_systematic;
  double complexity_correlation;
  double spike_mag_min, spike_mag_max;
  uint64_t seed; /* of the device's per-cell draws */
} bgnn_noise_params;

/* One blob.  row >= 0: the centre is (row, col).  row < 0: the centre is the floor(centre_u * n_valid)-th valid cell of the
 * tile in row-major order, found on the device (the mask never goes to the host). */
typedef struct bgnn_noise_blob {
  int32_t row, col, size, pad;
  double centre_u;  /* in [0, 1) */
  double magnitude; /* the uniform draw of blob_magnitude_range, negated for a shadow */
} bgnn_noise_blob;

/* The scalar draws of one tile and its slice [blob_first, blob_first + blob_count) of the blob list. */
typedef struct bgnn_noise_plan {
  uint64_t sample;            /* sample index of the device's per-cell draws */
  double intensity;
  double gaussian_std_factor; /* uniform draw of gaussian_std_range */
  double spike_density;       /* uniform draw of spike_density_range, times intensity */
  double amplitude_factor;    /* uniform draw of systematic_amplitude_range */
  double freq_a, freq_b, phase; /* stripes: freq_a; wave: freq_a (x), freq_b (y), phase */
  int32_t artifact;           /* BGNN_NOISE_* */
  int32_t blob_first, blob_count, pad;
} bgnn_noise_plan;

/* Supplied per-cell draws, DEVICE, [cells] in the layout of depth; any may be NULL (then the device draws that field). */
typedef struct bgnn_noise_fields {
  const double *gaussian;  /* the final noise field noise_std * z, before its rounding to float32 */
  const double *uniform;   /* u of the spike location test */
  const int8_t *sign;      /* +1 / -1 */
  const double *magnitude; /* m, the draw of spike_magnitude_range */
} bgnn_noise_fields;

/* bgnn_noise_workspace_bytes: bytes of DEVICE workspace bgnn_noise_generate needs for these tiles and n_blobs blobs (hw HOST
 *   int32 [n_tiles][2]); 0 for arguments bgnn_noise_generate refuses.
 *
 * bgnn_noise_generate: depth (float32) and mask (u8, non-zero = valid) DEVICE [cells]; plans HOST [n_tiles], blobs HOST
 *   [n_blobs] (copied before the call returns); fields may be NULL.  Outputs, DEVICE [cells]: noisy (float32), noise_mask (u8,
 *   0 / 1), magnitude (float32), classification (int64); noisy must not alias depth.  Asynchronous, on the context's stream; the
 *   workspace must stay untouched until the call's work has completed.
 *   BGNN_ERR_INVALID: NULL arguments, a tile with rows or cols < 1, a blob slice outside the list, a blob size < 0,
 *   workspace_bytes too small.  BGNN_ERR_UNSUPPORTED: an artifact code this library does not know, a tile with more than 32768
 *   rows or columns, a batch of 2^31 cells or more or of more than 65535 tiles. */
size_t bgnn_noise_workspace_bytes(int32_t n_tiles, const int32_t *hw, int32_t n_blobs);
int bgnn_noise_generate(bgnn_ctx *ctx, int32_t n_tiles, const int32_t *hw, const float *depth, const uint8_t *mask,
                        const bgnn_noise_params *params, const bgnn_noise_plan *plans, const bgnn_noise_blob *blobs,
                        int32_t n_blobs, const bgnn_noise_fields *fields, void *workspace, size_t workspace_bytes, float *noisy,
                        uint8_t *noise_mask, float *magnitude, int64_t *classification);

#ifdef __cplusplus
}
#endif
#endif /* BGNN_NOISE_H */
