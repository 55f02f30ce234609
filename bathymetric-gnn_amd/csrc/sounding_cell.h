// The cell of a sounding (include/bgnn_soundings.h): one definition for the device pass and for the host check
// (tests/soundings_host_check.cpp compiles this header alone, with a host compiler).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BGNN_SOUNDING_HD __host__ __device__
#else
#define BGNN_SOUNDING_HD
#endif

namespace bgnn {

// row * width + col of (x, y) on the grid of height x width cells of res metres with the upper-left corner (x0, y0), or -1 where
// the sounding lies outside or a coordinate is not finite.  float64 and a true division: a multiply by 1 / res puts a sounding
// that lies on a cell border into the neighbour for many k * res.  The comparisons are made on the floored float64 values, before
// any conversion to an integer, so no coordinate, however large, takes the address out of range; NaN fails every comparison.
BGNN_SOUNDING_HD inline int64_t sounding_cell(double x, double y, double x0, double y0, double res, int64_t height, int64_t width) {
  const double col = floor((x - x0) / res), row = floor((y0 - y) / res);
  if (!(col >= 0.0 && col < (double)width && row >= 0.0 && row < (double)height)) return -1;
  return (int64_t)row * width + (int64_t)col;
}

}  // namespace bgnn
