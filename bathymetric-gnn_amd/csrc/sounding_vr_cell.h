// The record of a sounding on a variable-resolution layout (include/bgnn_soundings_vr.h): one definition for the device passes
// and for the host check (tests/vr_cell_host_check.cpp compiles this header alone, with a host compiler).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BGNN_VR_CELL_HD __host__ __device__
#else
#define BGNN_VR_CELL_HD
#endif

namespace bgnn {

// one base cell of the layout table: the first record of its refinement grid and the grid's dimensions (0, 0: not refined)
struct VRLayoutEntry {
  int64_t index;
  int32_t dx, dy;
};
static_assert(sizeof(VRLayoutEntry) == 16, "the entry the header documents");

// br * BW + bc of (x, y) on the base grid of BH x BW cells of B metres with the SOUTH-WEST corner (x0, y0), base row 0 the
// southmost, or -1 where the sounding lies off the base grid or a coordinate is not finite.  float64 and true divisions, the
// comparisons on the floored float64 values before any conversion to an integer (as sounding_cell.h).  *fu, *fv: the position
// inside the base cell, in base cells, each in [0, 1): u - floor(u) is exact.
BGNN_VR_CELL_HD inline int64_t vr_base_cell(double x, double y, double x0, double y0, double B, int64_t BH, int64_t BW, double *fu,
                                            double *fv) {
  const double u = (x - x0) / B, v = (y - y0) / B;
  const double bc = floor(u), br = floor(v);
  if (!(bc >= 0.0 && bc < (double)BW && br >= 0.0 && br < (double)BH)) return -1;
  *fu = u - bc;
  *fv = v - br;
  return (int64_t)br * BW + (int64_t)bc;
}

// The record of a position inside a refined base cell: refinement row 0 the southmost, row-major.  No clamp: fu <= 1 - 2^-53 and
// round-to-nearest give fl(fu * d) < d for every d in 1 .. 32768 (tests/test_host_vr_soundings.py asserts it for every d).
BGNN_VR_CELL_HD inline int64_t vr_record(const VRLayoutEntry &e, double fu, double fv) {
  const double sc = floor(fu * (double)e.dx), sr = floor(fv * (double)e.dy);
  return e.index + (int64_t)sr * e.dx + (int64_t)sc;
}

// Whether the entry is a refinement grid that lies inside a state of `total` records.  Every entry of a planned layout that has
// dimensions does; this is what keeps a table that does not belong to the state from taking a store out of it.
BGNN_VR_CELL_HD inline bool vr_entry_refined(const VRLayoutEntry &e, int64_t total) {
  if (e.dx < 1 || e.dy < 1 || e.dx > 32768 || e.dy > 32768 || e.index < 0) return false;
  return e.index <= total - (int64_t)e.dx * (int64_t)e.dy;
}

}  // namespace bgnn
