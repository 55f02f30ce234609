// What the entry points of the sounding gridders (sounding_grid.hip, sounding_robust.hip, sounding_vr.hip) check of their arguments
// before anything is launched: one definition each.  Every check sets bgnn_last_error() with the entry point's name in front and
// returns its code; the callers go through BGNN_TRY and check the context last, so what is wrong with the other arguments is
// reported whatever the context.
#pragma once
#include "bgnn_internal.h"
#include "../../include/bgnn_soundings.h"
#include "../../include/bgnn_soundings_robust.h"

namespace bgnn {

constexpr int64_t SOUNDING_MAX_DIM = 2147483647;

inline bool dim_ok(int64_t v) { return v >= 1 && v <= SOUNDING_MAX_DIM; }
inline bool cells_ok(int64_t height, int64_t width, int64_t max_cells) { return height <= max_cells / width; }      // (width >= 1)
inline bool stage_capacity_ok(int64_t v) { return v >= 1 && v <= (int64_t)BGNN_ROBUST_MAX_CAPACITY; }
inline bool aligned8(const void *p) { return ((uintptr_t)p & 7) == 0; }
inline bool finite_arg(double v) { return v - v == 0.0; }

// n, the three coordinate arrays, the resolution (what_res: "resolution" or "base resolution") and the origin of a cloud pass.
// others: whether the other pointers are there that the entry point reports at the same place, under the same message.
inline int require_cloud(const char *fn, const void *x, const void *y, const void *z, int64_t n, double res, double x0, double y0,
                         const char *what_res, bool others = true) {
  BGNN_REQUIRE(n >= 0, "%s: %lld soundings", fn, (long long)n);
  BGNN_REQUIRE(others && (n == 0 || (x && y && z)), "%s: NULL argument", fn);
  BGNN_REQUIRE(finite_arg(res) && res > 0.0, "%s: a %s of %g, a finite number above 0 expected", fn, what_res, res);
  BGNN_REQUIRE(finite_arg(x0) && finite_arg(y0), "%s: the origin (%g, %g) is not finite", fn, x0, y0);
  return BGNN_OK;
}

// what: "grid" or "base grid".  max_cells: the cap on height * width (0: none), beyond which the grid is unsupported; why: what
// the message says after the cap.
inline int require_grid(const char *fn, int64_t height, int64_t width, const char *what, int64_t max_cells, const char *why) {
  BGNN_REQUIRE(dim_ok(height) && dim_ok(width), "%s: a %s of %lld x %lld cells, 1 .. 2147483647 each way expected", fn, what,
               (long long)height, (long long)width);
  if (max_cells && !cells_ok(height, width, max_cells)) {
    set_error("%s: a %s of %lld x %lld cells: more than %lld in all%s", fn, what, (long long)height, (long long)width,
              (long long)max_cells, why);
    return BGNN_ERR_UNSUPPORTED;
  }
  return BGNN_OK;
}
inline int require_robust_grid(const char *fn, int64_t height, int64_t width) {
  return require_grid(fn, height, width, "grid", BGNN_ROBUST_MAX_CELLS, ", a cell would not fit the int32 of the stage");
}

inline int require_capacity(const char *fn, int64_t capacity) {
  BGNN_REQUIRE(stage_capacity_ok(capacity), "%s: a capacity of %lld soundings, 1 .. %lld expected", fn, (long long)capacity,
               (long long)BGNN_ROBUST_MAX_CAPACITY);
  return BGNN_OK;
}

// n more soundings after `offered`: within the total a state counts ...
inline int require_offered_total(const char *fn, int64_t n, int64_t offered) {
  BGNN_REQUIRE(offered >= 0, "%s: %lld soundings offered before", fn, (long long)offered);
  BGNN_REQUIRE(n <= (int64_t)BGNN_SOUNDINGS_MAX_TOTAL && offered <= (int64_t)BGNN_SOUNDINGS_MAX_TOTAL - n,
               "%s: %lld soundings after %lld offered before: a total above %lld", fn, (long long)n, (long long)offered,
               (long long)BGNN_SOUNDINGS_MAX_TOTAL);
  return BGNN_OK;
}
// ... or within the capacity of a stage
inline int require_offered_capacity(const char *fn, int64_t n, int64_t offered, int64_t capacity) {
  BGNN_REQUIRE(offered >= 0, "%s: %lld soundings offered before", fn, (long long)offered);
  BGNN_REQUIRE(n <= capacity && offered <= capacity - n, "%s: %lld soundings after %lld offered before: more than the capacity of %lld",
               fn, (long long)n, (long long)offered, (long long)capacity);
  return BGNN_OK;
}

}  // namespace bgnn
