// The address function of the variable-resolution sounding gridders (csrc/sounding_vr_cell.h) on the host, without HIP: reads
// cases "x y x0 y0 B BH BW index dx dy total" (the floats in any form strtod takes: hex floats, nan, inf) from the file named on
// the command line; the entry (index, dx, dy) is that of the sounding's base cell, whichever that is.  Prints per case the base
// cell (-1: off the base grid), whether the entry is a refinement grid inside `total` records, and the record (-1 where there is
// none).  tests/test_host_vr_soundings.py compiles this with -fsanitize=address,undefined, writes the cases and compares the
// answers with the numpy restatement.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "../bathymetric-gnn_amd/csrc/sounding_vr_cell.h"

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 3;
  char line[1024];
  while (std::fgets(line, sizeof line, f)) {
    char *p = line;
    double v[5];
    for (double &d : v) d = std::strtod(p, &p);
    const long long BH = std::strtoll(p, &p, 10), BW = std::strtoll(p, &p, 10);
    bgnn::VRLayoutEntry e;
    e.index = std::strtoll(p, &p, 10);
    e.dx = (int32_t)std::strtol(p, &p, 10);
    e.dy = (int32_t)std::strtol(p, &p, 10);
    const long long total = std::strtoll(p, &p, 10);
    double fu = 0.0, fv = 0.0;
    const int64_t b = bgnn::vr_base_cell(v[0], v[1], v[2], v[3], v[4], BH, BW, &fu, &fv);
    const bool refined = b >= 0 && bgnn::vr_entry_refined(e, total);
    std::printf("%" PRId64 " %d %" PRId64 "\n", b, refined ? 1 : 0, refined ? bgnn::vr_record(e, fu, fv) : (int64_t)-1);
  }
  std::fclose(f);
  return 0;
}
