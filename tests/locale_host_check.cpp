// The window selection of the locale guide (csrc/locale_window.h) on the host, without HIP, against a sort: windows of every size
// 0 .. 288 (radius 8 holds 288 cells beside its own) at every number of witnesses for the small ones and a spread of numbers for
// the large, values in a narrow range (ties), all equal, over the full +-(2^32 - 1) and at the two ends alone; k even and odd;
// min_support at k, k + 1 and 1; windows clipped at all four corners and all four edges of an image, with marks and witnesses
// outside the window that must not be read into it; a wild value at the cell itself; the one rounding of the conversion.
// tests/test_host_locale_window.py compiles this with -fsanitize=address,undefined and runs it; it prints "ok <windows checked>"
// and returns 0, or says what differs.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../bathymetric-gnn_amd/csrc/locale_window.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t next_u64() {                                  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

const int64_t TOP = 4294967295ll;                      // 2^32 - 1: the widest witness value
long long checked = 0;

enum Values { NARROW, EQUAL, FULL, ENDS };

int64_t draw(Values how) {
  switch (how) {
    case NARROW: return (int64_t)(next_u64() % 16) - 8;
    case EQUAL: return -123456789;
    case FULL: return (int64_t)(next_u64() % (2 * (uint64_t)TOP + 1)) - TOP;
    default: return next_u64() & 1 ? TOP : -TOP;
  }
}

[[noreturn]] void fail(const char *what, int rows, int cols, int k, long long got, long long want) {
  std::printf("%s differs: a window of %d x %d with %d witnesses: %lld, %lld expected\n", what, rows, cols, k, got, want);
  std::exit(1);
}

// An image of ih x iw whose window is rows r0 .. r1, columns c0 .. c1 with the cell itself at (sr, sc) inside it.  `witnesses` of
// the window's other cells hold values, the rest marks; everything outside the window, and the cell itself, holds what must not
// count: values below and above every witness, and marks.
void check_window(int ih, int iw, int r0, int r1, int c0, int c1, int sr, int sc, int witnesses, Values how) {
  std::vector<int64_t> image((size_t)ih * iw);
  for (auto &v : image) v = next_u64() % 3 == 0 ? bgnn::LOCALE_NO_WITNESS : (next_u64() & 1 ? TOP : -TOP);
  const int self = sr * iw + sc;
  std::vector<int> cells;
  for (int r = r0; r <= r1; ++r)
    for (int c = c0; c <= c1; ++c)
      if (r * iw + c != self) cells.push_back(r * iw + c);
  for (size_t i = cells.size(); i > 1; --i) std::swap(cells[i - 1], cells[next_u64() % i]);
  std::vector<int64_t> w;
  for (size_t i = 0; i < cells.size(); ++i) {
    const bool is_w = (int)i < witnesses;
    image[cells[i]] = is_w ? draw(how) : bgnn::LOCALE_NO_WITNESS;
    if (is_w) w.push_back(image[cells[i]]);
  }
  std::sort(w.begin(), w.end());
  const int k = (int)w.size();
  const int rows = r1 - r0 + 1, cols = c1 - c0 + 1;
  for (int min_support : {1, k, k + 1}) {
    if (min_support < 1) continue;
    const int64_t untouched = 0x5555555555555555ll;
    int64_t med2 = untouched;
    const int32_t got = bgnn::locale_window(image.data(), iw, r0, r1, c0, c1, self, min_support, &med2);
    if (got != k) fail("the support", rows, cols, k, got, k);
    const uint32_t bits = bgnn::locale_guide_bits(got, min_support, med2);
    if (k < min_support) {
      if (med2 != untouched) fail("med2 under min_support", rows, cols, k, (long long)med2, (long long)untouched);
      if (bits != 0x7FC00000u) fail("the NaN", rows, cols, k, bits, 0x7FC00000u);
    } else {
      const int64_t want = w[(k - 1) / 2] + w[k / 2];
      if (med2 != want) fail("med2", rows, cols, k, (long long)med2, (long long)want);
      const float g = (float)((double)want / 262144.0);
      uint32_t want_bits;
      std::memcpy(&want_bits, &g, 4);
      if (bits != want_bits) fail("the guide's bits", rows, cols, k, bits, want_bits);
    }
    ++checked;
  }
}

}  // namespace

int main() {
  // every window size 0 .. 288 as the widest rectangle that holds it: the cell itself in the middle of a (2R + 1)^2 window cut
  // down row by row and column by column, so that sizes between the squares appear as clipped windows do
  bool seen[289] = {false};
  for (int R = 1; R <= 8; ++R)
    for (int up = 0; up <= R; ++up)
      for (int left = 0; left <= R; ++left)
        for (int down : {0, R})
          for (int right : {0, R}) {                   // the four corners: (up, left) clipped with (down, right) whole, and so on
            const int rows = up + 1 + down, cols = left + 1 + right, size = rows * cols - 1;
            seen[size] = true;
            const int ih = rows + 2, iw = cols + 3;    // a margin of cells that are not the window's
            for (Values how : {NARROW, EQUAL, FULL, ENDS}) {
              const int step = size <= 24 ? 1 : 1 + size / 7;
              for (int witnesses = 0; witnesses <= size; witnesses += step) check_window(ih, iw, 1, rows, 1, cols, 1 + up, 1 + left, witnesses, how);
              if (size) check_window(ih, iw, 1, rows, 1, cols, 1 + up, 1 + left, size, how);
              if (size > 1) check_window(ih, iw, 1, rows, 1, cols, 1 + up, 1 + left, size - 1, how);
            }
          }
  // the sizes that no such rectangle has: a row of 1 x (size + 1) with the cell itself anywhere
  for (int size = 0; size <= 288; ++size) {
    for (Values how : {NARROW, EQUAL, FULL, ENDS})
      for (int witnesses : {0, 1, 2, size / 2, size - 1, size})
        if (witnesses >= 0 && witnesses <= size) check_window(3, size + 3, 1, 1, 1, size + 1, 1, 1 + (int)(next_u64() % (size + 1)), witnesses, how);
    seen[size] = true;
  }
  for (int size = 0; size <= 288; ++size)
    if (!seen[size]) { std::printf("no window of size %d\n", size); return 1; }
  // the full 17 x 17 window inside the largest image of the kernel (24 x 48), dense
  for (int i = 0; i < 16; ++i) check_window(24, 48, 3, 19, 20, 36, 11, 28, 288 - i, i & 1 ? FULL : NARROW);
  // the one rounding: 2^33 - 2 is no float32 and no float32 after a rounding to 24 bits first would differ; 32768.0 comes out
  if (bgnn::locale_guide_bits(2, 1, 2 * TOP) != 0x47000000u || bgnn::locale_guide_bits(2, 1, -2 * TOP) != 0xC7000000u) {
    std::printf("the guide of +-(2^33 - 2) is not +-32768.0\n");
    return 1;
  }
  if (bgnn::locale_guide_bits(1, 1, (1ll << 25) + 1) != 0x43000000u) {               // 128 + 2^-18: rounds down to 128.0
    std::printf("the guide of 2^25 + 1\n");
    return 1;
  }
  std::printf("ok %lld\n", checked);
  return 0;
}
