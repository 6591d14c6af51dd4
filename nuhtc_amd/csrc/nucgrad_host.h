// The parts of the per-nucleus gradient integers (nucgrad.hip) that are plain C++ and run on the host as well -- everything that decides an
// index or a limit: the constants of a row, the two pixels a doubled central difference reads and its weight, the exact integer root, the
// direction sector of the edge test with its two neighbours, the histogram bin, and the limits of the entry point (nucleus_sizes_error of
// nucleus_list.h and the threshold).  Header-only, so a host program can exercise them under a sanitizer
// (tools/dev/nucgrad_host_check.cpp); the kernel calls the same functions.  nuhtc_amd/nucgrad.py defines every value.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

#include "nucmorph_host.h"

// a row: A, S1..S4, mn, mx, n_edge, hist[NUCGRAD_BINS]; m = isqrt(4 q) is at most NUCGRAD_M_MAX (q <= 2 * 510^2)
enum { NUCGRAD_BINS = 10, NUCGRAD_HIST = 8, NUCGRAD_ROW = NUCGRAD_HIST + NUCGRAD_BINS, NUCGRAD_M_MAX = 1442, NUCGRAD_Q_MAX = 2 * 510 * 510,
       NUCGRAD_TAN_22 = 13573 };
static_assert(NUCGRAD_ROW == 18 && NUCGRAD_Q_MAX == 520200, "18 words a row; the largest squared doubled gradient");
static_assert(1442ll * 1442 <= 4ll * NUCGRAD_Q_MAX && 4ll * NUCGRAD_Q_MAX < 1443ll * 1443, "the largest magnitude");
static_assert(1024.0 * 1024 * 1442 * 1442 * 1442 * 1442 < 9.2e18, "S4 of a full 1024-px frame fits an int64");

// the doubled difference at position i of an axis of n pixels is (h[nucgrad_hi(i, n)] - h[nucgrad_lo(i)]) * nucgrad_weight(i, n): the
// central difference inside, twice the one-sided difference at both ends, 0 for n == 1 (both reads are pixel 0).  0 <= i < n.
NUCMORPH_HD inline int nucgrad_lo(int i) { return i > 0 ? i - 1 : 0; }
NUCMORPH_HD inline int nucgrad_hi(int i, int n) { return i + 1 < n ? i + 1 : n - 1; }
NUCMORPH_HD inline int nucgrad_weight(int i, int n) { return (i == 0 || i == n - 1) ? 2 : 1; }

// m = floor(sqrt(4 q)), 0 <= q <= NUCGRAD_Q_MAX: 4 q < 2^24 is exact in fp32, the rounded root is off by at most one either way
NUCMORPH_HD inline int nucgrad_mag(int q) {
  const int v = 4 * q;
  int r = (int)sqrtf((float)v);
  if (r * r > v) --r;
  else if ((r + 1) * (r + 1) <= v) ++r;
  return r;
}

// the sector of the doubled gradient (gx2, gy2), OpenCV's integer rule: 0 horizontal, 1 vertical, 2 the diagonal of equal signs, 3 the
// other diagonal; |g| <= 510, so every product stays below 2^26
NUCMORPH_HD inline int nucgrad_sector(int gx2, int gy2) {
  const int ax = gx2 < 0 ? -gx2 : gx2, ay = gy2 < 0 ? -gy2 : gy2;
  if ((ay << 15) < ax * NUCGRAD_TAN_22) return 0;
  if ((ay << 15) > ax * NUCGRAD_TAN_22 + (ax << 16)) return 1;
  return gx2 * gy2 > 0 ? 2 : 3;
}
// the step from a pixel to the FIRST neighbour of its sector (the second is the opposite step): q(p) > q(first) and q(p) >= q(second)
NUCMORPH_HD inline void nucgrad_step(int sector, int& dx, int& dy) {
  dx = sector == 1 ? 0 : (sector == 3 ? 1 : -1);
  dy = sector == 0 ? 0 : -1;
}

// numpy's np.histogram(m, bins=10) over [mn, mx] in integers; mn <= m <= mx
NUCMORPH_HD inline int nucgrad_bin(int m, int mn, int mx) {
  if (mx == mn) return NUCGRAD_BINS / 2;
  const int b = (m - mn) * NUCGRAD_BINS / (mx - mn);
  return b < NUCGRAD_BINS - 1 ? b : NUCGRAD_BINS - 1;
}

// what is wrong with the arguments of the entry point, or empty
inline std::string nucgrad_args_error(int B, int K, int H, int W, int pitch, int n_max, int channel_mode, int edge_thr) {
  const std::string why = nucleus_sizes_error("nucleus_gradient", B, K, H, W, pitch, n_max, channel_mode);
  if (!why.empty()) return why;
  if (edge_thr < 1 || edge_thr > NUCGRAD_M_MAX) return "nucleus_gradient: edge_thr 1..1442 (quarter grey levels)";
  return std::string();
}
