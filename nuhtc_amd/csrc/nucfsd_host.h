// The parts of the per-nucleus Fourier-descriptor integers (nucfsd.hip) that are plain C++ and run on the host as well -- everything that
// decides a sign, an index or a limit: the constants of a row, the classifier of one edge of a ring, the exact sign of p + q sqrt 2, the
// search of a sample's edge in one chunk of cumulative step counts, and the limits of the entry point.  Header-only, so a host program
// can exercise them under a sanitizer (tools/dev/nucfsd_host_check.cpp); the kernel calls the same functions.  nuhtc_amd/nucfsd.py
// defines every value.
#pragma once
#include <cstdint>

#include "nucmorph_host.h"

// a row: status, A, B, n, then x_e y_e d_e a_e b_e of the edge that holds sample k = 0 .. 127
enum { NUCFSD_K = 128, NUCFSD_HEAD = 4, NUCFSD_PER = 5, NUCFSD_ROW = NUCFSD_HEAD + NUCFSD_PER * NUCFSD_K, NUCFSD_CHUNK = 256 };
enum { NUCFSD_OK = 0, NUCFSD_DEGENERATE = 1, NUCFSD_NOT_TRACED = 2, NUCFSD_TOO_LONG = 3 };
constexpr int64_t NUCFSD_MAX_STEPS = (int64_t)1 << 24;        // A + B of a measured ring: every cumulative count fits an int32, and see nucfsd_sign
constexpr int64_t NUCFSD_MAX_VERTS = (int64_t)1 << 30;       // nv of the entry point: a ring's vertex count, and an edge index plus a chunk, fit an int32
static_assert(NUCFSD_ROW == 644, "644 words a row");

// ---- one edge (dx, dy) of a ring, |dx| and |dy| below 2^32: false when it is off the eight chain directions; otherwise its unit steps,
// whether they are diagonal, and its Freeman code (0 = east, counter-clockwise on the screen as in contour.hip; 0 for no step)
NUCMORPH_HD inline bool nucfsd_edge(int64_t dx, int64_t dy, int64_t& steps, bool& diagonal, int& code) {
  const int64_t ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
  diagonal = ax != 0 && ay != 0;
  steps = ax > ay ? ax : ay;
  const int sx = (dx > 0) - (dx < 0), sy = (dy > 0) - (dy < 0);
  // one nibble per (sy, sx), row-major from (-1, -1): 3 2 1 / 4 0 0 / 5 6 7
  code = (int)((0x765004123ull >> (4 * ((sy + 1) * 3 + sx + 1))) & 7);
  return !diagonal || ax == ay;
}

// ---- the sign of p + q sqrt 2, exactly.  Where p and q do not contradict each other that is their sign; otherwise p q < 0 and the sign
// is that of p times that of p^2 - 2 q^2, which is never 0 for non-zero integers.  The squares are formed only there: with
// |p|, |q| <= 2^7 (2^24 - 1) (nucfsd.py: A + B <= 2^24 and both at least 1) p^2 < 2^62 and 2 q^2 < 2^63.
NUCMORPH_HD inline int nucfsd_sign(int64_t p, int64_t q) {
  if (p >= 0 && q >= 0) return (p | q) != 0;
  if (p <= 0 && q <= 0) return -1;
  const int64_t pp = p * p, qq = 2 * q * q;
  return (pp > qq) == (p > 0) ? 1 : -1;
}

// does the length a + b sqrt 2 lie at or before sample k of a ring of A axial and B diagonal steps, i.e. a + b sqrt 2 <= (k / K) (A + B sqrt 2)?
NUCMORPH_HD inline bool nucfsd_at_or_before(int a, int b, int k, int64_t A, int64_t B) {
  return nucfsd_sign((int64_t)NUCFSD_K * a - (int64_t)k * A, (int64_t)NUCFSD_K * b - (int64_t)k * B) <= 0;
}

// ---- the last j in 0 .. m - 1 whose start length ca[j] + cb[j] sqrt 2 lies at or before sample k.  The lengths do not decrease with j
// and entry 0 is known to qualify; m >= 1.  Reads ca and cb only inside [0, m).
NUCMORPH_HD inline int nucfsd_search(const int* ca, const int* cb, int m, int k, int64_t A, int64_t B) {
  int lo = 0, hi = m;                                          // lo qualifies, hi does not (or is m)
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (nucfsd_at_or_before(ca[mid], cb[mid], k, A, B)) lo = mid; else hi = mid;
  }
  return lo;
}

// the limits of the entry point: n rings of nv vertices in all
inline bool nucfsd_args_ok(int64_t nv, int n) { return nv >= 1 && nv <= NUCFSD_MAX_VERTS && n >= 1 && n <= 4096; }
