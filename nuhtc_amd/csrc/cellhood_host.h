// The parts of the cellular-neighbourhood kernels (cellhood.hip) that are plain C++ and run on the host as well -- everything of ITS OWN
// that decides a value, an index or a limit: the generator of the seeding draws, the pick rule on a prefix sum, the squared distance of two
// windows (seeding) and of a window to a centre (Lloyd), the rounding of a centre, the packing of a window into 16 bytes and the limits.
// Header-only, so a host program can exercise them under a sanitizer (tools/dev/cellhood_host_check.cpp); the kernels and the host-only
// exports nuhtc_neighbourhood_draws / nuhtc_neighbourhood_rule call the same functions.  nuhtc_amd/neighbourhoods.py defines every value.
//
// The budget, stated here once.  A window entry is a count of at most k + 1 <= 33 rows and fits a byte; C <= 14 of them fit 16 bytes.
// Seeding: (a - b)^2 <= 33^2 per class, and since both windows sum to at most 33 the distance is at most 2 * 33^2 = 2178; n <= 2^24 rows
// make T <= 2^24 * 2178 < 2^36: int64.  Lloyd: a centre is 0 .. 34000 (1024 * 33 = 33792 is the largest a fit makes), so
// |1024 w - q| <= 34000 and one squared term is below 2^31 (uint32); 14 terms are below 2^34 and are added in 64 bits; 2^24 rows are
// below 2^58.  The rounding takes s <= 2^24 * 33 < 2^30: 2 * 1024 * s + m < 2^42.  A workgroup of the assign kernel counts its rows in
// uint32 LDS counters: at most 2^24 * 33 < 2^30 per entry.
#pragma once
#include "cellenrich_host.h"

enum { HOOD_NT = 256, HOOD_MAX_K = 32, HOOD_MAX_TYPES = 32, HOOD_MAX_ITER = 1000, HOOD_LANES = 16, HOOD_FRAC_BITS = 10, HOOD_ONE = 1 << HOOD_FRAC_BITS,
       HOOD_MAX_CENTRE = 34000, HOOD_BATCH = 8, HOOD_PICK_NT = 1024 };
constexpr int64_t HOOD_MAX_POINTS = (int64_t)1 << 24;

// ---- a window as 16 bytes: byte c of (lo, hi) holds w[c], c < 14; the bytes 14 and 15 stay zero
struct alignas(16) HoodWin { unsigned long long lo, hi; };      // one 128-bit load per row
CELL_HD inline void hood_win_add(HoodWin& w, int label, int C) {   // a label outside 0 .. C - 1 (C <= 14) is counted in no class
  if ((unsigned)label >= (unsigned)C) return;
  if (label < 8) w.lo += 1ull << (8 * label);
  else w.hi += 1ull << (8 * (label - 8));
}
CELL_HD inline int hood_win_at(const HoodWin& w, int c) { return (int)(((c < 8 ? w.lo >> (8 * c) : w.hi >> (8 * (c - 8)))) & 0xffull); }

// ---- the generator: u_j, j = 0 .. K - 1
CELL_HD inline unsigned long long hood_draw(uint32_t seed, int j) {
  const uint32_t b = ce_fmix(seed + 0x9E3779B9u * (uint32_t)(j + 1));
  return ((unsigned long long)ce_fmix(b + 0x7F4A7C15u) << 32) | (unsigned long long)ce_fmix(b + 2u * 0x7F4A7C15u);
}

// ---- the pick rule: the element with exclusive prefix `before` and value `v` is the smallest one whose inclusive prefix exceeds t exactly
// when before <= t < before + v (the prefix never decreases; an element of value 0 is never picked)
CELL_HD inline bool hood_picks(long long before, long long v, long long t) { return before <= t && t < before + v; }
// on an inclusive prefix array: the smallest i with incl[i] > t, n when there is none
inline int64_t hood_pick_row(const int64_t* incl, int64_t n, int64_t t) {
  for (int64_t i = 0; i < n; ++i)
    if (hood_picks(i ? incl[i - 1] : 0, incl[i] - (i ? incl[i - 1] : 0), t)) return i;
  return n;
}

// ---- the squared distance of two windows in count units (seeding)
CELL_HD inline int hood_win_d2(const HoodWin& a, const HoodWin& b) {
  int d2 = 0;
#pragma unroll
  for (int c = 0; c < CELL_MAX_CLASSES; ++c) { const int d = hood_win_at(a, c) - hood_win_at(b, c); d2 += d * d; }
  return d2;
}

// ---- D: the squared distance of a window to a centre in fixed point; q has HOOD_LANES entries, zero from C on
CELL_HD inline unsigned long long hood_distance(const HoodWin& w, const int* q) {
  unsigned long long D = 0;
#pragma unroll
  for (int c = 0; c < CELL_MAX_CLASSES; ++c) {
    const int d = HOOD_ONE * hood_win_at(w, c) - q[c];           // |d| <= 34000: d * d < 2^31
    D += (unsigned long long)(unsigned)(d * d);
  }
  return D;
}

// ---- the update of one centre entry: floor((2 * 1024 * s + m) / (2 * m)), half up; an empty type keeps q
CELL_HD inline int hood_round(long long s, long long m, int q) { return m > 0 ? (int)((2 * (long long)HOOD_ONE * s + m) / (2 * m)) : q; }

// ---- the front checks of the entry point
inline bool hood_call_ok(int64_t n, int k, int num_classes, int num_types, int max_iter) {
  return n >= 0 && n <= HOOD_MAX_POINTS && k >= 1 && k <= HOOD_MAX_K && num_classes >= 1 && num_classes <= CELL_MAX_CLASSES && num_types >= 1 &&
         num_types <= HOOD_MAX_TYPES && max_iter >= 1 && max_iter <= HOOD_MAX_ITER;
}
CELL_HD inline bool hood_neighbour_ok(int j, int n) { return j >= -1 && j < n; }
inline bool hood_centre_ok(int q) { return q >= 0 && q <= HOOD_MAX_CENTRE; }
// the blocks of HOOD_NT rows, and how many of their sums one thread of the pick workgroup takes
CELL_HD inline int hood_blocks(int64_t n) { return (int)((n + HOOD_NT - 1) / HOOD_NT); }
CELL_HD inline int hood_pick_chunk(int nblk) { return (nblk + HOOD_PICK_NT - 1) / HOOD_PICK_NT; }
