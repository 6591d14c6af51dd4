// The parts of the per-nucleus shape integers (nucshape.hip) that are plain C++ and run on the host as well -- everything that decides an
// index or a limit: the constants of a row, the geometry of the box pyramid (rows and words of a level, where a level lies in LDS), the
// read of one mask word aligned to the rectangle's corner, the pair-compress of a word, the two front levels from four aligned rows, a
// further level from its four child words, and the limits of the entry point (nucleus_sizes_error of nucleus_list.h).  Header-only, so a
// host program can exercise them under a sanitizer (tools/dev/nucshape_host_check.cpp); the kernel calls the same functions.
// nuhtc_amd/nucshape.py defines every value.
#pragma once
#include <cstdint>
#include <string>

#include "nucmorph_host.h"

// a row: A, x0 y0 x1 y1 (x1, y1 exclusive), Sx Sy Sxx Sxy Syy, Sxxx Sxxy Sxyy Syyy, N_1 .. N_10 (box side 2^j)
enum { NUCSHAPE_RECT = 1, NUCSHAPE_SUMS = 5, NUCSHAPE_NSUMS = 9, NUCSHAPE_BOXES = 14, NUCSHAPE_LEVELS = 10,
       NUCSHAPE_ROW = NUCSHAPE_BOXES + NUCSHAPE_LEVELS };
static_assert(NUCSHAPE_ROW == 24 && (1 << NUCSHAPE_LEVELS) == NUCLEUS_MAX_SIDE, "24 words a row; the largest box holds the largest frame");
static_assert(1024.0 * 1024 * 1023 * 1023 * 1023 < 9.2e18, "a third-order sum of a full 1024-px frame fits an int64");

// ---- the pyramid of a w x h rectangle (1 .. 1024 each): level L = 1 .. 10 has one bit per box of side 2^L anchored at the rectangle's
// corner, nucshape_rows x nucshape_bits of them, a row in nucshape_words 32-bit words whose unused high bits are zero
NUCMORPH_HD inline int nucshape_rows(int h, int L) { return (h + (1 << L) - 1) >> L; }
NUCMORPH_HD inline int nucshape_bits(int w, int L) { return (w + (1 << L) - 1) >> L; }
NUCMORPH_HD inline int nucshape_words(int w, int L) { return (nucshape_bits(w, L) + 31) >> 5; }
// levels 2 .. 10 are kept (level 1 lives in registers only): the words of level L start at nucshape_base(L) of a plane of
// NUCSHAPE_PLANE words, each level sized for the 1024-px rectangle -- 256 x 8, 128 x 4, 64 x 2, 32, 16, 8, 4, 2, 1
NUCMORPH_HD constexpr int nucshape_level_words(int L) { return (NUCLEUS_MAX_SIDE >> L) * ((NUCLEUS_MAX_SIDE >> L) >= 32 ? (NUCLEUS_MAX_SIDE >> L) / 32 : 1); }
NUCMORPH_HD constexpr int nucshape_base(int L) { return L <= 2 ? 0 : nucshape_base(L - 1) + nucshape_level_words(L - 1); }
enum { NUCSHAPE_PLANE = nucshape_base(NUCSHAPE_LEVELS) + nucshape_level_words(NUCSHAPE_LEVELS) };
static_assert(nucshape_level_words(2) == 2048 && nucshape_level_words(5) == 32 && nucshape_level_words(10) == 1 && NUCSHAPE_PLANE == 2751, "the kept levels");

// ---- word a (0, 1, ..) of a mask row aligned to the rectangle's corner: the bits x0 + 32 a .. x0 + 32 a + 31 of the row.  row: the
// wpr words of one mask row; wx1: the last word the rectangle touches (<= wpr - 1) -- words behind it hold no set pixel and are not
// read; last: the bits of word wpr - 1 that are pixels (the padding bits are masked off on every read).
NUCMORPH_HD inline uint32_t nucshape_mask_word(const uint32_t* row, int cw, int wx1, int wpr, uint32_t last) {
  if (cw > wx1) return 0u;
  const uint32_t v = row[cw];
  return cw == wpr - 1 ? v & last : v;
}
NUCMORPH_HD inline uint32_t nucshape_aligned_word(const uint32_t* row, int x0, int a, int wx1, int wpr, uint32_t last) {
  const int cw = (x0 >> 5) + a;
  const uint64_t two = (uint64_t)nucshape_mask_word(row, cw, wx1, wpr, last) | ((uint64_t)nucshape_mask_word(row, cw + 1, wx1, wpr, last) << 32);
  return (uint32_t)(two >> (x0 & 31));          // the funnel shift across two adjacent words
}

// ---- pair-compress: bit i of the result is the OR (the AND) of the bits 2 i and 2 i + 1 of v
NUCMORPH_HD inline uint32_t nucshape_even_bits(uint64_t t) {      // the bits 0, 2, 4, .. of t (its odd bits are zero) packed into 32
  t = (t | (t >> 1)) & 0x3333333333333333ull;
  t = (t | (t >> 2)) & 0x0f0f0f0f0f0f0f0full;
  t = (t | (t >> 4)) & 0x00ff00ff00ff00ffull;
  t = (t | (t >> 8)) & 0x0000ffff0000ffffull;
  return (uint32_t)(t | (t >> 16));
}
NUCMORPH_HD inline uint32_t nucshape_pair_any(uint64_t v) { return nucshape_even_bits((v | (v >> 1)) & 0x5555555555555555ull); }
NUCMORPH_HD inline uint32_t nucshape_pair_all(uint64_t v) { return nucshape_even_bits((v & (v >> 1)) & 0x5555555555555555ull); }
// classify: the boxes of a word that hold a set pixel and an unset position
NUCMORPH_HD inline int nucshape_mixed(uint32_t any, uint32_t all) { return __builtin_popcount(any & ~all); }

// ---- one parent word from its four child words (two adjacent words of two adjacent child rows; a child outside the level is 0):
// any = OR, all = AND
NUCMORPH_HD inline void nucshape_parent(uint32_t any00, uint32_t any01, uint32_t any10, uint32_t any11, uint32_t all00, uint32_t all01,
                                        uint32_t all10, uint32_t all11, uint32_t& any, uint32_t& all) {
  any = nucshape_pair_any((uint64_t)(any00 | any10) | ((uint64_t)(any01 | any11) << 32));
  all = nucshape_pair_all((uint64_t)(all00 & all10) | ((uint64_t)(all01 & all11) << 32));
}

// ---- the two front levels from the mask: px[r][a], the aligned words a = 0 .. 3 (128 pixels) of four adjacent aligned rows r (zero
// where the row lies below the rectangle) -> word (any2, all2) of level 2 (32 boxes of side 4) and the mixed boxes of levels 1 and 2
NUCMORPH_HD inline void nucshape_front(const uint32_t px[4][4], uint32_t& any2, uint32_t& all2, int& n1, int& n2) {
  uint32_t any1[2][2], all1[2][2];                 // level 1: two rows of 64 boxes of side 2; a pixel is its own any and all
  n1 = 0;
  for (int t = 0; t < 2; ++t)
    for (int c = 0; c < 2; ++c) {
      nucshape_parent(px[2 * t][2 * c], px[2 * t][2 * c + 1], px[2 * t + 1][2 * c], px[2 * t + 1][2 * c + 1],
                      px[2 * t][2 * c], px[2 * t][2 * c + 1], px[2 * t + 1][2 * c], px[2 * t + 1][2 * c + 1], any1[t][c], all1[t][c]);
      n1 += nucshape_mixed(any1[t][c], all1[t][c]);
    }
  nucshape_parent(any1[0][0], any1[0][1], any1[1][0], any1[1][1], all1[0][0], all1[0][1], all1[1][0], all1[1][1], any2, all2);
  n2 = nucshape_mixed(any2, all2);
}

// what is wrong with the arguments of the entry point, or empty (no tiles: the pitch is W, the channel mode the default)
inline std::string nucshape_args_error(int B, int K, int H, int W, int n_max) {
  return nucleus_sizes_error("nucleus_shape", B, K, H, W, W, n_max, 0);
}
