// The parts of the per-nucleus texture counts (nuctex.hip) that are plain C++ and run on the host as well: the constants of a record, the
// index of a cell of the upper triangle (the limits of the entry points are nucleus_sizes_error of nucleus_list.h).  Header-only, so a
// host program can exercise them under a sanitizer (tools/dev/nuctex_host_check.cpp); the kernel calls the same nuctex_cell.
#pragma once
#include <cstdint>

#include "nucmorph_host.h"

// a grey level is the haematoxylin value (0..255) >> NUCTEX_SHIFT; a record is NUCTEX_OFFSETS upper triangles of NUCTEX_CELLS int32
enum { NUCTEX_SHIFT = 4, NUCTEX_LEVELS = 16, NUCTEX_OFFSETS = 2, NUCTEX_CELLS = NUCTEX_LEVELS * (NUCTEX_LEVELS + 1) / 2,
       NUCTEX_ROW = NUCTEX_OFFSETS * NUCTEX_CELLS };
static_assert((256 >> NUCTEX_SHIFT) == NUCTEX_LEVELS && NUCTEX_CELLS == 136 && NUCTEX_ROW == 272, "16 levels over 0..255, 136 cells an offset");

// cell of the unordered pair of levels {a, b}, 0 <= a, b < NUCTEX_LEVELS: the upper triangle in row-major order
NUCMORPH_HD inline int nuctex_cell(int a, int b) {
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  return lo * NUCTEX_LEVELS - lo * (lo - 1) / 2 + (hi - lo);
}
