// The parts of the per-nucleus texture counts (nuctex.hip) that are plain C++ and run on the host as well: the constants of a record, the
// index of a cell of the upper triangle and the limits of the entry points.  Header-only and free of HIP calls, so a host program can
// exercise them under a sanitizer (tools/dev/nuctex_host_check.cpp); the kernel calls the same nuctex_cell.
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

// what is wrong with the sizes of a texture call, or null.  The frame is the one the morphometry takes (a full 1024-px frame holds
// 1024 x 1023 pairs an offset: every count fits an int32); pitch = pixels per tile row (>= W).
inline const char* nuctex_args_error(int B, int K, int H, int W, int pitch, int n_max, int channel_mode) {
  if (B < 1 || B > 4096 || K < 1 || K > 65536) return "nucleus_texture: B 1..4096, K 1..65536";
  if (H < 1 || H > NUCMORPH_MAX_SIDE || W < 1 || W > NUCMORPH_MAX_SIDE || pitch < W || pitch > NUCMORPH_MAX_SIDE) return "nucleus_texture: H and W 1..1024, row pitch W..1024";
  if (n_max < 1 || n_max > (1 << 24)) return "nucleus_texture: n_max 1..2^24";
  if (channel_mode != 0 && channel_mode != 1) return "nucleus_texture: channel_mode is NUHTC_CH_AS_IS or NUHTC_CH_SWAP";
  return nullptr;
}
