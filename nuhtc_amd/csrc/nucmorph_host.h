// The part of the per-nucleus morphometry (nucmorph.hip) that is plain C++ and runs on the host as well: one side of the convex hull
// (the limits of the entry points are nucleus_sizes_error of nucleus_list.h).  Header-only, so a host program can exercise it under a
// sanitizer (tools/dev/nucmorph_host_check.cpp); the kernel calls the same hull_chain2.
#pragma once
#include <cstdint>

#include "nucleus_list.h"

#if defined(__HIPCC__)
#define NUCMORPH_HD __host__ __device__
#else
#define NUCMORPH_HD
#endif

enum { NUCMORPH_MAX_SIDE = NUCLEUS_MAX_SIDE, NUCMORPH_RAW = 16, NUCMORPH_BINS = 256 };
constexpr uint32_t NUCMORPH_EMPTY_ROW = 0xffffffffu;

// One side of the convex hull of the pixel corners of a mask, as twice the integral over Y of that side's x: ext[i] = l | r << 16, the
// leftmost and rightmost set pixel of pixel row i of the bounding rectangle (NUCMORPH_EMPTY_ROW: none), rows >= 1 of them.  Lattice row
// Y = 0 .. rows carries the corners of the pixel rows Y - 1 and Y: the smallest l (left side) or the largest r + 1 (right side).  One
// monotone chain over those points with integer cross products (all below 2^21), on a stack `st` of rows + 1 entries (x << 16 | Y);
// returns sum (x_i + x_i+1) (Y_i+1 - Y_i) over the chain.  hull2 = right - left.
template <bool RIGHT>
NUCMORPH_HD inline long long hull_chain2(const uint32_t* ext, int rows, uint32_t* st) {
  int n = 0;
  for (int Y = 0; Y <= rows; ++Y) {
    const uint32_t a = Y > 0 ? ext[Y - 1] : NUCMORPH_EMPTY_ROW, b = Y < rows ? ext[Y] : NUCMORPH_EMPTY_ROW;
    if (a == NUCMORPH_EMPTY_ROW && b == NUCMORPH_EMPTY_ROW) continue;
    int x;
    if (RIGHT) {
      const int xa = a == NUCMORPH_EMPTY_ROW ? 0 : (int)(a >> 16) + 1, xb = b == NUCMORPH_EMPTY_ROW ? 0 : (int)(b >> 16) + 1;
      x = xa > xb ? xa : xb;
    } else {
      const int xa = a == NUCMORPH_EMPTY_ROW ? 0xffff : (int)(a & 0xffffu), xb = b == NUCMORPH_EMPTY_ROW ? 0xffff : (int)(b & 0xffffu);
      x = xa < xb ? xa : xb;
    }
    while (n >= 2) {
      const int ax = (int)(st[n - 2] >> 16), ay = (int)(st[n - 2] & 0xffffu), bx = (int)(st[n - 1] >> 16), by = (int)(st[n - 1] & 0xffffu);
      const int lhs = (bx - ax) * (Y - by), rhs = (x - bx) * (by - ay);
      if (RIGHT ? lhs <= rhs : lhs >= rhs) --n; else break;
    }
    st[n++] = ((uint32_t)x << 16) | (uint32_t)Y;
  }
  long long sum = 0;
  for (int i = 0; i + 1 < n; ++i)
    sum += (long long)((int)(st[i] >> 16) + (int)(st[i + 1] >> 16)) * ((int)(st[i + 1] & 0xffffu) - (int)(st[i] & 0xffffu));
  return sum;
}
