// The parts of the uniform-grid point kernels (cellbin.h, cellgraph.hip, cellspatial.hip) that are plain C++ and run on the host as well --
// everything that decides an index or a limit: the grid geometry over the bounding box, the cell and the (cell, class) key of a point,
// the distance bin of a pair, the LDS carve of the pair-histogram search, and the limits of nuhtc_cell_spatial.  Header-only, so a host
// program can exercise them under a sanitizer (tools/dev/cellspatial_host_check.cpp); the kernels call the same functions.
// nuhtc_amd/spatial.py and nuhtc_amd/cellgraph.py define every value.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define CELL_HD __host__ __device__
#else
#define CELL_HD
#endif

enum { CS_NT = 256, CS_MAX_BINS = 32, CS_MAX_CLASSES = 14, CS_MAX_EDGE = 16384 };
constexpr int CELL_COORD_LIMIT = 1 << 27;              // |p| < 2^27 half pixels
constexpr int64_t CELL_MAX_POINTS = (int64_t)1 << 28;
constexpr int CS_MAX_CELLS = 1 << 18;                  // cells of the pair-histogram grid: (2^18 cells) x (C + 1 <= 15 keys) < 2^22 table entries
constexpr int CS_NO_EDGE = 0x7fffffff;                 // fills the table of squared edges behind bin B - 1: no d2 (<= 2^29) exceeds it

// ---- grid geometry over the inclusive bounding box
CELL_HD inline long long cell_cells_along(int lo, int hi, long long side) { return ((long long)hi - lo) / side + 1; }

// the cell side: the smallest multiple m * r of the reach r whose grid over the box has at most max_cells cells, so side >= r and the
// 3 x 3 cells around a point hold its whole disc.  The cell count does not grow with m: bisection; at hi the grid is one cell.
inline int cell_grid_side(int x_min, int y_min, int x_max, int y_max, int r, int max_cells) {
  long long lo = 1, hi = (1LL << 29) / r + 1;
  while (lo < hi) {
    const long long m = (lo + hi) / 2;
    if (cell_cells_along(x_min, x_max, m * r) * cell_cells_along(y_min, y_max, m * r) <= max_cells) hi = m; else lo = m + 1;
  }
  return (int)(lo * r);
}

// the cell of a point INSIDE the box (the caller has compared it with the box)
CELL_HD inline int cell_index(int x, int y, int x_min, int y_min, int side, int ncx) { return ((y - y_min) / side) * ncx + (x - x_min) / side; }

// ---- the class of a label among C classes: itself, or C for a label outside 0 .. C - 1 (counted in no row and no column)
CELL_HD inline int cs_class(int label, int C) { return (unsigned)label < (unsigned)C ? label : C; }

// the counting-sort key: `sub` keys per cell.  sub == 1: the cell alone (the cell graph); sub == C + 1: (cell, class)
CELL_HD inline int cell_key(int cell, int label, int sub) { return sub == 1 ? cell : cell * sub + cs_class(label, sub - 1); }

// ---- the bin of a pair: the smallest t with d2 <= e2[t], for a d2 that is known to be <= e2[B - 1].  e2 holds the B squared edges,
// strictly increasing, and CS_NO_EDGE from B to 31.  Branch-free lower bound over e2[0 .. 30] (entry 31 is never needed: t <= B - 1 <= 31),
// five compares: t = the number of edges below d2.
CELL_HD inline int cs_bin_of(const int* e2, int d2) {
  int t = 0;
#pragma unroll
  for (int step = 16; step >= 1; step >>= 1) t += d2 > e2[t + step - 1] ? step : 0;
  return t;
}

// ---- the LDS of one search workgroup (CS_NT threads), carved in this order; every offset is a multiple of 16 bytes:
//   table  uint64 [C][C][B]      the workgroup's pair counts, entry (a, b, t) at cs_table_at
//   priv   uint32 [B][CS_NT]     the private bin counters of every thread, slot-major: counter t of thread tid at cs_priv_at
//   e2     int32  [32]           the squared edges, padded with CS_NO_EDGE
//   cls    int32  [CS_NT]        the class of every thread's query point (C: none)
//   cn     uint32 [16]           the workgroup's class census
CELL_HD inline int cs_table_at(int a, int b, int t, int C, int B) { return (a * C + b) * B + t; }
CELL_HD inline int cs_priv_at(int t, int tid) { return t * CS_NT + tid; }
CELL_HD inline int cs_lds_priv_off(int C, int B) { return (C * C * B * 8 + 15) & ~15; }
CELL_HD inline int cs_lds_e2_off(int C, int B) { return cs_lds_priv_off(C, B) + B * CS_NT * 4; }
CELL_HD inline int cs_lds_cls_off(int C, int B) { return cs_lds_e2_off(C, B) + 32 * 4; }
CELL_HD inline int cs_lds_cn_off(int C, int B) { return cs_lds_cls_off(C, B) + CS_NT * 4; }
CELL_HD inline int cs_lds_bytes(int C, int B) { return cs_lds_cn_off(C, B) + 16 * 4; }

// the column of its own wave that lane `lane` reads in step jj of the row sums: rotated by the lane, so the 32 lanes of a half wave
// (rows t = lane, CS_NT words apart: one bank) read 32 different banks
CELL_HD inline int cs_rotated_column(int jj, int lane) { return (jj + lane) & 63; }

// ---- the limits of the entry point, checked before anything is launched; on success e2 holds the padded table of squared edges
inline bool cs_args_ok(int64_t n, int C, const int32_t* edges, int B, int e2[CS_MAX_BINS]) {
  if (n < 0 || n > CELL_MAX_POINTS || C < 1 || C > CS_MAX_CLASSES || B < 1 || B > CS_MAX_BINS || !edges) return false;
  for (int t = 0; t < B; ++t)
    if (edges[t] < 1 || edges[t] > CS_MAX_EDGE || (t && edges[t] <= edges[t - 1])) return false;
  for (int t = 0; t < CS_MAX_BINS; ++t) e2[t] = t < B ? edges[t] * edges[t] : CS_NO_EDGE;      // <= 2^28
  return true;
}
inline bool cell_box_ok(int x_min, int y_min, int x_max, int y_max) {
  return x_min <= x_max && y_min <= y_max && x_min > -CELL_COORD_LIMIT && y_min > -CELL_COORD_LIMIT && x_max < CELL_COORD_LIMIT && y_max < CELL_COORD_LIMIT;
}
