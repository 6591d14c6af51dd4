// The parts of the pair-histogram kernels (cellspatial.hip) that are plain C++ and run on the host as well -- everything of ITS OWN that
// decides an index or a limit: the distance bin of a pair, the LDS carve of the search, the rotated column of the row sums and the check of
// the bin edges.  The grid, the keys and the pair distance it shares with the other per-slide analyses are in cellgrid_host.h.
// Header-only, so a host program can exercise them under a sanitizer (tools/dev/cellspatial_host_check.cpp); the kernels call the same
// functions.  nuhtc_amd/spatial.py defines every value.
#pragma once
#include "cellgrid_host.h"

enum { CS_NT = 256, CS_MAX_BINS = 32, CS_MAX_CLASSES = CELL_MAX_CLASSES, CS_MAX_EDGE = CELL_MAX_REACH };
constexpr int CS_MAX_CELLS = 1 << 18;                  // cells of the pair-histogram grid: (2^18 cells) x (C + 1 <= 15 keys) < 2^22 table entries
constexpr int CS_NO_EDGE = 0x7fffffff;                 // fills the table of squared edges behind bin B - 1: no d2 (<= 2^29) exceeds it

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

// ---- the bin edges of the entry point, checked before anything is launched (cell_call_ok takes e_B as the reach); on success e2 holds
// the padded table of squared edges
inline bool cs_edges_ok(const int32_t* edges, int B, int e2[CS_MAX_BINS]) {
  if (B < 1 || B > CS_MAX_BINS || !edges) return false;
  for (int t = 0; t < B; ++t)
    if (edges[t] < 1 || edges[t] > CS_MAX_EDGE || (t && edges[t] <= edges[t - 1])) return false;
  for (int t = 0; t < CS_MAX_BINS; ++t) e2[t] = t < B ? edges[t] * edges[t] : CS_NO_EDGE;      // <= 2^28
  return true;
}
