// What the host checks of the site rasters share (celldensity_host_check.cpp, cellterritory_host_check.cpp): the grid of cellbin.h laid
// on the host, and the walk of site_sweep (nuhtc_amd/csrc/cellsites.h) over it -- the cells of a footprint come from site_cells of
// cellgrid_host.h, the function the kernels call, not from a restatement.  Every index goes through std::vector::at.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "cellgrid_host.h"

struct Rec { int x, y, label, row; };
struct Grid {
  int x_min, y_min, x_max, y_max, side, ncx, ncy;
  std::vector<int> start;            // [ncx * ncy + 1]
  std::vector<Rec> recs;             // the records in cell order
};

// the points (label lab[i], or 0 without labels) into cells of side >= reach, at most max_cells of them
static Grid bin(const std::vector<int>& p, const std::vector<int>& lab, int reach, int max_cells) {
  Grid g;
  const int n = (int)p.size() / 2;
  g.x_min = g.x_max = p[0]; g.y_min = g.y_max = p[1];
  for (int i = 0; i < n; ++i) {
    g.x_min = std::min(g.x_min, p[2 * i]); g.x_max = std::max(g.x_max, p[2 * i]);
    g.y_min = std::min(g.y_min, p[2 * i + 1]); g.y_max = std::max(g.y_max, p[2 * i + 1]);
  }
  g.side = cell_grid_side(g.x_min, g.y_min, g.x_max, g.y_max, reach, max_cells);
  g.ncx = (int)cell_cells_along(g.x_min, g.x_max, g.side); g.ncy = (int)cell_cells_along(g.y_min, g.y_max, g.side);
  std::vector<int> count(g.ncx * g.ncy + 1, 0);
  for (int i = 0; i < n; ++i) count.at(cell_index(p[2 * i], p[2 * i + 1], g.x_min, g.y_min, g.side, g.ncx)) += 1;
  g.start.assign(g.ncx * g.ncy + 1, 0);
  for (int c = 0; c < g.ncx * g.ncy; ++c) g.start.at(c + 1) = g.start.at(c) + count.at(c);
  g.recs.assign(n, Rec{0, 0, 0, 0});
  std::vector<int> fill(g.start);
  for (int i = n - 1; i >= 0; --i)                                                         // backwards: the rows of a cell are NOT ascending
    g.recs.at(fill.at(cell_index(p[2 * i], p[2 * i + 1], g.x_min, g.y_min, g.side, g.ncx))++) = Rec{p[2 * i], p[2 * i + 1], lab.empty() ? 0 : lab.at(i), i};
  return g;
}

// take(record) on the records of the cells a footprint touches: the loop of both forms of site_sweep
template <class Take>
static void walk(const Grid& g, int x_lo, int x_hi, int y_lo, int y_hi, Take&& take) {
  const SiteCells c = site_cells(x_lo, x_hi, y_lo, y_hi, g.x_min, g.y_min, g.side, g.ncx, g.ncy);
  for (int gy = c.cy0; gy <= c.cy1; ++gy)
    for (int j = g.start.at(gy * g.ncx + c.cx0); j < g.start.at(gy * g.ncx + c.cx1 + 1); ++j) take(g.recs.at(j));
}

// the two footprints of site (u, v) at pitch s in the window (gx0, gy0, W, H), grown by the reach r: its own disc (direct) and its tile's
// (staged), as site_sweep forms them
struct Foot { int x_lo, x_hi, y_lo, y_hi; };
static Foot own_foot(int qx, int qy, int r) { return Foot{qx - r, qx + r, qy - r, qy + r}; }
static Foot tile_foot(int u, int v, int s, int gx0, int gy0, int W, int H, int r) {
  const int u0 = u / SITE_TILE * SITE_TILE, v0 = v / SITE_TILE * SITE_TILE, u1 = std::min(u0 + SITE_TILE, W) - 1, v1 = std::min(v0 + SITE_TILE, H) - 1;
  return Foot{(gx0 + u0) * s - r, (gx0 + u1) * s + r, (gy0 + v0) * s - r, (gy0 + v1) * s + r};
}

// one of the 80 random boxes at the corners of the coordinate range (P = CELL_COORD_LIMIT - 1): where it starts, and its window -- two
// tiles and a ragged edge each way, reaching past the box on all four sides (at most 37 x 21 sites: on a wide box the window hangs on the
// left and upper end in even rounds, on the right and lower end in odd ones)
static void box_origin(int rep, int extent, int* ox, int* oy) {
  constexpr int P = CELL_COORD_LIMIT - 1;
  *ox = rep % 4 == 0 ? -P : rep % 4 == 1 ? P - extent : rep % 4 == 2 ? -P : 1000;
  *oy = rep % 4 == 0 ? -P : rep % 4 == 1 ? P - extent : rep % 4 == 2 ? P - extent : -777;
}
static void box_window(const Grid& g, int rep, int r, int s, int* gx0, int* gy0, int* W, int* H) {
  *gx0 = cell_floor_div(g.x_min - r, s) - 3; *gy0 = cell_floor_div(g.y_min - r, s) - 3;
  const int gx1 = cell_floor_div(g.x_max + r, s) + 3, gy1 = cell_floor_div(g.y_max + r, s) + 3;
  *W = std::min(gx1 - *gx0 + 1, 37); *H = std::min(gy1 - *gy0 + 1, 21);
  if (rep & 1) { *gx0 = gx1 - *W + 1; *gy0 = gy1 - *H + 1; }
}

// the window limits, stated once for both caps -> the number of failed expectations
static int site_window_limits() {
  int bad = 0;
  auto expect = [&](bool ok, const char* what) { if (!ok) { std::printf("FAIL %s\n", what); ++bad; } };
  constexpr int Q = SITE_LIMIT - 1;
  for (const int64_t cap : {DENS_MAX_SITES, TERR_MAX_SITES}) {
    auto ok = [&](int s, int gx0, int gy0, int W, int H) { return site_window_ok(s, gx0, gy0, W, H, cap); };
    expect(ok(1, -Q, -Q, 1, 1) && ok(1 << 20, 255, -255, 1, 1) && !ok(1 << 20, 256, 0, 1, 1) && !ok(1 << 20, 0, -256, 1, 1) && !ok(1 << 20, 254, 0, 3, 1) && ok(1 << 20, 253, 0, 3, 1),
           "sites up to +-(2^28 - 1)");
    expect(!ok(4, 0, 0, 0, 1) && !ok(4, 0, 0, 1, 0) && !ok(0, 0, 0, 1, 1) && !ok((1 << 20) + 1, 0, 0, 1, 1) && !ok(1, INT32_MAX, 0, INT32_MAX, 1), "the window limits in 64 bits");
  }
  auto dens = [](int s, int gx0, int gy0, int W, int H) { return site_window_ok(s, gx0, gy0, W, H, DENS_MAX_SITES); };
  auto terr = [](int s, int gx0, int gy0, int W, int H) { return site_window_ok(s, gx0, gy0, W, H, TERR_MAX_SITES); };
  expect(dens(4, 0, 0, 1 << 12, 1 << 12) && !dens(4, 0, 0, (1 << 12) + 1, 1 << 12) && !dens(4, 0, 0, (1 << 24) + 1, 1), "the window limits in 64 bits: 2^24 sites");
  expect(terr(1, 0, 0, 1 << 14, 1 << 14) && !terr(1, 0, 0, (1 << 14) + 1, 1 << 14) && terr(1, -(1 << 27), 0, 1 << 28, 1) && !terr(1, -(1 << 27), 0, (1 << 28) + 1, 1),
         "the window limits in 64 bits: 2^28 sites");
  expect(terr(4, 0, 0, (1 << 24) + 1, 1) && !dens(4, 0, 0, (1 << 24) + 1, 1) && dens(4, 0, 0, 1 << 24, 1), "density's own cap is unchanged");
  return bad;
}
