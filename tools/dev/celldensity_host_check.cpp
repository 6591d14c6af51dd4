// Host check of the plain-C++ parts of the density rasters (nuhtc_amd/csrc/cellgrid_host.h: the floor cell of a site site_cell, the
// clamped cell range site_cell_range, the weight term dens_term, the window check dens_window_ok and the route dens_route_staged), meant
// to be built with a sanitizer and run on the host -- it never touches a GPU, and the kernel code itself (celldensity.hip) is NOT
// sanitized:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I nuhtc_amd/csrc tools/dev/celldensity_host_check.cpp \
//       -o /tmp/celldensity_host_check && /tmp/celldensity_host_check
//
// Three parts.  The functions at the extremes of the bit budget: a site at +-(2^28 - 1) against a box at -+(2^27 - 1), the floor left of
// the origin, the term at 0 and at 2^28, the window limits in 64 bits.  The two walks of the kernels restated with the header's functions
// -- every site over the cells its own disc touches (dens_site_kernel), and every site of a 16 x 16 tile over the tile's footprint
// (dens_tile_kernel) -- on grids laid by cell_grid_side over boxes at the four corners of the coordinate range, with windows that reach
// past the box on all four sides, against a count over ALL points in 64 bits: the same counts and weights at every site.  Every index into
// the start table and the records goes through std::vector::at.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "cellgrid_host.h"

struct Grid {
  int x_min, y_min, x_max, y_max, side, ncx, ncy;
  std::vector<int> start;            // [ncx * ncy + 1]
  std::vector<int> rx, ry;           // the records in cell order
};

static Grid bin(const std::vector<int>& p, int h, int max_cells) {
  Grid g;
  const int n = (int)p.size() / 2;
  g.x_min = g.x_max = p[0]; g.y_min = g.y_max = p[1];
  for (int i = 0; i < n; ++i) {
    g.x_min = std::min(g.x_min, p[2 * i]); g.x_max = std::max(g.x_max, p[2 * i]);
    g.y_min = std::min(g.y_min, p[2 * i + 1]); g.y_max = std::max(g.y_max, p[2 * i + 1]);
  }
  g.side = cell_grid_side(g.x_min, g.y_min, g.x_max, g.y_max, h, max_cells);
  g.ncx = (int)cell_cells_along(g.x_min, g.x_max, g.side); g.ncy = (int)cell_cells_along(g.y_min, g.y_max, g.side);
  std::vector<int> count(g.ncx * g.ncy + 1, 0);
  for (int i = 0; i < n; ++i) count.at(cell_index(p[2 * i], p[2 * i + 1], g.x_min, g.y_min, g.side, g.ncx)) += 1;
  g.start.assign(g.ncx * g.ncy + 1, 0);
  for (int c = 0; c < g.ncx * g.ncy; ++c) g.start.at(c + 1) = g.start.at(c) + count.at(c);
  g.rx.assign(n, 0); g.ry.assign(n, 0);
  std::vector<int> fill(g.start);
  for (int i = 0; i < n; ++i) {
    const int at = fill.at(cell_index(p[2 * i], p[2 * i + 1], g.x_min, g.y_min, g.side, g.ncx))++;
    g.rx.at(at) = p[2 * i]; g.ry.at(at) = p[2 * i + 1];
  }
  return g;
}

// the records of the cells that lo .. hi touch on each axis, against the site (qx, qy): the loop both kernels run
static void walk(const Grid& g, int x_lo, int x_hi, int y_lo, int y_hi, int qx, int qy, int h, long long* count, long long* weight) {
  int cx0, cx1, cy0, cy1;
  site_cell_range(x_lo, x_hi, g.x_min, g.side, g.ncx, &cx0, &cx1);
  site_cell_range(y_lo, y_hi, g.y_min, g.side, g.ncy, &cy0, &cy1);
  if (cx0 > cx1) cy1 = cy0 - 1;
  for (int gy = cy0; gy <= cy1; ++gy) {
    const int j0 = g.start.at(gy * g.ncx + cx0), j1 = g.start.at(gy * g.ncx + cx1 + 1);
    for (int j = j0; j < j1; ++j) {
      const int t = dens_term(g.rx.at(j) - qx, g.ry.at(j) - qy, h, h * h);
      if (t >= 0) { *count += 1; *weight += t; }
    }
  }
}

int main() {
  int bad = 0;
  auto expect = [&](bool ok, const char* what) { if (!ok) { std::printf("FAIL %s\n", what); ++bad; } };
  // ---- the extremes
  constexpr int top = CELL_MAX_REACH * CELL_MAX_REACH, P = CELL_COORD_LIMIT - 1, Q = DENS_SITE_LIMIT - 1;
  static_assert(top == 1 << 28, "a term is at most 2^28");
  expect(cell_floor_div(-1, 4) == -1 && cell_floor_div(-4, 4) == -1 && cell_floor_div(-5, 4) == -2 && cell_floor_div(0, 4) == 0 && cell_floor_div(7, 4) == 1, "the floor left of the origin");
  expect(site_cell(-Q, P, 1) == -Q - P && site_cell(Q, -P, 1) == Q + P && site_cell(-Q - CELL_MAX_REACH, P, CELL_MAX_REACH) < 0, "a site at the far end from the box");
  expect(dens_term(0, 0, CELL_MAX_REACH, top) == top && dens_term(CELL_MAX_REACH, 0, CELL_MAX_REACH, top) == 0 && dens_term(CELL_MAX_REACH, 1, CELL_MAX_REACH, top) == -1,
         "the term on the site, at exactly h and one step past it");
  expect(dens_term(Q + P, -(Q + P), CELL_MAX_REACH, top) == -1 && dens_term(-(Q + P), Q + P, 1, 1) == -1, "the box test comes before the products");
  expect(dens_term(3, 4, 5, 25) == 0 && dens_term(3, 5, 5, 25) == -1 && dens_term(0, 0, 1, 1) == 1 && dens_term(1, 0, 1, 1) == 0 && dens_term(1, 1, 1, 1) == -1, "3-4-5 and h = 1");
  {
    int c0, c1;
    site_cell_range(-Q - CELL_MAX_REACH, -Q + CELL_MAX_REACH, P - 10, CELL_MAX_REACH, 1, &c0, &c1);
    expect(c0 > c1, "left of a one-cell grid: empty");
    site_cell_range(Q - CELL_MAX_REACH, Q + CELL_MAX_REACH, -P, CELL_MAX_REACH, 3, &c0, &c1);
    expect(c0 > c1, "right of the grid: empty");
    site_cell_range(-5, 5, 0, 10, 4, &c0, &c1);
    expect(c0 == 0 && c1 == 0, "across the left edge");
    site_cell_range(35, 45, 0, 10, 4, &c0, &c1);
    expect(c0 == 3 && c1 == 3, "across the right edge: one cell past the last is clamped");
    site_cell_range(-20, -11, 0, 10, 4, &c0, &c1);
    expect(c0 == 0 && c1 == -2, "wholly left");
  }
  expect(dens_window_ok(1, -Q, -Q, 1, 1) && dens_window_ok(1 << 20, 255, -255, 1, 1) && !dens_window_ok(1 << 20, 256, 0, 1, 1) && !dens_window_ok(1 << 20, 0, -256, 1, 1) &&
             !dens_window_ok(1 << 20, 254, 0, 3, 1) && dens_window_ok(1 << 20, 253, 0, 3, 1),
         "sites up to +-(2^28 - 1)");
  expect(dens_window_ok(4, 0, 0, 1 << 12, 1 << 12) && !dens_window_ok(4, 0, 0, (1 << 12) + 1, 1 << 12) && !dens_window_ok(4, 0, 0, (1 << 24) + 1, 1) && !dens_window_ok(4, 0, 0, 0, 1) &&
             !dens_window_ok(4, 0, 0, 1, 0) && !dens_window_ok(0, 0, 0, 1, 1) && !dens_window_ok((1 << 20) + 1, 0, 0, 1, 1) && !dens_window_ok(1, INT32_MAX, 0, INT32_MAX, 1),
         "the window limits in 64 bits");
  expect(dens_route_staged(1, 9, 9) && !dens_route_staged(4, 9, 9) && dens_route_staged(1 << 20, 16384, 1 << 29), "the route at the largest pitch and side");
  // ---- the two walks against a count over all points, boxes at the corners of the coordinate range
  std::mt19937 rng(11);
  for (int rep = 0; rep < 80; ++rep) {
    const int n = 1 + (int)(rng() % 150), extent = rep % 3 == 0 ? 6 : rep % 3 == 1 ? 60 : 400, h = 1 + (int)(rng() % 16), s = 1 + (int)(rng() % 24);
    const int ox = rep % 4 == 0 ? -P : rep % 4 == 1 ? P - extent : rep % 4 == 2 ? -P : 1000, oy = rep % 4 == 0 ? -P : rep % 4 == 1 ? P - extent : rep % 4 == 2 ? P - extent : -777;
    std::vector<int> p;
    for (int i = 0; i < n; ++i) { p.push_back(ox + (int)(rng() % (unsigned)(extent + 1))); p.push_back(oy + (int)(rng() % (unsigned)(extent + 1))); }
    const Grid g = bin(p, h, rep % 5 == 0 ? 6 : 1 << 22);                                  // a few grids with cells wider than h
    // the window: two tiles and a ragged edge each way, reaching past the box on all four sides
    // (at most 37 x 21 sites: on a wide box the window hangs on the left and upper end in even rounds, on the right and lower end in odd ones)
    int gx0 = cell_floor_div(g.x_min - h, s) - 3, gy0 = cell_floor_div(g.y_min - h, s) - 3;
    const int gx1 = cell_floor_div(g.x_max + h, s) + 3, gy1 = cell_floor_div(g.y_max + h, s) + 3;
    const int W = std::min(gx1 - gx0 + 1, 37), H = std::min(gy1 - gy0 + 1, 21);
    if (rep & 1) { gx0 = gx1 - W + 1; gy0 = gy1 - H + 1; }
    if (!dens_window_ok(s, gx0, gy0, W, H)) { std::printf("FAIL window of rep %d\n", rep); ++bad; continue; }
    for (int v = 0; v < H; ++v)
      for (int u = 0; u < W; ++u) {
        const int qx = (gx0 + u) * s, qy = (gy0 + v) * s;
        long long want_c = 0, want_w = 0, c1 = 0, w1 = 0, c2 = 0, w2 = 0;
        for (int i = 0; i < n; ++i) {
          const long long dx = (long long)p[2 * i] - qx, dy = (long long)p[2 * i + 1] - qy, d2 = dx * dx + dy * dy;
          if (d2 <= (long long)h * h) { want_c += 1; want_w += (long long)h * h - d2; }
        }
        walk(g, qx - h, qx + h, qy - h, qy + h, qx, qy, h, &c1, &w1);                      // the site on its own
        const int u0 = u / DENS_TILE * DENS_TILE, v0 = v / DENS_TILE * DENS_TILE, u1 = std::min(u0 + DENS_TILE, W) - 1, v1 = std::min(v0 + DENS_TILE, H) - 1;
        walk(g, (gx0 + u0) * s - h, (gx0 + u1) * s + h, (gy0 + v0) * s - h, (gy0 + v1) * s + h, qx, qy, h, &c2, &w2);   // its tile's footprint
        if (c1 != want_c || w1 != want_w || c2 != want_c || w2 != want_w) {
          std::printf("FAIL rep %d site (%d, %d): %lld %lld, direct %lld %lld, tile %lld %lld\n", rep, u, v, want_c, want_w, c1, w1, c2, w2);
          ++bad;
        }
      }
  }
  {
    // the largest reach at the corner of the range: 1500 coincident points, the sum past 2^32
    std::vector<int> p;
    for (int i = 0; i < 1500; ++i) { p.push_back(P - CELL_MAX_REACH); p.push_back(-P + CELL_MAX_REACH); }
    const Grid g = bin(p, CELL_MAX_REACH, 1 << 22);
    long long c = 0, w = 0;
    walk(g, P - 2 * CELL_MAX_REACH, P, -P, -P + 2 * CELL_MAX_REACH, P - CELL_MAX_REACH, -P + CELL_MAX_REACH, CELL_MAX_REACH, &c, &w);
    expect(c == 1500 && w == 1500LL * top, "1500 coincident points at reach 16384");
    c = w = 0;
    walk(g, P, P + 2 * CELL_MAX_REACH, -P, -P + 2 * CELL_MAX_REACH, P + CELL_MAX_REACH, -P + CELL_MAX_REACH, CELL_MAX_REACH, &c, &w);      // a site past 2^27
    expect(c == 0 && w == 0, "a site two reaches right of them");
  }
  if (bad) std::printf("%d FAILED\n", bad); else std::printf("celldensity host check ok\n");
  return bad ? 1 : 0;
}
