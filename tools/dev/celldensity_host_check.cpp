// Host check of the plain-C++ parts of the density rasters (nuhtc_amd/csrc/cellgrid_host.h: the floor cell of a site site_cell, the
// clamped cell range site_cell_range and the cells of a footprint site_cells, the weight term dens_term, the window check site_window_ok
// and the route site_route_staged), meant to be built with a sanitizer and run on the host -- it never touches a GPU, and the kernel code
// itself (celldensity.hip, cellsites.h) is NOT sanitized:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I nuhtc_amd/csrc tools/dev/celldensity_host_check.cpp \
//       -o /tmp/celldensity_host_check && /tmp/celldensity_host_check
//
// Three parts.  The functions at the extremes of the bit budget: a site at +-(2^28 - 1) against a box at -+(2^27 - 1), the floor left of
// the origin, the term at 0 and at 2^28, the window limits in 64 bits (cellsites_check.h, with both caps).  The two forms of the sweep
// (the walk of cellsites_check.h, on the cells site_cells gives) -- every site over the cells its own disc touches (dens_site_kernel), and
// every site of a 16 x 16 tile over the tile's footprint (dens_tile_kernel) -- on grids laid by cell_grid_side over boxes at the four
// corners of the coordinate range, with windows that reach past the box on all four sides, against a count over ALL points in 64 bits:
// the same counts and weights at every site.
#include "cellsites_check.h"

// what dens_take adds for the site (qx, qy)
struct Sum {
  int qx, qy, h;
  long long count = 0, weight = 0;
  void operator()(const Rec& o) {
    const int t = dens_term(o.x - qx, o.y - qy, h, h * h);
    if (t >= 0) { count += 1; weight += t; }
  }
};
static Sum sum_over(const Grid& g, const Foot& f, int qx, int qy, int h) {
  Sum m{qx, qy, h};
  walk(g, f.x_lo, f.x_hi, f.y_lo, f.y_hi, m);
  return m;
}

int main() {
  int bad = 0;
  auto expect = [&](bool ok, const char* what) { if (!ok) { std::printf("FAIL %s\n", what); ++bad; } };
  // ---- the extremes
  constexpr int top = CELL_MAX_REACH * CELL_MAX_REACH, P = CELL_COORD_LIMIT - 1, Q = SITE_LIMIT - 1;
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
    const SiteCells left = site_cells(-20, -11, 5, 15, 0, 0, 10, 4, 4), above = site_cells(5, 15, -20, -11, 0, 0, 10, 4, 4), in = site_cells(5, 15, 35, 45, 0, 0, 10, 4, 4);
    expect(left.cy0 > left.cy1 && above.cy0 > above.cy1 && in.cx0 == 0 && in.cx1 == 1 && in.cy0 == 3 && in.cy1 == 3, "beside the grid on either axis: no row");
  }
  bad += site_window_limits();
  expect(site_route_staged(1, 9, 9) && !site_route_staged(4, 9, 9) && site_route_staged(1 << 20, 16384, 1 << 29), "the route at the largest pitch and side");
  // ---- the two walks against a count over all points, boxes at the corners of the coordinate range
  std::mt19937 rng(11);
  for (int rep = 0; rep < 80; ++rep) {
    const int n = 1 + (int)(rng() % 150), extent = rep % 3 == 0 ? 6 : rep % 3 == 1 ? 60 : 400, h = 1 + (int)(rng() % 16), s = 1 + (int)(rng() % 24);
    int ox, oy, gx0, gy0, W, H;
    box_origin(rep, extent, &ox, &oy);
    std::vector<int> p;
    for (int i = 0; i < n; ++i) { p.push_back(ox + (int)(rng() % (unsigned)(extent + 1))); p.push_back(oy + (int)(rng() % (unsigned)(extent + 1))); }
    const Grid g = bin(p, {}, h, rep % 5 == 0 ? 6 : 1 << 22);                              // a few grids with cells wider than h
    box_window(g, rep, h, s, &gx0, &gy0, &W, &H);
    if (!site_window_ok(s, gx0, gy0, W, H, DENS_MAX_SITES)) { std::printf("FAIL window of rep %d\n", rep); ++bad; continue; }
    for (int v = 0; v < H; ++v)
      for (int u = 0; u < W; ++u) {
        const int qx = (gx0 + u) * s, qy = (gy0 + v) * s;
        long long want_c = 0, want_w = 0;
        for (int i = 0; i < n; ++i) {
          const long long dx = (long long)p[2 * i] - qx, dy = (long long)p[2 * i + 1] - qy, d2 = dx * dx + dy * dy;
          if (d2 <= (long long)h * h) { want_c += 1; want_w += (long long)h * h - d2; }
        }
        const Sum a = sum_over(g, own_foot(qx, qy, h), qx, qy, h), b = sum_over(g, tile_foot(u, v, s, gx0, gy0, W, H, h), qx, qy, h);
        if (a.count != want_c || a.weight != want_w || b.count != want_c || b.weight != want_w) {
          std::printf("FAIL rep %d site (%d, %d): %lld %lld, direct %lld %lld, tile %lld %lld\n", rep, u, v, want_c, want_w, a.count, a.weight, b.count, b.weight);
          ++bad;
        }
      }
  }
  {
    // the largest reach at the corner of the range: 1500 coincident points, the sum past 2^32
    std::vector<int> p;
    for (int i = 0; i < 1500; ++i) { p.push_back(P - CELL_MAX_REACH); p.push_back(-P + CELL_MAX_REACH); }
    const Grid g = bin(p, {}, CELL_MAX_REACH, 1 << 22);
    Sum m = sum_over(g, Foot{P - 2 * CELL_MAX_REACH, P, -P, -P + 2 * CELL_MAX_REACH}, P - CELL_MAX_REACH, -P + CELL_MAX_REACH, CELL_MAX_REACH);
    expect(m.count == 1500 && m.weight == 1500LL * top, "1500 coincident points at reach 16384");
    m = sum_over(g, Foot{P, P + 2 * CELL_MAX_REACH, -P, -P + 2 * CELL_MAX_REACH}, P + CELL_MAX_REACH, -P + CELL_MAX_REACH, CELL_MAX_REACH);       // a site past 2^27
    expect(m.count == 0 && m.weight == 0, "a site two reaches right of them");
  }
  if (bad) std::printf("%d FAILED\n", bad); else std::printf("celldensity host check ok\n");
  return bad ? 1 : 0;
}
