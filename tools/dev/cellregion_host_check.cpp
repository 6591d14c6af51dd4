// Host check of the plain-C++ parts of the region census (nuhtc_amd/csrc/cellgrid_host.h: the crossing test region_crossed, the boundary
// test region_on_edge, the slab range of an edge edge_slab_range at R = 0, and the limits region_edge_ok / region_call_ok), meant to be built
// with a sanitizer and run on the host -- it never touches a GPU, and the kernel code itself (cellregion.hip) is NOT sanitized:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I nuhtc_amd/csrc tools/dev/cellregion_host_check.cpp \
//       -o /tmp/cellregion_host_check && /tmp/cellregion_host_check
//
// Three parts.  The two predicates against __int128 arithmetic: at the corners of the coordinate range (every vertex and the point
// drawn from +-(2^27 - 1) and their neighbours, where the products pass 2^55), on small lattices where many points lie on edges, and the
// hand-written rows of a rectangle (min sides in, max sides out).  The slab ranges against a direct loop over the slabs of grids laid by
// cell_grid_side, boxes at the corners of the range included: slab k is in the range exactly when the edge's closed y-range meets the
// slab's rows inside the box and the edge is not wholly left of it -- and the census a kernel would take from the slab's edges equals the
// one taken from all edges, for every point of the box row.  The limits at their last accepted and first refused values.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "cellgrid_host.h"

typedef __int128 wide;

static bool crossed_wide(int ax, int ay, int bx, int by, int px, int py) {
  if ((ay <= py) == (by <= py)) return false;
  const bool up = ay < by;
  const wide lx = up ? ax : bx, ly = up ? ay : by, hx = up ? bx : ax, hy = up ? by : ay;
  return (hx - lx) * ((wide)py - ly) - (hy - ly) * ((wide)px - lx) > 0;
}

static bool on_edge_wide(int ax, int ay, int bx, int by, int px, int py) {
  const wide c = ((wide)bx - ax) * ((wide)py - ay) - ((wide)by - ay) * ((wide)px - ax);
  return c == 0 && px >= std::min(ax, bx) && px <= std::max(ax, bx) && py >= std::min(ay, by) && py <= std::max(ay, by);
}

int main() {
  int bad = 0;
  auto expect = [&](bool ok, const char* what) { if (!ok) { std::printf("FAIL %s\n", what); ++bad; } };
  constexpr int P = CELL_COORD_LIMIT - 1;
  // ---- the predicates at the corners of the range: 9 values per coordinate, all 9^6 combinations would be 531441 -- taken in full
  {
    const int v[9] = {-P, -P + 1, -P + 2, -1, 0, 1, P - 2, P - 1, P};
    long long n = 0;
    for (int a = 0; a < 9; ++a) for (int b = 0; b < 9; ++b) for (int c = 0; c < 9; ++c) for (int d = 0; d < 9; ++d)
      for (int e = 0; e < 9; ++e) for (int f = 0; f < 9; ++f) {
        const bool c1 = region_crossed(v[a], v[b], v[c], v[d], v[e], v[f]), c2 = crossed_wide(v[a], v[b], v[c], v[d], v[e], v[f]);
        const bool o1 = region_on_edge(v[a], v[b], v[c], v[d], v[e], v[f]), o2 = on_edge_wide(v[a], v[b], v[c], v[d], v[e], v[f]);
        if (c1 != c2 || o1 != o2) { if (bad < 10) std::printf("FAIL corner (%d %d %d %d) p (%d %d): %d %d / %d %d\n", v[a], v[b], v[c], v[d], v[e], v[f], c1, c2, o1, o2); ++bad; }
        ++n;
      }
    expect(n == 531441, "all corner combinations");
  }
  // the thin triangle of the tests: one half-pixel step on either side of an edge from corner to corner
  expect(region_crossed(-P, -P, P, P - 1, -1, -1) == crossed_wide(-P, -P, P, P - 1, -1, -1) && region_crossed(-P, -P, P, P - 1, 1, 0) == crossed_wide(-P, -P, P, P - 1, 1, 0),
         "one step beside the long edge");
  // ---- small lattices: many points on edges
  std::mt19937 rng(7);
  for (int rep = 0; rep < 20000; ++rep) {
    int q[6];
    for (int& t : q) t = (int)(rng() % 9) - 4;
    const int ox = rep % 3 == 0 ? P - 4 : rep % 3 == 1 ? -P + 4 : 0, oy = rep % 2 ? -P + 4 : P - 4;
    const int ax = q[0] + ox, ay = q[1] + oy, bx = q[2] + ox, by = q[3] + oy, px = q[4] + ox, py = q[5] + oy;
    if (region_crossed(ax, ay, bx, by, px, py) != crossed_wide(ax, ay, bx, by, px, py) || region_on_edge(ax, ay, bx, by, px, py) != on_edge_wide(ax, ay, bx, by, px, py)) {
      if (bad < 10) std::printf("FAIL lattice rep %d\n", rep);
      ++bad;
    }
  }
  // ---- the rectangle (0, 0) .. (10, 6) by hand: the min-x and min-y sides belong to it, the max sides do not
  {
    const int r[4][4] = {{0, 0, 10, 0}, {10, 0, 10, 6}, {10, 6, 0, 6}, {0, 6, 0, 0}};
    auto inside = [&](int px, int py) { int par = 0; for (auto& e : r) par ^= (int)region_crossed(e[0], e[1], e[2], e[3], px, py); return par == 1; };
    auto on = [&](int px, int py) { bool t = false; for (auto& e : r) t |= region_on_edge(e[0], e[1], e[2], e[3], px, py); return t; };
    expect(inside(0, 0) && !inside(10, 0) && !inside(10, 6) && !inside(0, 6), "corners: only the min-min one is inside");
    expect(inside(5, 0) && inside(0, 3) && !inside(10, 3) && !inside(5, 6), "mid-sides: min sides in, max sides out");
    expect(inside(5, 3) && !inside(-1, 3) && !inside(11, 3) && !inside(5, -1) && !inside(5, 7), "inside and outside");
    expect(on(0, 0) && on(10, 0) && on(10, 6) && on(0, 6) && on(5, 0) && on(0, 3) && on(10, 3) && on(5, 6) && !on(5, 3) && !on(11, 0) && !on(-1, 6), "on the boundary");
    expect(region_on_edge(3, 3, 3, 3, 3, 3) && !region_on_edge(3, 3, 3, 3, 3, 4) && !region_crossed(3, 3, 3, 3, 0, 3), "a zero-length edge");
  }
  // ---- the slab ranges against a direct loop, and the census from a slab's edges against the census from all edges
  for (int rep = 0; rep < 300; ++rep) {
    const int extent_x = 1 + (int)(rng() % 200), extent_y = 1 + (int)(rng() % 200), slab = 1 + (int)(rng() % 9);
    const int ox = rep % 4 == 0 ? -P : rep % 4 == 1 ? P - extent_x : rep % 4 == 2 ? -P : 500, oy = rep % 4 == 0 ? -P : rep % 4 == 1 ? P - extent_y : rep % 4 == 2 ? P - extent_y : -300;
    const int x_min = ox, x_max = ox + extent_x, y_min = oy, y_max = oy + extent_y;
    const int side = cell_grid_side(x_min, y_min, x_max, y_max, slab, rep % 5 == 0 ? 7 : 1 << 22);
    const int ncy = (int)cell_cells_along(y_min, y_max, side);
    auto clampc = [&](long long v) { return (int)std::max<long long>(-P, std::min<long long>(P, v)); };
    std::vector<int> edges;
    const int E = 1 + (int)(rng() % 12);
    for (int e = 0; e < E; ++e)
      for (int k = 0; k < 4; ++k) edges.push_back(clampc((long long)(k % 2 ? oy : ox) - 60 + (long long)(rng() % (unsigned)((k % 2 ? extent_y : extent_x) + 120))));
    std::vector<std::vector<int>> of_slab(ncy);
    for (int e = 0; e < E; ++e) {
      const int ax = edges[4 * e], ay = edges[4 * e + 1], bx = edges[4 * e + 2], by = edges[4 * e + 3];
      int s0 = -1, s1 = -2;
      const bool kept = edge_slab_range(ax, ay, bx, by, 0, x_min, y_min, y_max, side, &s0, &s1);
      const int ylo = std::min(ay, by), yhi = std::max(ay, by);
      for (int s = 0; s < ncy; ++s) {
        const long long r0 = (long long)y_min + (long long)s * side, r1 = std::min<long long>(r0 + side - 1, y_max);
        const bool meets = yhi >= r0 && ylo <= r1 && !(ax < x_min && bx < x_min);
        const bool said = kept && s >= s0 && s <= s1;
        if (meets != said) { if (bad < 10) std::printf("FAIL slab range rep %d edge %d slab %d: %d %d\n", rep, e, s, meets, said); ++bad; }
        if (said) of_slab.at(s).push_back(e);
      }
      if (kept && (s0 < 0 || s1 >= ncy || s0 > s1)) { std::printf("FAIL slab range outside the grid, rep %d\n", rep); ++bad; }
    }
    for (int t = 0; t < 60; ++t) {
      const int px = x_min + (int)(rng() % (unsigned)(extent_x + 1)), py = y_min + (int)(rng() % (unsigned)(extent_y + 1));
      int all = 0, all_on = 0, part = 0, part_on = 0;
      for (int e = 0; e < E; ++e) {
        all ^= (int)crossed_wide(edges[4 * e], edges[4 * e + 1], edges[4 * e + 2], edges[4 * e + 3], px, py);
        all_on |= (int)on_edge_wide(edges[4 * e], edges[4 * e + 1], edges[4 * e + 2], edges[4 * e + 3], px, py);
      }
      for (int e : of_slab.at((py - y_min) / side)) {
        part ^= (int)region_crossed(edges[4 * e], edges[4 * e + 1], edges[4 * e + 2], edges[4 * e + 3], px, py);
        part_on |= (int)region_on_edge(edges[4 * e], edges[4 * e + 1], edges[4 * e + 2], edges[4 * e + 3], px, py);
      }
      if (all != part || all_on != part_on) { if (bad < 10) std::printf("FAIL census rep %d point (%d, %d)\n", rep, px, py); ++bad; }
    }
  }
  // ---- the limits
  expect(region_edge_ok(P, -P, -P, P, 0, 0, 1) && !region_edge_ok(P + 1, 0, 0, 0, 0, 0, 1) && !region_edge_ok(0, -P - 1, 0, 0, 0, 0, 1) && !region_edge_ok(0, 0, P + 1, 0, 0, 0, 1) &&
             !region_edge_ok(0, 0, 0, INT32_MIN, 0, 0, 1), "a vertex at and past the range");
  expect(region_edge_ok(0, 0, 1, 1, 3, 3, 4) && region_edge_ok(0, 0, 1, 1, 3, 2, 4) && !region_edge_ok(0, 0, 1, 1, 2, 3, 4) && !region_edge_ok(0, 0, 1, 1, 4, 3, 4) &&
             !region_edge_ok(0, 0, 1, 1, -1, 0, 4) && !region_edge_ok(0, 0, 1, 1, 0, 0, 0), "the region of an edge");
  expect(region_call_ok(0, 0, 1, 0) && region_call_ok(REGION_MAX_EDGES, REGION_MAX_REGIONS, CELL_MAX_REACH, REGION_MAX_SLOTS) && !region_call_ok(REGION_MAX_EDGES + 1, 1, 1, 0) &&
             !region_call_ok(0, REGION_MAX_REGIONS + 1, 1, 0) && !region_call_ok(0, 0, 0, 0) && !region_call_ok(0, 0, CELL_MAX_REACH + 1, 0) && !region_call_ok(0, 0, 1, -1) &&
             !region_call_ok(0, 0, 1, REGION_MAX_SLOTS + 1) && !region_call_ok(-1, 0, 1, 0) && !region_call_ok(0, -1, 1, 0),
         "the limits of a call");
  if (bad) std::printf("%d FAILED\n", bad); else std::printf("cellregion host check ok\n");
  return bad ? 1 : 0;
}
