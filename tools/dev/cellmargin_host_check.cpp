// Host check of the plain-C++ parts of the margin bands (nuhtc_amd/csrc/cellgrid_host.h: the distance test margin_near with its parts
// margin_measure / margin_within / margin_mul_wide, the box reject margin_box_near, the record range edge_slab_range, and the limits
// margin_thresholds_ok / margin_call_ok), meant to be built with a sanitizer and run on the host -- it never touches a GPU, and the
// kernel code itself (cellmargin.hip) is NOT sanitized:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I nuhtc_amd/csrc tools/dev/cellmargin_host_check.cpp \
//       -o /tmp/cellmargin_host_check && /tmp/cellmargin_host_check
//
// Four parts.  margin_near against a restatement in __int128 throughout (no 64-bit intermediate): at the corners of the coordinate range
// -- the edge from (-2^27 + 1, -2^27 + 1) to (2^27 - 1, 2^27 - 1) with the point at the other corners among them -- at the smallest and
// the largest threshold, on small lattices where many pairs lie exactly at a threshold, and on Pythagorean edges (3-4-5, 119-120-169) with
// the point exactly at the threshold distance and one step beyond it, the float64-failing pair of the tests among them.  The box reject:
// near implies margin_box_near.  The record ranges against a direct loop over the slabs of grids laid by cell_grid_side: slab k is in the
// range exactly when the edge's y-range grown by R meets the slab's rows inside the box and the edge is not wholly left of x_min - R --
// and for every point of the box, every edge that crosses it or is near it has a record in the point's slab.  The limits at their last
// accepted and first refused values.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "cellgrid_host.h"

typedef __int128 wide;

static bool near_wide(int ax, int ay, int bx, int by, int px, int py, int e) {
  const wide dx = (wide)bx - ax, dy = (wide)by - ay, wx = (wide)px - ax, wy = (wide)py - ay, e2 = (wide)e * e;
  const wide L2 = dx * dx + dy * dy, s = wx * dx + wy * dy;
  if (L2 == 0 || s <= 0) return wx * wx + wy * wy <= e2;
  if (s >= L2) return ((wide)px - bx) * ((wide)px - bx) + ((wide)py - by) * ((wide)py - by) <= e2;
  const wide c = dx * wy - dy * wx;
  return (unsigned __int128)(c * c) <= (unsigned __int128)e2 * (unsigned __int128)L2;      // c^2 < 2^114: fits 127 bits
}

static bool crossed_wide(int ax, int ay, int bx, int by, int px, int py) {
  if ((ay <= py) == (by <= py)) return false;
  const bool up = ay < by;
  const wide lx = up ? ax : bx, ly = up ? ay : by, hx = up ? bx : ax, hy = up ? by : ay;
  return (hx - lx) * ((wide)py - ly) - (hy - ly) * ((wide)px - lx) > 0;
}

int main() {
  int bad = 0;
  auto expect = [&](bool ok, const char* what) { if (!ok) { std::printf("FAIL %s\n", what); ++bad; } };
  auto same = [&](int ax, int ay, int bx, int by, int px, int py, int e, const char* what) {
    const bool got = margin_near(ax, ay, bx, by, px, py, e), want = near_wide(ax, ay, bx, by, px, py, e);
    if (got != want) { if (bad < 10) std::printf("FAIL %s (%d %d %d %d) p (%d %d) e %d: %d, wide %d\n", what, ax, ay, bx, by, px, py, e, got, want); ++bad; }
    if (want) {
      const int x0 = std::min(ax, bx), x1 = std::max(ax, bx), y0 = std::min(ay, by), y1 = std::max(ay, by);
      if (!margin_box_near(x0, y0, x1, y1, px, py, e)) { if (bad < 10) std::printf("FAIL %s: near but rejected by the box\n", what); ++bad; }
    }
    return got;
  };
  constexpr int P = CELL_COORD_LIMIT - 1;
  // ---- the products: the two words against __int128
  {
    std::mt19937_64 rng(3);
    for (int rep = 0; rep < 100000; ++rep) {
      const uint64_t a = rng() >> (rep % 40), b = rng() >> (rep % 23);
      uint64_t hi, lo;
      margin_mul_wide(a, b, &hi, &lo);
      const unsigned __int128 p = (unsigned __int128)a * b;
      if (hi != (uint64_t)(p >> 64) || lo != (uint64_t)p) { ++bad; if (bad < 10) std::printf("FAIL mul_wide\n"); }
    }
  }
  // ---- the corners of the range: 7 values per coordinate, all 7^6 combinations, at the smallest and the largest threshold and one between
  {
    const int v[7] = {-P, -P + 1, -1, 0, 1, P - 1, P}, es[3] = {1, 5000, CELL_MAX_REACH};
    long long n = 0;
    for (int a = 0; a < 7; ++a) for (int b = 0; b < 7; ++b) for (int c = 0; c < 7; ++c) for (int d = 0; d < 7; ++d)
      for (int e = 0; e < 7; ++e) for (int f = 0; f < 7; ++f)
        for (int t : es) { same(v[a], v[b], v[c], v[d], v[e], v[f], t, "corner"); ++n; }
    expect(n == 3 * 117649, "all corner combinations");
    // the diagonal from corner to corner: the other corners are 2^27 sqrt 2 away, the ends and the points of the diagonal are on it
    expect(!same(-P, -P, P, P, -P, P, CELL_MAX_REACH, "diagonal") && !same(-P, -P, P, P, P, -P, CELL_MAX_REACH, "diagonal"), "the other corners are far");
    expect(same(-P, -P, P, P, -P, -P, 1, "diagonal") && same(-P, -P, P, P, P, P, 1, "diagonal") && same(-P, -P, P, P, 0, 0, 1, "diagonal"), "on the diagonal");
    // one step beside the diagonal: the distance is 1 / sqrt 2 <= 1; two steps: sqrt 2 > 1 and <= 2
    expect(same(-P, -P, P, P, 1, 0, 1, "diagonal") && !same(-P, -P, P, P, 2, 0, 1, "diagonal") && same(-P, -P, P, P, 2, 0, 2, "diagonal"), "beside the diagonal");
  }
  // ---- Pythagorean edges: the point exactly at the threshold distance is within, one step farther out is not
  {
    const int tri[2][3] = {{3, 4, 5}, {119, 120, 169}};
    std::mt19937 rng(11);
    for (int rep = 0; rep < 20000; ++rep) {
      const int* t = tri[rep & 1];
      const int len = 1 + (int)(rng() % 1000), k = 1 + (int)(rng() % (unsigned)(CELL_MAX_REACH / t[2]));     // e = k * t[2] <= 16384
      const int ox = (int)(rng() % 2000001) - 1000000, oy = (int)(rng() % 2000001) - 1000000, along = (int)(rng() % (unsigned)(len + 1));
      const int ax = ox, ay = oy, bx = ox + len * t[0], by = oy + len * t[1];
      // the foot along the edge, then k unit normals (-t[1], t[0]) of length t[2]: the distance is exactly k * t[2]
      const int px = ox + along * t[0] - k * t[1], py = oy + along * t[1] + k * t[0], e = k * t[2];
      const bool at = same(ax, ay, bx, by, px, py, e, "pythagorean"), past = same(ax, ay, bx, by, px - 1, py, e, "pythagorean");
      const bool below = e > 1 && same(ax, ay, bx, by, px, py, e - 1, "pythagorean");
      if (!at || (past && along > 0 && along < len) || below) { if (bad < 10) std::printf("FAIL pythagorean rep %d: %d %d %d\n", rep, at, past, below); ++bad; }
    }
    // the pair float64 decides wrongly: direction 119:120:169, the distance exactly 3549
    expect(same(-4576275, 3091603, 23000071, 30899683, 2840736, 10575982, 3549, "float64 pair"), "the float64-failing pair is within");
    expect(!same(-4576275, 3091603, 23000071, 30899683, 2840735, 10575982, 3549, "float64 pair") && !same(-4576275, 3091603, 23000071, 30899683, 2840736, 10575982, 3548, "float64 pair"),
           "and one step farther out, or one threshold lower, is not");
  }
  // ---- small lattices: the three regimes, s == 0 and s == L2 exactly, zero-length edges, points on edges
  {
    std::mt19937 rng(7);
    for (int rep = 0; rep < 200000; ++rep) {
      int q[6];
      for (int& t : q) t = (int)(rng() % 13) - 6;
      const int ox = rep % 3 == 0 ? P - 6 : rep % 3 == 1 ? -P + 6 : 0, oy = rep % 2 ? -P + 6 : P - 6;
      same(q[0] + ox, q[1] + oy, q[2] + ox, q[3] + oy, q[4] + ox, q[5] + oy, 1 + (int)(rng() % 8), "lattice");
    }
    expect(margin_near(0, 0, 0, 0, 3, 4, 5) && !margin_near(0, 0, 0, 0, 3, 4, 4), "a zero-length edge is its point");
    expect(margin_near(0, 0, 10, 0, 0, 5, 5) && margin_near(0, 0, 10, 0, 10, 5, 5) && !margin_near(0, 0, 10, 0, -3, 5, 5) && margin_near(0, 0, 10, 0, -3, 4, 5), "s == 0, s == L2, past an end");
    expect(margin_near(0, 0, 10, 10, 5, 5, 1) && margin_near(0, 0, 10, 10, 0, 0, 1), "on the edge and on a vertex");
  }
  // ---- the record ranges against a direct loop, and what a point sees from its slab against what it sees from all edges
  {
    std::mt19937 rng(5);
    for (int rep = 0; rep < 300; ++rep) {
      const int extent_x = 1 + (int)(rng() % 200), extent_y = 1 + (int)(rng() % 200), slab = 1 + (int)(rng() % 9), R = rep % 7 == 0 ? 0 : 1 + (int)(rng() % 40);
      const int ox = rep % 4 == 0 ? -P : rep % 4 == 1 ? P - extent_x : rep % 4 == 2 ? -P : 500, oy = rep % 4 == 0 ? -P : rep % 4 == 1 ? P - extent_y : rep % 4 == 2 ? P - extent_y : -300;
      const int x_min = ox, x_max = ox + extent_x, y_min = oy, y_max = oy + extent_y;
      const int side = cell_grid_side(x_min, y_min, x_max, y_max, slab, rep % 5 == 0 ? 7 : 1 << 22);
      const int ncy = (int)cell_cells_along(y_min, y_max, side);
      auto clampc = [&](long long v) { return (int)std::max<long long>(-P, std::min<long long>(P, v)); };
      std::vector<int> edges;
      const int E = 1 + (int)(rng() % 12);
      for (int e = 0; e < E; ++e)
        for (int k = 0; k < 4; ++k) edges.push_back(clampc((long long)(k % 2 ? oy : ox) - 100 + (long long)(rng() % (unsigned)((k % 2 ? extent_y : extent_x) + 200))));
      std::vector<std::vector<int>> of_slab(ncy);
      for (int e = 0; e < E; ++e) {
        const int ax = edges[4 * e], ay = edges[4 * e + 1], bx = edges[4 * e + 2], by = edges[4 * e + 3];
        int s0 = -1, s1 = -2;
        const bool kept = edge_slab_range(ax, ay, bx, by, R, x_min, y_min, y_max, side, &s0, &s1);
        const long long ylo = (long long)std::min(ay, by) - R, yhi = (long long)std::max(ay, by) + R;
        if (R == 0) {                                     // the census's range, written without R: the closed y-range clipped to the box
          const int lo = std::min(ay, by), hi = std::max(ay, by);
          const bool k0 = hi >= y_min && lo <= y_max && !(ax < x_min && bx < x_min);
          const int t0 = (std::max(lo, y_min) - y_min) / side, t1 = (std::min(hi, y_max) - y_min) / side;
          if (k0 != kept || (kept && (t0 != s0 || t1 != s1))) { std::printf("FAIL R == 0 is not the census's range, rep %d\n", rep); ++bad; }
        }
        for (int s = 0; s < ncy; ++s) {
          const long long r0 = (long long)y_min + (long long)s * side, r1 = std::min<long long>(r0 + side - 1, y_max);
          const bool meets = yhi >= r0 && ylo <= r1 && !((long long)ax < (long long)x_min - R && (long long)bx < (long long)x_min - R);
          const bool said = kept && s >= s0 && s <= s1;
          if (meets != said) { if (bad < 10) std::printf("FAIL record range rep %d edge %d slab %d: %d %d\n", rep, e, s, meets, said); ++bad; }
          if (said) of_slab.at(s).push_back(e);
        }
        if (kept && (s0 < 0 || s1 >= ncy || s0 > s1)) { std::printf("FAIL record range outside the grid, rep %d\n", rep); ++bad; }
      }
      for (int t = 0; t < 60; ++t) {
        const int px = x_min + (int)(rng() % (unsigned)(extent_x + 1)), py = y_min + (int)(rng() % (unsigned)(extent_y + 1));
        int all = 0, part = 0, all_near = 0, part_near = 0;
        for (int e = 0; e < E; ++e) {
          all ^= (int)crossed_wide(edges[4 * e], edges[4 * e + 1], edges[4 * e + 2], edges[4 * e + 3], px, py);
          all_near += R > 0 && near_wide(edges[4 * e], edges[4 * e + 1], edges[4 * e + 2], edges[4 * e + 3], px, py, R);
        }
        for (int e : of_slab.at((py - y_min) / side)) {
          part ^= (int)region_crossed(edges[4 * e], edges[4 * e + 1], edges[4 * e + 2], edges[4 * e + 3], px, py);
          part_near += R > 0 && margin_near(edges[4 * e], edges[4 * e + 1], edges[4 * e + 2], edges[4 * e + 3], px, py, R);
        }
        if (all != part || all_near != part_near) { if (bad < 10) std::printf("FAIL slab view rep %d point (%d, %d): %d %d / %d %d\n", rep, px, py, all, part, all_near, part_near); ++bad; }
      }
    }
  }
  // ---- the limits
  {
    const int32_t ok1[1] = {1}, top[2] = {1, CELL_MAX_REACH}, over[2] = {1, CELL_MAX_REACH + 1}, zero[2] = {0, 5}, flat[3] = {2, 5, 5}, down[3] = {2, 5, 4};
    int32_t full[MARGIN_MAX_BANDS + 1];
    for (int k = 0; k <= MARGIN_MAX_BANDS; ++k) full[k] = 10 * (k + 1);
    expect(margin_thresholds_ok(ok1, 1) && margin_thresholds_ok(top, 2) && margin_thresholds_ok(full, MARGIN_MAX_BANDS), "accepted rows");
    expect(!margin_thresholds_ok(full, MARGIN_MAX_BANDS + 1) && !margin_thresholds_ok(ok1, 0) && !margin_thresholds_ok(nullptr, 1) && !margin_thresholds_ok(over, 2) &&
               !margin_thresholds_ok(zero, 2) && !margin_thresholds_ok(flat, 3) && !margin_thresholds_ok(down, 3) && !margin_thresholds_ok(ok1, -1),
           "refused rows");
    expect(margin_call_ok(0, 0, 1, 0, ok1, 1) && margin_call_ok(REGION_MAX_EDGES, REGION_MAX_REGIONS, CELL_MAX_REACH, REGION_MAX_SLOTS, full, MARGIN_MAX_BANDS) &&
               !margin_call_ok(REGION_MAX_EDGES + 1, 1, 1, 0, ok1, 1) && !margin_call_ok(0, 0, 0, 0, ok1, 1) && !margin_call_ok(0, 0, 1, -1, ok1, 1) &&
               !margin_call_ok(0, 0, 1, 0, flat, 3) && !margin_call_ok(0, 0, 1, 0, ok1, 33),
           "the limits of a call");
  }
  if (bad) std::printf("%d FAILED\n", bad); else std::printf("cellmargin host check ok\n");
  return bad ? 1 : 0;
}
