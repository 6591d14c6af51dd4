// Host check of the plain-C++ parts of the nucleus territories (nuhtc_amd/csrc/cellgrid_host.h: the window check terr_window_ok, the key
// terr_key with its order and its two halves, the offer of a record terr_offer, the tally table index terr_table_at, the flush bound
// terr_table_fits and the route terr_route_staged), meant to be built with a sanitizer and run on the host -- it never touches a GPU, and
// the kernel code itself (cellterritory.hip) is NOT sanitized:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I nuhtc_amd/csrc tools/dev/cellterritory_host_check.cpp \
//       -o /tmp/cellterritory_host_check && /tmp/cellterritory_host_check
//
// Four parts.  The window limits in 64 bits, with this analysis' own cap of 2^28 sites.  The key: the unsigned order of the packed words
// against a compare of the pairs (d2, row) at the extremes of the bit budget and on random pairs, and the way back to d2 and row.  The
// table: every (a, b) of every C lands on a word of its own inside the (C + 1)^2 words in use, and the bound that lets a workgroup flush
// once.  The two sweeps of the owner kernels restated with the header's functions -- every site over the cells its own disc touches, and
// every site of a 16 x 16 tile over the tile's footprint -- on grids laid by cell_grid_side over boxes at the corners of the coordinate
// range, against a minimum over ALL points in 64 bits: the same owner and the same d2 at every site.  Every index into the start table
// and the records goes through std::vector::at.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "cellgrid_host.h"

struct Grid {
  int x_min, y_min, x_max, y_max, side, ncx, ncy;
  std::vector<int> start;            // [ncx * ncy + 1]
  std::vector<int> rx, ry, rl, rw;   // the records in cell order: x, y, label, row
};

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
  g.rx.assign(n, 0); g.ry.assign(n, 0); g.rl.assign(n, 0); g.rw.assign(n, 0);
  std::vector<int> fill(g.start);
  for (int i = n - 1; i >= 0; --i) {                                                       // backwards: the rows of a cell are NOT ascending
    const int at = fill.at(cell_index(p[2 * i], p[2 * i + 1], g.x_min, g.y_min, g.side, g.ncx))++;
    g.rx.at(at) = p[2 * i]; g.ry.at(at) = p[2 * i + 1]; g.rl.at(at) = lab[i]; g.rw.at(at) = i;
  }
  return g;
}

// the records of the cells that lo .. hi touch on each axis, against the site (qx, qy): the loop both kernels run
static unsigned long long sweep(const Grid& g, int x_lo, int x_hi, int y_lo, int y_hi, int qx, int qy, int C, int R) {
  unsigned long long best = TERR_NO_KEY;
  int cx0, cx1, cy0, cy1;
  site_cell_range(x_lo, x_hi, g.x_min, g.side, g.ncx, &cx0, &cx1);
  site_cell_range(y_lo, y_hi, g.y_min, g.side, g.ncy, &cy0, &cy1);
  if (cx0 > cx1) cy1 = cy0 - 1;
  for (int gy = cy0; gy <= cy1; ++gy) {
    const int j0 = g.start.at(gy * g.ncx + cx0), j1 = g.start.at(gy * g.ncx + cx1 + 1);
    for (int j = j0; j < j1; ++j) best = std::min(best, terr_offer(g.rx.at(j) - qx, g.ry.at(j) - qy, g.rl.at(j), g.rw.at(j), C, R, R * R));
  }
  return best;
}

int main() {
  int bad = 0;
  auto expect = [&](bool ok, const char* what) { if (!ok) { std::printf("FAIL %s\n", what); ++bad; } };
  constexpr int top = CELL_MAX_REACH * CELL_MAX_REACH, P = CELL_COORD_LIMIT - 1, Q = DENS_SITE_LIMIT - 1, last = (int)MST_MAX_POINTS - 1;
  static_assert(top == 1 << 28, "d2 is at most 2^28");
  // ---- the window
  expect(terr_window_ok(1, -Q, -Q, 1, 1) && terr_window_ok(1 << 20, 255, -255, 1, 1) && !terr_window_ok(1 << 20, 256, 0, 1, 1) && !terr_window_ok(1 << 20, 0, -256, 1, 1) &&
             !terr_window_ok(1 << 20, 254, 0, 3, 1) && terr_window_ok(1 << 20, 253, 0, 3, 1),
         "sites up to +-(2^28 - 1)");
  expect(terr_window_ok(1, 0, 0, 1 << 14, 1 << 14) && !terr_window_ok(1, 0, 0, (1 << 14) + 1, 1 << 14) && terr_window_ok(1, -(1 << 27), 0, 1 << 28, 1) &&
             !terr_window_ok(1, -(1 << 27), 0, (1 << 28) + 1, 1) && !terr_window_ok(4, 0, 0, 0, 1) && !terr_window_ok(4, 0, 0, 1, 0) && !terr_window_ok(0, 0, 0, 1, 1) &&
             !terr_window_ok((1 << 20) + 1, 0, 0, 1, 1) && !terr_window_ok(1, INT32_MAX, 0, INT32_MAX, 1),
         "the window limits in 64 bits: 2^28 sites");
  expect(terr_window_ok(4, 0, 0, (1 << 24) + 1, 1) && !dens_window_ok(4, 0, 0, (1 << 24) + 1, 1) && dens_window_ok(4, 0, 0, 1 << 24, 1), "density's own cap is unchanged");
  // ---- the key
  expect(terr_key(0, 0) == 0 && terr_key(top, last) < TERR_NO_KEY && terr_key_d2(terr_key(top, last)) == top && terr_key_row(terr_key(top, last)) == last &&
             terr_key_d2(TERR_NO_KEY) == -1 && terr_key_row(TERR_NO_KEY) == -1,
         "the extremes of the key");
  expect(terr_key(5, last) < terr_key(6, 0) && terr_key(5, 3) < terr_key(5, 4) && terr_key(top, 0) > terr_key(top - 1, last), "d2 first, then the row");
  std::mt19937 rng(7);
  for (int k = 0; k < 200000; ++k) {
    const int da = (int)(rng() % (unsigned)(top + 1)), db = k % 3 ? (int)(rng() % (unsigned)(top + 1)) : da, ra = (int)(rng() % (unsigned)(last + 1)), rb = (int)(rng() % (unsigned)(last + 1));
    if ((terr_key(da, ra) < terr_key(db, rb)) != (std::make_pair(da, ra) < std::make_pair(db, rb)) || terr_key_d2(terr_key(da, ra)) != da || terr_key_row(terr_key(da, ra)) != ra) {
      std::printf("FAIL key order (%d, %d) (%d, %d)\n", da, ra, db, rb);
      ++bad;
      break;
    }
  }
  expect(terr_offer(3, 4, 0, 9, 1, 5, 25) == terr_key(25, 9) && terr_offer(3, 5, 0, 9, 1, 5, 25) == TERR_NO_KEY && terr_offer(0, 0, 1, 9, 1, 5, 25) == TERR_NO_KEY &&
             terr_offer(0, 0, -1, 9, 14, 5, 25) == TERR_NO_KEY && terr_offer(0, 0, 13, 9, 14, 5, 25) == terr_key(0, 9),
         "the offer: inclusive reach, labels outside the classes");
  expect(terr_offer(Q + P, -(Q + P), 0, 1, 1, CELL_MAX_REACH, top) == TERR_NO_KEY && terr_offer(CELL_MAX_REACH, 0, 0, last, 1, CELL_MAX_REACH, top) == terr_key(top, last),
         "the box test comes before the products");
  // ---- the table and the flush bound
  for (int C = 1; C <= CELL_MAX_CLASSES; ++C) {
    std::set<int> seen;
    for (int a = 0; a <= C; ++a)
      for (int b = 0; b <= C; ++b) {
        const int at = terr_table_at(a, b, C);
        if (at < 0 || at >= (C + 1) * (C + 1) || at >= TERR_TABLE_WORDS || !seen.insert(at).second) { std::printf("FAIL table index C %d (%d, %d)\n", C, a, b); ++bad; }
        if (at / (C + 1) != a || at % (C + 1) != b) { std::printf("FAIL table index back C %d (%d, %d)\n", C, a, b); ++bad; }      // how the flush reads it
      }
  }
  expect(terr_table_fits(TERR_MAX_SITES) && terr_table_fits(((int64_t)1 << 30) - 1) && !terr_table_fits((int64_t)1 << 30) && TERR_PER_SITE == 4, "one flush per workgroup is enough");
  expect(terr_route_staged(1, 9, 9) && !terr_route_staged(4, 9, 9) && terr_route_staged(8, 128, 128) && !terr_route_staged(64, 128, 128), "the route");
  // ---- the two sweeps against a minimum over all points, boxes at the corners of the coordinate range
  for (int rep = 0; rep < 80; ++rep) {
    const int n = 1 + (int)(rng() % 150), extent = rep % 3 == 0 ? 6 : rep % 3 == 1 ? 60 : 400, R = 1 + (int)(rng() % 16), s = 1 + (int)(rng() % 24), C = 1 + rep % 3;
    const int ox = rep % 4 == 0 ? -P : rep % 4 == 1 ? P - extent : rep % 4 == 2 ? -P : 1000, oy = rep % 4 == 0 ? -P : rep % 4 == 1 ? P - extent : rep % 4 == 2 ? P - extent : -777;
    std::vector<int> p, lab;
    const int grain = rep % 2 ? 3 : 1;                                                     // a coarse grid: ties and coincident points
    for (int i = 0; i < n; ++i) {
      p.push_back(ox + (int)(rng() % (unsigned)(extent / grain + 1)) * grain); p.push_back(oy + (int)(rng() % (unsigned)(extent / grain + 1)) * grain);
      lab.push_back((int)(rng() % (unsigned)(C + 2)) - 1);                                 // -1 .. C: some do not compete
    }
    const Grid g = bin(p, lab, R, rep % 5 == 0 ? 6 : 1 << 22);
    int gx0 = cell_floor_div(g.x_min - R, s) - 3, gy0 = cell_floor_div(g.y_min - R, s) - 3;
    const int gx1 = cell_floor_div(g.x_max + R, s) + 3, gy1 = cell_floor_div(g.y_max + R, s) + 3;
    const int W = std::min(gx1 - gx0 + 1, 37), H = std::min(gy1 - gy0 + 1, 21);
    if (rep & 1) { gx0 = gx1 - W + 1; gy0 = gy1 - H + 1; }
    if (!terr_window_ok(s, gx0, gy0, W, H)) { std::printf("FAIL window of rep %d\n", rep); ++bad; continue; }
    for (int v = 0; v < H; ++v)
      for (int u = 0; u < W; ++u) {
        const int qx = (gx0 + u) * s, qy = (gy0 + v) * s;
        long long want_d2 = -1, want_row = -1;
        for (int i = 0; i < n; ++i) {
          const long long dx = (long long)p[2 * i] - qx, dy = (long long)p[2 * i + 1] - qy, d2 = dx * dx + dy * dy;
          if (lab[i] >= 0 && lab[i] < C && d2 <= (long long)R * R && (want_row < 0 || d2 < want_d2)) { want_d2 = d2; want_row = i; }      // ascending rows: the first minimum
        }
        const unsigned long long k1 = sweep(g, qx - R, qx + R, qy - R, qy + R, qx, qy, C, R);                                          // the site on its own
        const int u0 = u / DENS_TILE * DENS_TILE, v0 = v / DENS_TILE * DENS_TILE, u1 = std::min(u0 + DENS_TILE, W) - 1, v1 = std::min(v0 + DENS_TILE, H) - 1;
        const unsigned long long k2 = sweep(g, (gx0 + u0) * s - R, (gx0 + u1) * s + R, (gy0 + v0) * s - R, (gy0 + v1) * s + R, qx, qy, C, R);    // its tile's footprint
        if (terr_key_row(k1) != want_row || terr_key_d2(k1) != want_d2 || k2 != k1) {
          std::printf("FAIL rep %d site (%d, %d): row %lld d2 %lld, direct %d %d, tile %d %d\n", rep, u, v, want_row, want_d2, terr_key_row(k1), terr_key_d2(k1), terr_key_row(k2), terr_key_d2(k2));
          ++bad;
        }
      }
  }
  {
    // the largest reach at the corner of the range: 1500 coincident points, the smallest competing row wins at exactly R
    std::vector<int> p, lab;
    for (int i = 0; i < 1500; ++i) { p.push_back(P - CELL_MAX_REACH); p.push_back(-P + CELL_MAX_REACH); lab.push_back(i < 7 ? 5 : 0); }
    const Grid g = bin(p, lab, CELL_MAX_REACH, 1 << 22);
    unsigned long long k = sweep(g, P - 2 * CELL_MAX_REACH, P, -P, -P + 2 * CELL_MAX_REACH, P, -P + CELL_MAX_REACH, 1, CELL_MAX_REACH);      // a site at exactly R
    expect(terr_key_row(k) == 7 && terr_key_d2(k) == top, "1500 coincident points at reach 16384");
    k = sweep(g, P, P + 2 * CELL_MAX_REACH, -P, -P + 2 * CELL_MAX_REACH, P + CELL_MAX_REACH, -P + CELL_MAX_REACH, 1, CELL_MAX_REACH);       // a site past 2^27
    expect(k == TERR_NO_KEY, "a site two reaches right of them");
  }
  if (bad) std::printf("%d FAILED\n", bad); else std::printf("cellterritory host check ok\n");
  return bad ? 1 : 0;
}
