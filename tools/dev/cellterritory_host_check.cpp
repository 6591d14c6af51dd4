// Host check of the plain-C++ parts of the nucleus territories (nuhtc_amd/csrc/cellgrid_host.h: the window check site_window_ok, the key
// terr_key with its order and its two halves, the offer of a record terr_offer, the tally table index terr_table_at, the flush bound
// terr_table_fits, the route site_route_staged and the cells of a footprint site_cells), meant to be built with a sanitizer and run on
// the host -- it never touches a GPU, and the kernel code itself (cellterritory.hip, cellsites.h) is NOT sanitized:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I nuhtc_amd/csrc tools/dev/cellterritory_host_check.cpp \
//       -o /tmp/cellterritory_host_check && /tmp/cellterritory_host_check
//
// Four parts.  The window limits in 64 bits (cellsites_check.h, with both caps: this analysis' own is 2^28 sites).  The key: the unsigned order of the packed words
// against a compare of the pairs (d2, row) at the extremes of the bit budget and on random pairs, and the way back to d2 and row.  The
// table: every (a, b) of every C lands on a word of its own inside the (C + 1)^2 words in use, and the bound that lets a workgroup flush
// once.  The two forms of the sweep (the walk of cellsites_check.h, on the cells site_cells gives) -- every site over the cells its own disc touches, and
// every site of a 16 x 16 tile over the tile's footprint -- on grids laid by cell_grid_side over boxes at the corners of the coordinate
// range, against a minimum over ALL points in 64 bits: the same owner and the same d2 at every site.
#include <set>
#include <utility>

#include "cellsites_check.h"

// the best key terr_take keeps for the site (qx, qy) over the records of a footprint
static unsigned long long sweep(const Grid& g, const Foot& f, int qx, int qy, int C, int R) {
  unsigned long long best = TERR_NO_KEY;
  walk(g, f.x_lo, f.x_hi, f.y_lo, f.y_hi, [&](const Rec& o) { best = std::min(best, terr_offer(o.x - qx, o.y - qy, o.label, o.row, C, R, R * R)); });
  return best;
}

int main() {
  int bad = 0;
  auto expect = [&](bool ok, const char* what) { if (!ok) { std::printf("FAIL %s\n", what); ++bad; } };
  constexpr int top = CELL_MAX_REACH * CELL_MAX_REACH, P = CELL_COORD_LIMIT - 1, Q = SITE_LIMIT - 1, last = (int)MST_MAX_POINTS - 1;
  static_assert(top == 1 << 28, "d2 is at most 2^28");
  // ---- the window
  bad += site_window_limits();
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
  expect(site_route_staged(1, 9, 9) && !site_route_staged(4, 9, 9) && site_route_staged(8, 128, 128) && !site_route_staged(64, 128, 128), "the route");
  // ---- the two sweeps against a minimum over all points, boxes at the corners of the coordinate range
  for (int rep = 0; rep < 80; ++rep) {
    const int n = 1 + (int)(rng() % 150), extent = rep % 3 == 0 ? 6 : rep % 3 == 1 ? 60 : 400, R = 1 + (int)(rng() % 16), s = 1 + (int)(rng() % 24), C = 1 + rep % 3;
    int ox, oy, gx0, gy0, W, H;
    box_origin(rep, extent, &ox, &oy);
    std::vector<int> p, lab;
    const int grain = rep % 2 ? 3 : 1;                                                     // a coarse grid: ties and coincident points
    for (int i = 0; i < n; ++i) {
      p.push_back(ox + (int)(rng() % (unsigned)(extent / grain + 1)) * grain); p.push_back(oy + (int)(rng() % (unsigned)(extent / grain + 1)) * grain);
      lab.push_back((int)(rng() % (unsigned)(C + 2)) - 1);                                 // -1 .. C: some do not compete
    }
    const Grid g = bin(p, lab, R, rep % 5 == 0 ? 6 : 1 << 22);
    box_window(g, rep, R, s, &gx0, &gy0, &W, &H);
    if (!site_window_ok(s, gx0, gy0, W, H, TERR_MAX_SITES)) { std::printf("FAIL window of rep %d\n", rep); ++bad; continue; }
    for (int v = 0; v < H; ++v)
      for (int u = 0; u < W; ++u) {
        const int qx = (gx0 + u) * s, qy = (gy0 + v) * s;
        long long want_d2 = -1, want_row = -1;
        for (int i = 0; i < n; ++i) {
          const long long dx = (long long)p[2 * i] - qx, dy = (long long)p[2 * i + 1] - qy, d2 = dx * dx + dy * dy;
          if (lab[i] >= 0 && lab[i] < C && d2 <= (long long)R * R && (want_row < 0 || d2 < want_d2)) { want_d2 = d2; want_row = i; }      // ascending rows: the first minimum
        }
        const unsigned long long k1 = sweep(g, own_foot(qx, qy, R), qx, qy, C, R), k2 = sweep(g, tile_foot(u, v, s, gx0, gy0, W, H, R), qx, qy, C, R);
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
    unsigned long long k = sweep(g, Foot{P - 2 * CELL_MAX_REACH, P, -P, -P + 2 * CELL_MAX_REACH}, P, -P + CELL_MAX_REACH, 1, CELL_MAX_REACH);      // a site at exactly R
    expect(terr_key_row(k) == 7 && terr_key_d2(k) == top, "1500 coincident points at reach 16384");
    k = sweep(g, Foot{P, P + 2 * CELL_MAX_REACH, -P, -P + 2 * CELL_MAX_REACH}, P + CELL_MAX_REACH, -P + CELL_MAX_REACH, 1, CELL_MAX_REACH);       // a site past 2^27
    expect(k == TERR_NO_KEY, "a site two reaches right of them");
  }
  if (bad) std::printf("%d FAILED\n", bad); else std::printf("cellterritory host check ok\n");
  return bad ? 1 : 0;
}
