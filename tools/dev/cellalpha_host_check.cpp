// Host check of the plain-C++ parts of the alpha complex (nuhtc_amd/csrc/cellgrid_host.h: alpha_frac_cmp, alpha_within_T, alpha_le_T,
// alpha_ge_neg_T, alpha_witness, alpha_dead, alpha_verdict, alpha_call_ok), meant to be built with a sanitizer and run on the host -- it
// never touches a GPU, and the kernel code itself (cellalpha.hip) is NOT sanitized:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I nuhtc_amd/csrc tools/dev/cellalpha_host_check.cpp \
//       -o /tmp/cellalpha_host_check && /tmp/cellalpha_host_check
//
// Three parts.  The compares at the extremes of the int64 budget (numerators and denominators at 2^20, d2 and D^2 - d2 at 2^20: products
// at 2^60, where UBSan would report a signed overflow).  The designed cases: the 6-8-10 triangle at r = 5 and r = 4 (a bound exactly at
// T), a witness on and one step inside the diametral circle, collinear witnesses between and outside the ends, a binding witness farther
// from i than j is, four cocircular points (both diagonals, lo == hi), the smallest row among tied apexes.  And the complex the kernels
// build, restated on small point sets with the header's functions the way the device runs them -- from the smaller row, every row offered
// to alpha_witness (which passes the far ones over before any product), the loop left once alpha_dead says so -- against the definition
// word for word in 128-bit fractions with NO witness passed over: the same edges, apexes and flags on every set, with ties, collinear,
// cocircular and coincident points, both label modes, the largest radius and the corners of the coordinate range.
#include <cstdio>
#include <random>
#include <tuple>
#include <vector>

#include "cellgrid_host.h"

using Edge = std::tuple<int, int, int, int, int, int>;      // (i, j, d2, apex0, apex1, gabriel)
typedef __int128 wide;

// the device's way: cellalpha.hip's alpha_test over every row instead of the window of cells
static std::vector<Edge> device_way(const std::vector<int>& p, const std::vector<int>& lab, int r, int by_class) {
  std::vector<Edge> e;
  const int n = (int)lab.size(), D = 2 * r, D2 = D * D;
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j) {
      if (by_class && lab[i] != lab[j]) continue;
      const int d2 = cell_pair_d2(p[2 * j] - p[2 * i], p[2 * j + 1] - p[2 * i + 1], D, D2);
      if (d2 < 0) continue;
      if (d2 == 0) { e.emplace_back(i, j, 0, -1, -1, 1); continue; }
      AlphaState st = alpha_open();
      bool dead = false;
      for (int k = 0; k < n && !dead; ++k) {
        if (by_class && lab[k] != lab[i]) continue;
        if (alpha_witness(st, p[2 * j] - p[2 * i], p[2 * j + 1] - p[2 * i + 1], p[2 * k] - p[2 * i], p[2 * k + 1] - p[2 * i + 1], k, D, D2))
          dead = alpha_dead(st, d2, D2);
      }
      int apex[2] = {-7, -7};
      const int f = dead ? 0 : alpha_verdict(st, d2, D2, apex);
      if (f & 1) e.emplace_back(i, j, d2, apex[0], apex[1], f >> 1);
    }
  return e;
}

// a / b against c / d for b, d > 0, and |a / b| <= T, in 128 bits
static int cmp_wide(wide a, wide b, wide c, wide d) { const wide l = a * d, r = c * b; return (l > r) - (l < r); }
static bool within_wide(wide a, wide b, wide d2, wide D2) { return a * a * d2 <= b * b * (D2 - d2); }

// the definition: every other row a witness, none passed over, the ends excluded by their row
static std::vector<Edge> definition(const std::vector<int>& p, const std::vector<int>& lab, int r, int by_class) {
  std::vector<Edge> e;
  const int n = (int)lab.size();
  const wide D2 = (wide)4 * r * r;
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j) {
      const wide qx = (wide)p[2 * j] - p[2 * i], qy = (wide)p[2 * j + 1] - p[2 * i + 1], d2 = qx * qx + qy * qy;
      if (d2 > D2 || (by_class && lab[i] != lab[j])) continue;
      if (d2 == 0) { e.emplace_back(i, j, 0, -1, -1, 1); continue; }
      wide hn = 0, hd = 0, ln = 0, ld = 0;
      int hk = -1, lk = -1;
      bool blocked = false, gab = true;
      for (int k = 0; k < n; ++k) {
        if (k == i || k == j || (by_class && lab[k] != lab[i])) continue;
        const wide rx = (wide)p[2 * k] - p[2 * i], ry = (wide)p[2 * k + 1] - p[2 * i + 1];
        const wide s = qx * ry - qy * rx, m = rx * (rx - qx) + ry * (ry - qy);
        if (m < 0) gab = false;
        if (s == 0) { blocked = blocked || m < 0; continue; }
        if (s > 0) { if (hd == 0 || cmp_wide(m, s, hn, hd) < 0) { hn = m; hd = s; hk = k; } }          // k ascends: the first row that attains it
        else if (ld == 0 || cmp_wide(-m, -s, ln, ld) > 0) { ln = -m; ld = -s; lk = k; }
      }
      const bool hi_ge = hd == 0 || hn >= 0 || within_wide(hn, hd, d2, D2), lo_le = ld == 0 || ln <= 0 || within_wide(ln, ld, d2, D2);
      if (blocked || !hi_ge || !lo_le || (hd != 0 && ld != 0 && cmp_wide(ln, ld, hn, hd) > 0)) continue;
      const int a0 = hd != 0 && (hn <= 0 || within_wide(hn, hd, d2, D2)) ? hk : -1, a1 = ld != 0 && (ln >= 0 || within_wide(ln, ld, d2, D2)) ? lk : -1;
      e.emplace_back(i, j, (int)d2, a0, a1, (int)gab);
    }
  return e;
}

static int bad = 0;
static void expect(bool ok, const char* what) { if (!ok) { std::printf("FAIL %s\n", what); ++bad; } }

static void designed(const char* what, std::vector<int> p, int r, const std::vector<Edge>& want) {
  const std::vector<int> lab(p.size() / 2, 0);
  const std::vector<Edge> got = device_way(p, lab, r, 0);
  if (got != want || definition(p, lab, r, 0) != want) {
    std::printf("FAIL %s: %zu edges\n", what, got.size());
    for (const Edge& g : got) std::printf("  (%d, %d) d2 %d apex %d %d gabriel %d\n", std::get<0>(g), std::get<1>(g), std::get<2>(g), std::get<3>(g), std::get<4>(g), std::get<5>(g));
    ++bad;
  }
}

int main() {
  // ---- the budget
  constexpr int64_t top = (int64_t)1 << 20;
  static_assert(4 * ALPHA_MAX_R * ALPHA_MAX_R == 1 << 20 && ALPHA_GABRIEL_BIT > (1 << 20), "D^2 <= 2^20, and an edge's d2 shares an int with the Gabriel bit");
  expect(alpha_frac_cmp(top, top, top, top) == 0 && alpha_frac_cmp(-top, 1, top, 1) < 0 && alpha_frac_cmp(top, 1, top - 1, 1) > 0, "fractions at 2^20");
  expect(alpha_frac_cmp(top, top - 1, top - 1, top - 2) < 0 && alpha_frac_cmp(-top, top - 1, -(top - 1), top - 2) > 0, "neighbouring fractions at 2^20");
  expect(alpha_within_T(top, top, (int)top / 2, (int)top) && !alpha_within_T(top, top - 1, (int)top / 2, (int)top), "num^2 d2 against den^2 (D^2 - d2) at 2^60");
  expect(alpha_within_T(-top, 1, 1, (int)top) == false && alpha_within_T(-1023, 1, 1, (int)top), "T^2 = 2^20 - 1: 1024 is beyond it, 1023 within");
  expect(alpha_le_T(-top, 1, 1, (int)top) && !alpha_le_T(top, 1, 1, (int)top) && alpha_ge_neg_T(top, 1, 1, (int)top) && !alpha_ge_neg_T(-top, 1, 1, (int)top), "the sign tests");
  expect(alpha_within_T(0, 1, (int)top, (int)top) && !alpha_within_T(1, top, (int)top, (int)top), "d2 == D^2: T = 0");
  expect(alpha_call_ok(5, 3, 512, 1, 0, 0, 0, 9, 9) && !alpha_call_ok(5, 3, 513, 0, 0, 0, 0, 9, 9) && !alpha_call_ok(5, 3, 0, 0, 0, 0, 0, 9, 9) &&
         !alpha_call_ok(5, 3, 5, 2, 0, 0, 0, 9, 9) && !alpha_call_ok(5, 3, 5, 0, -1, 0, 0, 9, 9) && !alpha_call_ok(5, 3, 5, 0, (int64_t)1 << 31, 0, 0, 9, 9) &&
         !alpha_call_ok(5, 15, 5, 0, 0, 0, 0, 9, 9) && !alpha_call_ok((int64_t)(1 << 24) + 1, 3, 5, 0, 0, 0, 0, 9, 9) && !alpha_call_ok(5, 3, 5, 0, 0, 0, 0, 1 << 27, 9) &&
         alpha_call_ok(0, 3, 5, 0, 0, 5, 5, 0, 0), "the front checks");
  // ---- the designed cases
  designed("6-8-10 at r = 5", {0, 0, 6, 0, 0, 8}, 5, {{0, 1, 36, 2, -1, 1}, {0, 2, 64, -1, 1, 1}, {1, 2, 100, 0, -1, 1}});
  designed("6-8-10 at r = 4", {0, 0, 6, 0, 0, 8}, 4, {{0, 1, 36, -1, -1, 1}, {0, 2, 64, -1, -1, 1}});
  designed("on the diametral circle", {0, 0, 10, 0, 5, 5}, 20, {{0, 1, 100, 2, -1, 1}, {0, 2, 50, -1, 1, 1}, {1, 2, 50, 0, -1, 1}});
  designed("one step inside it", {0, 0, 10, 0, 5, 4}, 20, {{0, 1, 100, 2, -1, 0}, {0, 2, 41, -1, 1, 1}, {1, 2, 41, 0, -1, 1}});
  designed("collinear", {0, 0, 5, 0, 10, 0, 17, 0}, 10, {{0, 1, 25, -1, -1, 1}, {1, 2, 25, -1, -1, 1}, {2, 3, 49, -1, -1, 1}});
  designed("a far witness", {0, 0, 4, 0, 10, 6}, 10, {{0, 1, 16, 2, -1, 1}, {0, 2, 136, -1, 1, 0}, {1, 2, 72, 0, -1, 1}});
  designed("a square: both diagonals", {0, 0, 10, 0, 10, 10, 0, 10}, 8,
           {{0, 1, 100, 2, -1, 1}, {0, 2, 200, 3, 1, 1}, {0, 3, 100, -1, 1, 1}, {1, 2, 100, 0, -1, 1}, {1, 3, 200, 0, 2, 1}, {2, 3, 100, 0, -1, 1}});
  designed("a square below its circumradius", {0, 0, 10, 0, 10, 10, 0, 10}, 7, {{0, 1, 100, -1, -1, 1}, {0, 3, 100, -1, -1, 1}, {1, 2, 100, -1, -1, 1}, {2, 3, 100, -1, -1, 1}});
  designed("two at D and two beyond", {0, 0, 6, 8, 100, 0, 110, 1}, 5, {{0, 1, 100, -1, -1, 1}});
  designed("coincident", {4, 4, 4, 4, 4, 4}, 1, {{0, 1, 0, -1, -1, 1}, {0, 2, 0, -1, -1, 1}, {1, 2, 0, -1, -1, 1}});
  // ---- the device's way against the definition
  std::mt19937 rng(9);
  for (int rep = 0; rep < 120; ++rep) {
    const int n = 1 + (int)(rng() % 90), extent = rep % 3 == 0 ? 5 : rep % 3 == 1 ? 24 : 150, r = 1 + (int)(rng() % (rep % 5 == 0 ? 60 : 9)), by_class = rep & 1;
    const int ox = rep % 4 == 0 ? -(CELL_COORD_LIMIT - 1) : rep % 4 == 1 ? CELL_COORD_LIMIT - 1 - extent : 1000;
    std::vector<int> p, lab;
    for (int i = 0; i < n; ++i) { p.push_back(ox + (int)(rng() % (unsigned)(extent + 1))); p.push_back(-ox - (int)(rng() % (unsigned)(extent + 1))); lab.push_back((int)(rng() % 4) - 1); }
    if (device_way(p, lab, r, by_class) != definition(p, lab, r, by_class)) { std::printf("FAIL the complex of %d points, r %d, by_class %d\n", n, r, by_class); ++bad; }
  }
  for (int rep = 0; rep < 6; ++rep) {                                   // the largest radius: points on a box D reaches across and well beyond it
    const int n = 70, extent = rep < 3 ? 700 : 4000;
    std::vector<int> p, lab;
    for (int i = 0; i < n; ++i) { p.push_back(CELL_COORD_LIMIT - 1 - (int)(rng() % (unsigned)extent)); p.push_back(-(CELL_COORD_LIMIT - 1) + (int)(rng() % (unsigned)extent)); lab.push_back(0); }
    const int ends[16] = {0, 0, 1, 0, 0, 1023, 1, -1023, 0, -1023, 1, 1023, 0, 1025, 1024, 0};      // the witnesses at the largest offsets that bind
    for (int k = 0; k < 16; ++k) p.push_back(ends[k] + (k & 1 ? -(CELL_COORD_LIMIT - 1) + 6000 : CELL_COORD_LIMIT - 1 - 6000));
    lab.insert(lab.end(), 8, 0);
    if (device_way(p, lab, ALPHA_MAX_R, 0) != definition(p, lab, ALPHA_MAX_R, 0)) { std::printf("FAIL the complex at r = 512, extent %d\n", extent); ++bad; }
  }
  if (bad) std::printf("%d FAILED\n", bad); else std::printf("cellalpha host check ok\n");
  return bad ? 1 : 0;
}
