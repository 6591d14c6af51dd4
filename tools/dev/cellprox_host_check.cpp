// Host check of the plain-C++ parts of the proximity graphs (nuhtc_amd/csrc/cellgrid_host.h: the two emptiness tests
// prox_gabriel_blocked and prox_rng_blocked over three squared distances, the -1 of cell_pair_d2 as "does not block", PROX_RNG_BIT), meant
// to be built with a sanitizer and run on the host -- it never touches a GPU, and the kernel code itself (cellprox.hip) is NOT sanitized:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I nuhtc_amd/csrc tools/dev/cellprox_host_check.cpp \
//       -o /tmp/cellprox_host_check && /tmp/cellprox_host_check
//
// Three parts.  The predicates at the extremes of the int32 budget (every d2 at 2^28, the sum at 2^29) and on the designed triples: a
// right angle at the witness and one step inside it, a witness at equal distance and one step nearer, a witness coincident with an end, a
// witness out of j's reach.  The graphs the kernels build, restated on small point sets with the header's functions the way the device
// runs them -- from the smaller row, witnesses skipped unless d2(i, k) < d2(i, j), djk through cell_pair_d2, the ends not told from the
// witnesses -- against the definition word for word in 64 bits with the ends excluded and no reach: the same edges and flags on every
// set, with ties, coincident points and both label modes.  The segment ordering of prox_place_kernel: every edge of a segment goes to
// the count of the edges there with a smaller larger-row, with the d2 | rng packing undone -- a sorted segment for any arrival order.  And
// cell_rank_in_segment itself, the function the four place kernels (cellprox, cellalpha, celladjacency, cellmst) call: the ranks of a
// shuffled segment of distinct values in the middle of a longer table are a permutation of j0 .. j1 - 1 in value order, whatever lies in
// front of the segment and behind it; an empty segment and a segment of one entry.
#include <algorithm>
#include <cstdio>
#include <random>
#include <tuple>
#include <vector>

#include "cellgrid_host.h"

using Edge = std::tuple<int, int, int, int>;      // (lo, hi, d2, rng)

// the device's way: cellprox.hip's prox_flags over every row instead of the 3 x 3 cells (a blocker is within reach of i either way)
static std::vector<Edge> device_way(const std::vector<int>& p, const std::vector<int>& lab, int r, int by_class) {
  std::vector<Edge> e;
  const int n = (int)lab.size(), r2 = r * r;
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j) {
      if (by_class && lab[i] != lab[j]) continue;
      const int dij = cell_pair_d2(p[2 * j] - p[2 * i], p[2 * j + 1] - p[2 * i + 1], r, r2);
      if (dij < 0) continue;
      bool gab = true, rng = true;
      for (int k = 0; k < n && gab; ++k) {
        if (by_class && lab[k] != lab[i]) continue;
        const int dik = cell_pair_d2(p[2 * k] - p[2 * i], p[2 * k + 1] - p[2 * i + 1], r, r2);
        if (dik < 0 || dik >= dij) continue;
        const int djk = cell_pair_d2(p[2 * k] - p[2 * j], p[2 * k + 1] - p[2 * j + 1], r, r2);
        if (prox_rng_blocked(dik, djk, dij)) { rng = false; gab = !prox_gabriel_blocked(dik, djk, dij); }
      }
      if (gab) e.emplace_back(i, j, dij, (int)rng);
    }
  return e;
}

// the definition: 64 bits, every other row a witness, no reach
static std::vector<Edge> definition(const std::vector<int>& p, const std::vector<int>& lab, int r, int by_class) {
  std::vector<Edge> e;
  const int n = (int)lab.size();
  auto d2 = [&](int a, int b) { const long long dx = (long long)p[2 * a] - p[2 * b], dy = (long long)p[2 * a + 1] - p[2 * b + 1]; return dx * dx + dy * dy; };
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j) {
      const long long dij = d2(i, j);
      if (dij > (long long)r * r || (by_class && lab[i] != lab[j])) continue;
      bool gab = true, rng = true;
      for (int k = 0; k < n; ++k) {
        if (k == i || k == j || (by_class && lab[k] != lab[i])) continue;
        const long long dik = d2(i, k), djk = d2(j, k);
        if (dik + djk < dij) gab = false;
        if (std::max(dik, djk) < dij) rng = false;
      }
      if (gab) e.emplace_back(i, j, (int)dij, (int)rng);
    }
  return e;
}

// prox_place_kernel on one segment: s_hi / s_d2 in arrival order -> (hi, d2, rng) in ascending hi
static bool place_ok(std::vector<int> s_hi, std::vector<int> s_d2) {
  const size_t m = s_hi.size();
  std::vector<int> hi(m, -1), d2(m, -1), rng(m, -1);
  for (size_t p = 0; p < m; ++p) {
    size_t at = 0;
    for (size_t j = 0; j < m; ++j) at += s_hi[j] < s_hi[p];
    hi.at(at) = s_hi[p]; d2.at(at) = s_d2[p] & (PROX_RNG_BIT - 1); rng.at(at) = (s_d2[p] & PROX_RNG_BIT) != 0;
  }
  for (size_t p = 0; p < m; ++p) {
    if (hi[p] < 0 || (p && hi[p - 1] >= hi[p])) return false;
    const size_t from = std::find(s_hi.begin(), s_hi.end(), hi[p]) - s_hi.begin();
    if (d2[p] != (s_d2[from] & ~PROX_RNG_BIT) || rng[p] != (s_d2[from] >> 30 & 1)) return false;
  }
  return true;
}

// cell_rank_in_segment over the segment j0 .. j0 + len - 1 of a table with other values around it: a permutation in value order
static bool rank_ok(size_t front, size_t len, size_t behind, std::mt19937& rng) {
  std::vector<int> table(front + len + behind);
  for (size_t k = 0; k < table.size(); ++k) table[k] = (int)(rng() % 1000);          // the neighbours: anything, smaller values among them
  std::vector<int> value(len);
  for (size_t k = 0; k < len; ++k) value[k] = (int)(7 * k + 2);
  std::shuffle(value.begin(), value.end(), rng);
  std::copy(value.begin(), value.end(), table.begin() + (long)front);
  const long long j0 = (long long)front, j1 = j0 + (long long)len;
  std::vector<int> placed(len, -1);
  for (size_t k = 0; k < len; ++k) {
    const long long at = cell_rank_in_segment(table.data(), j0, j1, value[k]);
    if (at < j0 || at >= j1 || placed.at((size_t)(at - j0)) != -1) return false;
    placed[(size_t)(at - j0)] = value[k];
  }
  return std::is_sorted(placed.begin(), placed.end());
}

int main() {
  int bad = 0;
  auto expect = [&](bool ok, const char* what) { if (!ok) { std::printf("FAIL %s\n", what); ++bad; } };
  // ---- the budget: every d2 within reach is at most 2^28, the sum at most 2^29, the rng bit above both
  constexpr int top = CELL_MAX_REACH * CELL_MAX_REACH;
  static_assert(top == 1 << 28 && PROX_RNG_BIT == 1 << 30 && top < PROX_RNG_BIT, "d2 and the rng bit share an int");
  expect(cell_pair_d2(CELL_MAX_REACH, 0, CELL_MAX_REACH, top) == top && cell_pair_d2(CELL_MAX_REACH, 1, CELL_MAX_REACH, top) == -1, "the reach is inclusive");
  expect(cell_pair_d2((1 << 28) - 1, -((1 << 28) - 1), CELL_MAX_REACH, top) == -1, "the box test comes before the products");
  expect(!prox_gabriel_blocked(top, top, top) && !prox_rng_blocked(top, top, top), "all three at 2^28");
  expect(prox_gabriel_blocked(top / 2 - 1, top / 2, top) && prox_rng_blocked(top - 1, top - 1, top) && !prox_gabriel_blocked(top - 1, top - 1, top), "just inside at 2^28");
  expect(((top | PROX_RNG_BIT) & (PROX_RNG_BIT - 1)) == top && ((top | PROX_RNG_BIT) & PROX_RNG_BIT), "the packing at 2^28");
  // ---- the designed triples: i = (0, 0), j = (10, 0), dij = 100
  expect(!prox_gabriel_blocked(50, 50, 100) && prox_rng_blocked(50, 50, 100), "a right angle at (5, 5): on the circle, inside the lune");
  expect(prox_gabriel_blocked(41, 41, 100), "(5, 4): one step inside the circle");
  expect(!prox_rng_blocked(100, 80, 100) && !prox_gabriel_blocked(100, 80, 100), "(6, 8): as far from i as j is");
  expect(prox_rng_blocked(85, 65, 100) && !prox_gabriel_blocked(85, 65, 100), "(6, 7): one step nearer");
  expect(!prox_rng_blocked(0, 100, 100) && !prox_gabriel_blocked(0, 100, 100) && !prox_rng_blocked(100, 0, 100) && !prox_gabriel_blocked(100, 0, 100), "a witness coincident with an end");
  expect(!prox_rng_blocked(4, -1, 81) && !prox_gabriel_blocked(4, -1, 81), "a witness out of j's reach");
  expect(!prox_rng_blocked(0, 0, 0) && !prox_gabriel_blocked(0, 0, 0), "coincident points: nothing is nearer than 0");
  for (int dij = 0; dij <= 40; ++dij)
    for (int dik = 0; dik <= 40; ++dik)
      for (int djk = -1; djk <= 40; ++djk)
        if (prox_gabriel_blocked(dik, djk, dij) && !prox_rng_blocked(dik, djk, dij)) { std::printf("FAIL Gabriel-blocked but not RNG-blocked %d %d %d\n", dik, djk, dij); ++bad; }
  // ---- the device's way against the definition
  std::mt19937 rng(9);
  for (int rep = 0; rep < 90; ++rep) {
    const int n = 1 + (int)(rng() % 120), extent = rep % 3 == 0 ? 5 : rep % 3 == 1 ? 24 : 150, r = 1 + (int)(rng() % 14), by_class = rep & 1;
    const int ox = rep % 4 == 0 ? -(CELL_COORD_LIMIT - 1) : rep % 4 == 1 ? CELL_COORD_LIMIT - 1 - extent : 1000;
    std::vector<int> p, lab;
    for (int i = 0; i < n; ++i) { p.push_back(ox + (int)(rng() % (unsigned)(extent + 1))); p.push_back(ox + (int)(rng() % (unsigned)(extent + 1))); lab.push_back((int)(rng() % 4) - 1); }
    if (device_way(p, lab, r, by_class) != definition(p, lab, r, by_class)) { std::printf("FAIL graphs of %d points, r %d, by_class %d\n", n, r, by_class); ++bad; }
  }
  {
    std::vector<int> p, lab;                                            // the largest reach at the edge of the coordinate range
    const int o = CELL_COORD_LIMIT - 1 - 2 * CELL_MAX_REACH;
    for (int y = 0; y < 3; ++y) for (int x = 0; x < 3; ++x) { p.push_back(o + x * CELL_MAX_REACH); p.push_back(-o - y * CELL_MAX_REACH); lab.push_back(0); }
    const std::vector<Edge> e = device_way(p, lab, CELL_MAX_REACH, 0);
    if (e != definition(p, lab, CELL_MAX_REACH, 0) || e.size() != 12) { std::printf("FAIL the 3 x 3 lattice at reach 16384: %zu edges\n", e.size()); ++bad; }
  }
  // ---- the segment ordering
  for (int rep = 0; rep < 200; ++rep) {
    const size_t m = rng() % 70;
    std::vector<int> hi(m), d2(m);
    for (size_t k = 0; k < m; ++k) { hi[k] = (int)(3 * k + 1); d2[k] = (int)(rng() % ((unsigned)top + 1)) | ((rng() & 1) ? PROX_RNG_BIT : 0); }
    std::vector<size_t> order(m);
    for (size_t k = 0; k < m; ++k) order[k] = k;
    std::shuffle(order.begin(), order.end(), rng);
    std::vector<int> s_hi(m), s_d2(m);
    for (size_t k = 0; k < m; ++k) { s_hi[k] = hi[order[k]]; s_d2[k] = d2[order[k]]; }
    if (!place_ok(s_hi, s_d2)) { std::printf("FAIL the order of a segment of %zu edges\n", m); ++bad; }
  }
  // ---- the shared rank: segments up to 300 long (past a wave's 64 and the 64 kept flags), empty and one-entry segments
  for (int rep = 0; rep < 200; ++rep) {
    const size_t len = rep < 3 ? (size_t)rep : rng() % 301;
    if (!rank_ok(rng() % 40, len, rng() % 40, rng)) { std::printf("FAIL the ranks of a segment of %zu entries\n", len); ++bad; }
  }
  {
    const std::vector<int> one = {5, 9, 1};
    expect(cell_rank_in_segment(one.data(), 1, 1, 100) == 1 && cell_rank_in_segment(one.data(), 3, 3, -5) == 3, "an empty segment: its own start");
    expect(cell_rank_in_segment(one.data(), 1, 2, 9) == 1 && cell_rank_in_segment(one.data(), 0, 1, 5) == 0, "a segment of one entry");
    expect(cell_rank_in_segment(one.data(), 0, 3, 9) == 2 && cell_rank_in_segment(one.data(), 0, 3, 1) == 0 && cell_rank_in_segment(one.data(), 0, 3, 5) == 1, "three entries");
  }
  if (bad) std::printf("%d FAILED\n", bad); else std::printf("cellprox host check ok\n");
  return bad ? 1 : 0;
}
