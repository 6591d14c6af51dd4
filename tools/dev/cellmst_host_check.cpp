// Host check of the plain-C++ parts of the minimum spanning forest (nuhtc_amd/csrc/cellgrid_host.h: the 53-bit pick key mst_key, its
// unpacking, the edge order mst_edge_less, the limits), meant to be built with a sanitizer and run on the host -- it never touches a GPU,
// and the kernel code itself (cellmst.hip) is NOT sanitized:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I nuhtc_amd/csrc tools/dev/cellmst_host_check.cpp \
//       -o /tmp/cellmst_host_check && /tmp/cellmst_host_check
//
// Three parts.  The round trip of (d2, lo) through the key at the extremes of both fields (d2 = 0 and 2^28, rows 0 and 2^24 - 1), inside
// 53 bits and below MST_NO_KEY.  The order: the unsigned order of the keys is the lexicographic order of (d2, lo), and mst_edge_less is
// the order of (d2, lo, hi).  And the rounds the kernels run, restated on small point sets with the header's functions -- every point
// keeps the smallest edge out of its component, a minimum over the (d2, lo) keys per component, then a minimum over hi among the points
// whose key equals it, the mutual picks emitted once -- against Kruskal's algorithm on the edges sorted by (d2, i, j): the same forest on
// every set, with ties, coincident points and both label modes.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <numeric>
#include <random>
#include <tuple>
#include <vector>

#include "cellgrid_host.h"

using Edge = std::tuple<int, int, int>;      // (d2, lo, hi)

static std::vector<Edge> all_edges(const std::vector<int>& p, const std::vector<int>& lab, int r, int by_class) {
  std::vector<Edge> e;
  const int n = (int)lab.size();
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j) {
      const int d2 = cell_pair_d2(p[2 * j] - p[2 * i], p[2 * j + 1] - p[2 * i + 1], r, r * r);
      if (d2 >= 0 && (!by_class || lab[i] == lab[j])) e.emplace_back(d2, i, j);
    }
  return e;
}

static int find(std::vector<int>& parent, int x) {
  while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
  return x;
}

static std::vector<Edge> kruskal(int n, std::vector<Edge> e) {
  std::sort(e.begin(), e.end());
  std::vector<int> parent(n);
  std::iota(parent.begin(), parent.end(), 0);
  std::vector<Edge> out;
  for (const Edge& x : e) {
    const int a = find(parent, std::get<1>(x)), b = find(parent, std::get<2>(x));
    if (a != b) { parent[std::max(a, b)] = std::min(a, b); out.push_back(x); }
  }
  std::sort(out.begin(), out.end(), [](const Edge& a, const Edge& b) { return std::make_pair(std::get<1>(a), std::get<2>(a)) < std::make_pair(std::get<1>(b), std::get<2>(b)); });
  return out;
}

// the rounds of cellmst.hip; *rounds = those that added an edge, -1 when round 25 still added one
static std::vector<Edge> boruvka(int n, const std::vector<Edge>& e, int* rounds) {
  std::vector<int> parent(n), comp(n), best2(n), lhi(n);
  std::vector<unsigned long long> best1(n), lkey(n);
  std::iota(parent.begin(), parent.end(), 0);
  std::vector<Edge> out;
  *rounds = 0;
  for (int round = 0; round < 25; ++round) {
    for (int i = 0; i < n; ++i) { comp[i] = find(parent, i); best1[i] = lkey[i] = MST_NO_KEY; best2[i] = lhi[i] = INT_MAX; }
    for (const Edge& x : e) {                                                // pick: every point's own smallest edge out
      const int d2 = std::get<0>(x), lo = std::get<1>(x), hi = std::get<2>(x);
      if (comp[lo] == comp[hi]) continue;
      const unsigned long long k = mst_key(d2, lo);
      for (int me : {lo, hi})
        if (mst_edge_less(k, hi, lkey[me], lhi[me])) { lkey[me] = k; lhi[me] = hi; }
    }
    for (int i = 0; i < n; ++i) best1[comp[i]] = std::min(best1[comp[i]], lkey[i]);
    for (int i = 0; i < n; ++i)
      if (lkey[i] != MST_NO_KEY && lkey[i] == best1[comp[i]]) best2[comp[i]] = std::min(best2[comp[i]], lhi[i]);
    size_t before = out.size();
    for (int c = 0; c < n; ++c) {                                            // emit and unite
      if (comp[c] != c || best1[c] == MST_NO_KEY) continue;
      const int lo = mst_key_lo(best1[c]), hi = best2[c], c2 = comp[comp[lo] == c ? hi : lo];
      if (!(c2 < c && best1[c2] == best1[c] && best2[c2] == hi)) out.emplace_back(mst_key_d2(best1[c]), lo, hi);
      const int a = find(parent, lo), b = find(parent, hi);
      if (a != b) parent[std::max(a, b)] = std::min(a, b);
    }
    if (out.size() == before) {
      std::sort(out.begin(), out.end(), [](const Edge& a, const Edge& b) { return std::make_pair(std::get<1>(a), std::get<2>(a)) < std::make_pair(std::get<1>(b), std::get<2>(b)); });
      return out;
    }
    ++*rounds;
  }
  *rounds = -1;
  return out;
}

int main() {
  int bad = 0;
  // ---- the bit budget and the round trip at the extremes
  static_assert(MST_MAX_D2 == 1 << 28 && MST_MAX_POINTS == 1 << 24 && MST_ROW_BITS == 24, "the budget of the key");
  const int d2s[] = {0, 1, 2, MST_MAX_D2 - 1, MST_MAX_D2}, rows[] = {0, 1, 2, (1 << 24) - 2, (1 << 24) - 1};
  std::vector<std::pair<int, int>> pts;
  for (int d2 : d2s) for (int lo : rows) pts.emplace_back(d2, lo);
  std::mt19937 rng(5);
  for (int k = 0; k < 2000; ++k) pts.emplace_back((int)(rng() % ((unsigned)MST_MAX_D2 + 1)), (int)(rng() % (1u << 24)));
  for (const auto& a : pts) {
    const unsigned long long k = mst_key(a.first, a.second);
    if (mst_key_d2(k) != a.first || mst_key_lo(k) != a.second || k >= (1ull << 53) || k == MST_NO_KEY) { std::printf("FAIL round trip d2 %d lo %d\n", a.first, a.second); ++bad; }
  }
  if (mst_key(MST_MAX_D2, (1 << 24) - 1) != (((unsigned long long)MST_MAX_D2 << 24) | 0xffffffull)) { std::printf("FAIL the largest key\n"); ++bad; }
  // ---- the order of the keys is the order of (d2, lo); mst_edge_less is the order of (d2, lo, hi)
  for (const auto& a : pts)
    for (size_t t = 0; t < pts.size(); t += 7) {
      const auto& b = pts[t];
      const unsigned long long ka = mst_key(a.first, a.second), kb = mst_key(b.first, b.second);
      if ((a < b) != (ka < kb) || (a == b) != (ka == kb)) { std::printf("FAIL order (%d, %d) (%d, %d)\n", a.first, a.second, b.first, b.second); ++bad; }
      for (int ha : {a.second + 1, (1 << 24) - 1}) for (int hb : {b.second + 1, (1 << 24) - 1})
        if (mst_edge_less(ka, ha, kb, hb) != (std::make_tuple(a.first, a.second, ha) < std::make_tuple(b.first, b.second, hb))) { std::printf("FAIL edge order\n"); ++bad; }
    }
  if (!mst_edge_less(mst_key(MST_MAX_D2, (1 << 24) - 2), (1 << 24) - 1, MST_NO_KEY, INT_MAX)) { std::printf("FAIL no key is not the largest\n"); ++bad; }
  // ---- the rounds against Kruskal
  for (int rep = 0; rep < 80; ++rep) {
    const int n = 1 + (int)(rng() % 260), extent = rep % 3 == 0 ? 6 : rep % 3 == 1 ? 30 : 200, r = 1 + (int)(rng() % 12), by_class = rep & 1;
    const int ox = rep % 4 == 0 ? -(CELL_COORD_LIMIT - 1) : rep % 4 == 1 ? CELL_COORD_LIMIT - 1 - extent : 1000;
    std::vector<int> p, lab;
    for (int i = 0; i < n; ++i) { p.push_back(ox + (int)(rng() % (unsigned)(extent + 1))); p.push_back(ox + (int)(rng() % (unsigned)(extent + 1))); lab.push_back((int)(rng() % 4) - 1); }
    const std::vector<Edge> e = all_edges(p, lab, r, by_class);
    int rounds = 0, cap = 0;
    while ((1 << cap) < n) ++cap;
    if (boruvka(n, e, &rounds) != kruskal(n, e) || rounds < 0 || rounds > cap) { std::printf("FAIL forest of %d points, r %d, by_class %d, %d rounds\n", n, r, by_class, rounds); ++bad; }
  }
  {
    std::vector<int> p, lab;                                          // the ruler of the tests: exactly log2 n rounds
    int x = 0;
    for (int k = 0; k < 256; ++k) { if (k) x += 2 + __builtin_ctz(k); p.push_back(x); p.push_back(0); lab.push_back(0); }
    int rounds = 0;
    const std::vector<Edge> e = all_edges(p, lab, 9, 0);
    if (boruvka(256, e, &rounds) != kruskal(256, e) || rounds != 8) { std::printf("FAIL ruler: %d rounds\n", rounds); ++bad; }
  }
  if (bad) std::printf("%d FAILED\n", bad); else std::printf("cellmst host check ok\n");
  return bad ? 1 : 0;
}
