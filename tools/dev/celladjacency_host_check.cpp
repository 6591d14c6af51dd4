// Host check of the plain-C++ parts of the territory adjacency (nuhtc_amd/csrc/cellgrid_host.h: the argument check adj_call_ok, the owner
// check adj_owner_ok, the edge test adj_is_edge, the key adj_key with its order and its two halves, the site of a thread site_uv, the pairs of a site adj_site_pairs,
// the slot hash adj_slot_hash / adj_slot_of and the slot count adj_table_slots), meant to be built with a sanitizer and run on the host --
// it never touches a GPU, and the kernel code itself (celladjacency.hip) is NOT sanitized:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I nuhtc_amd/csrc tools/dev/celladjacency_host_check.cpp \
//       -o /tmp/celladjacency_host_check && /tmp/celladjacency_host_check
//
// Five parts.  The argument limits in 64 bits.  The key: the unsigned order of the packed words against a compare of the pairs (i, j) at
// the extremes of the bit budget and on random pairs, the way back to its halves, and that no key is the empty mark.  The pairs of a
// site: over every site of small windows (one row, one column, no multiple of a tile) every 4-adjacent pair of the window comes up
// exactly once, and no pair leaves the window.  The slot count: a power of two, at least 2 M, at most 2^30 at the largest M.  The whole
// chain restated with the header's functions -- tile by tile, a table of ADJ_TILE_SLOTS slots per tile with linear probing, its records
// into one table of adj_table_slots(M) slots, the segments and the rank -- on random maps and on the designed ones, against a std::map
// over every site pair: the same edges in the same order, the same shared, the same degree; no probe runs past its table (every index
// goes through std::vector::at, and a probe that visits every slot is a failure).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "cellgrid_host.h"

struct Graph {
  std::vector<int> edges, shared, degree;      // [m][2], [m], [n]
  int64_t records = 0;
  bool bad = false;
};

// a table with linear probing: -> the slot of the key (inserted when absent, *fresh says so), or -1 when every slot was visited
static long long probe(std::vector<unsigned long long>& keys, unsigned long long key, bool* fresh) {
  const unsigned long long slots = keys.size();
  unsigned long long g = adj_slot_of(key, slots);
  for (unsigned long long t = 0; t < slots; ++t, g = (g + 1) & (slots - 1)) {
    if (keys.at(g) == ADJ_NO_KEY) { keys.at(g) = key; *fresh = true; return (long long)g; }
    if (keys.at(g) == key) { *fresh = false; return (long long)g; }
  }
  return -1;
}

// the stages of celladjacency.hip, one after the other
static Graph chain(const std::vector<int>& own, int W, int H, int n) {
  Graph out;
  out.degree.assign(n, 0);
  const int tiles_x = (W + SITE_TILE - 1) / SITE_TILE, tiles_y = (H + SITE_TILE - 1) / SITE_TILE;
  std::vector<std::vector<std::pair<unsigned long long, unsigned>>> records(tiles_x * tiles_y);
  for (int tile = 0; tile < tiles_x * tiles_y; ++tile) {                                  // count and insert: the tile pass
    std::vector<unsigned long long> keys(ADJ_TILE_SLOTS, ADJ_NO_KEY);
    std::vector<unsigned> cnt(ADJ_TILE_SLOTS, 0);
    for (int tid = 0; tid < SITE_TILE * SITE_TILE; ++tid) {
      int u, v;
      site_uv((unsigned)tile, tiles_x, tid, &u, &v);
      if (u >= W || v >= H) continue;
      const int at = v * W + u, pairs = adj_site_pairs(u, v, W, H), me = own.at(at);
      if (!adj_owner_ok(me, n)) out.bad = true;
      const int other[2] = {pairs & 1 ? own.at(at + 1) : me, pairs & 2 ? own.at(at + W) : me};
      for (int o : other) {
        if (!adj_is_edge(me, o, n)) continue;
        bool fresh = false;
        const long long s = probe(keys, adj_key(me, o), &fresh);
        if (s < 0) { std::printf("FAIL the tile table filled\n"); out.bad = true; return out; }
        cnt.at(s) += 1;
        out.records += fresh;
      }
    }
    for (int s = 0; s < ADJ_TILE_SLOTS; ++s)
      if (keys.at(s) != ADJ_NO_KEY) records.at(tile).push_back({keys.at(s), cnt.at(s)});
  }
  if (out.bad) return out;
  std::vector<unsigned long long> tkey((size_t)adj_table_slots(out.records), ADJ_NO_KEY);
  std::vector<unsigned> tcnt(tkey.size(), 0);
  std::vector<int> up(n, 0), start(n + 1, 0), fill(n, 0);
  for (const auto& tile : records)
    for (const auto& rec : tile) {
      bool fresh = false;
      const long long g = probe(tkey, rec.first, &fresh);
      if (g < 0) { std::printf("FAIL the call's table filled\n"); out.bad = true; return out; }
      if (fresh) { up.at(adj_key_lo(rec.first)) += 1; out.degree.at(adj_key_lo(rec.first)) += 1; out.degree.at(adj_key_hi(rec.first)) += 1; }
      tcnt.at(g) += rec.second;
    }
  for (int i = 0; i < n; ++i) start.at(i + 1) = start.at(i) + up.at(i);
  const int m = start.at(n);
  std::vector<int> s_hi(m, -1), s_cnt(m, 0);
  out.edges.assign(2 * (size_t)m, -1); out.shared.assign(m, 0);
  for (size_t g = 0; g < tkey.size(); ++g) {                                               // gather: slot order, i.e. hash order
    if (tkey.at(g) == ADJ_NO_KEY) continue;
    const int i = adj_key_lo(tkey.at(g)), p = start.at(i) + fill.at(i)++;
    out.edges.at(2 * p) = i; s_hi.at(p) = adj_key_hi(tkey.at(g)); s_cnt.at(p) = (int)tcnt.at(g);
  }
  for (int p = 0; p < m; ++p) {                                                           // place: the rank inside the segment
    const int lo = out.edges.at(2 * p), hi = s_hi.at(p);
    int at = start.at(lo);
    for (int j = start.at(lo); j < start.at(lo) + up.at(lo); ++j) at += s_hi.at(j) < hi;
    out.edges.at(2 * at + 1) = hi; out.shared.at(at) = s_cnt.at(p);
  }
  return out;
}

static Graph brute(const std::vector<int>& own, int W, int H, int n) {
  std::map<std::pair<int, int>, int> found;
  for (int v = 0; v < H; ++v)
    for (int u = 0; u < W; ++u) {
      const int a = own[v * W + u];
      if (u + 1 < W) { const int b = own[v * W + u + 1]; if (a != b && a >= 0 && b >= 0) found[{std::min(a, b), std::max(a, b)}] += 1; }
      if (v + 1 < H) { const int b = own[(v + 1) * W + u]; if (a != b && a >= 0 && b >= 0) found[{std::min(a, b), std::max(a, b)}] += 1; }
    }
  Graph out;
  out.degree.assign(n, 0);
  for (const auto& e : found) {                                                           // std::map: ascending (i, j)
    out.edges.push_back(e.first.first); out.edges.push_back(e.first.second); out.shared.push_back(e.second);
    out.degree.at(e.first.first) += 1; out.degree.at(e.first.second) += 1;
  }
  return out;
}

int main() {
  int bad = 0;
  auto expect = [&](bool ok, const char* what) { if (!ok) { std::printf("FAIL %s\n", what); ++bad; } };
  constexpr int last = (int)MST_MAX_POINTS - 1;
  // ---- the arguments
  expect(adj_call_ok(1, 1, 0, 0) && adj_call_ok(1 << 14, 1 << 14, MST_MAX_POINTS, INT32_MAX) && adj_call_ok(1 << 28, 1, 1, 0) && adj_call_ok(1, 1 << 28, 1, 0), "the limits themselves");
  expect(!adj_call_ok(0, 1, 1, 0) && !adj_call_ok(1, 0, 1, 0) && !adj_call_ok(-4, -4, 1, 0) && !adj_call_ok((1 << 14) + 1, 1 << 14, 1, 0) && !adj_call_ok(INT32_MAX, INT32_MAX, 1, 0) &&
             !adj_call_ok(4, 4, -1, 0) && !adj_call_ok(4, 4, MST_MAX_POINTS + 1, 0) && !adj_call_ok(4, 4, 1, -1) && !adj_call_ok(4, 4, 1, (int64_t)INT32_MAX + 1),
         "the limits in 64 bits");
  expect(adj_owner_ok(-1, 0) && !adj_owner_ok(0, 0) && adj_owner_ok(4, 5) && !adj_owner_ok(5, 5) && !adj_owner_ok(-2, 5) && !adj_owner_ok(INT32_MIN, 5) && !adj_owner_ok(INT32_MAX, last + 1),
         "an owner is -1 .. n - 1");
  expect(adj_is_edge(0, 1, 2) && adj_is_edge(1, 0, 2) && !adj_is_edge(1, 1, 2) && !adj_is_edge(-1, 1, 2) && !adj_is_edge(1, -1, 2) && !adj_is_edge(0, 2, 2) && !adj_is_edge(-2, 1, 2) &&
             !adj_is_edge(-1, -1, 2) && !adj_is_edge(0, 1, 0),
         "an edge: two different rows");
  // ---- the key
  expect(adj_key(0, 1) == 1ull && adj_key(1, 0) == 1ull && adj_key(last, last - 1) == adj_key(last - 1, last) && adj_key(last - 1, last) != ADJ_NO_KEY &&
             adj_key_lo(adj_key(last, 0)) == 0 && adj_key_hi(adj_key(last, 0)) == last && adj_key_lo(adj_key(last, last - 1)) == last - 1,
         "the extremes of the key");
  expect(adj_key(5, last) < adj_key(6, 7) && adj_key(5, 6) < adj_key(5, 7) && adj_key(0, last) < adj_key(1, 2), "the smaller row first, then the larger");
  std::mt19937 rng(11);
  for (int k = 0; k < 200000; ++k) {
    int a = (int)(rng() % (unsigned)(last + 1)), b = (int)(rng() % (unsigned)(last + 1)), c = k % 3 ? (int)(rng() % (unsigned)(last + 1)) : a, d = (int)(rng() % (unsigned)(last + 1));
    if (a == b || c == d) continue;
    const auto p = std::make_pair(std::min(a, b), std::max(a, b)), q = std::make_pair(std::min(c, d), std::max(c, d));
    if ((adj_key(a, b) < adj_key(c, d)) != (p < q) || adj_key_lo(adj_key(a, b)) != p.first || adj_key_hi(adj_key(a, b)) != p.second || adj_key(a, b) == ADJ_NO_KEY) {
      std::printf("FAIL key order (%d, %d) (%d, %d)\n", a, b, c, d);
      ++bad;
      break;
    }
  }
  // ---- the pairs of a site
  for (const auto& wh : {std::make_pair(1, 1), std::make_pair(1, 9), std::make_pair(9, 1), std::make_pair(17, 5), std::make_pair(16, 16), std::make_pair(33, 18)}) {
    const int W = wh.first, H = wh.second;
    std::set<std::pair<int, int>> seen;
    size_t count = 0;
    for (int v = 0; v < H; ++v)
      for (int u = 0; u < W; ++u) {
        const int pairs = adj_site_pairs(u, v, W, H), at = v * W + u;
        if (pairs & ~3) { std::printf("FAIL pairs of (%d, %d)\n", u, v); ++bad; }
        if (pairs & 1) { if (u + 1 >= W) { std::printf("FAIL a right pair leaves the window\n"); ++bad; } seen.insert({at, at + 1}); ++count; }
        if (pairs & 2) { if (v + 1 >= H) { std::printf("FAIL a lower pair leaves the window\n"); ++bad; } seen.insert({at, at + W}); ++count; }
      }
    if (count != (size_t)(2 * W * H - W - H) || seen.size() != count) { std::printf("FAIL %d x %d: %zu pairs, %zu distinct\n", W, H, count, seen.size()); ++bad; }
  }
  // ---- the slot count
  expect(adj_table_slots(0) == ADJ_MIN_SLOTS && adj_table_slots(512) == 1024 && adj_table_slots(513) == 2048 && adj_table_slots(ADJ_MAX_RECORDS) == (int64_t)1 << 30, "the slot count at its ends");
  for (int k = 0; k < 100000; ++k) {
    const int64_t M = k < 3000 ? k : (int64_t)(((uint64_t)rng() << 32 | rng()) % (uint64_t)(ADJ_MAX_RECORDS + 1)), slots = adj_table_slots(M);
    if (slots < 2 * M || slots < ADJ_MIN_SLOTS || (slots & (slots - 1)) || (slots > ADJ_MIN_SLOTS && slots / 2 >= 2 * M) || slots > (int64_t)1 << 30) {
      std::printf("FAIL slots of %lld: %lld\n", (long long)M, (long long)slots);
      ++bad;
      break;
    }
    const unsigned long long key = adj_key((int)(rng() % (unsigned)last), last);
    if (adj_slot_of(key, (unsigned long long)slots) >= (unsigned long long)slots) { std::printf("FAIL slot of a key\n"); ++bad; break; }
  }
  // ---- the chain against a map over every site pair
  auto compare = [&](const std::vector<int>& own, int W, int H, int n, const char* what) {
    const Graph got = chain(own, W, H, n), want = brute(own, W, H, n);
    if (got.bad || got.edges != want.edges || got.shared != want.shared || got.degree != want.degree || got.records < (int64_t)want.shared.size()) {
      std::printf("FAIL %s: %zu edges for %zu\n", what, got.shared.size(), want.shared.size());
      ++bad;
    }
  };
  for (int rep = 0; rep < 60; ++rep) {
    const int W = 1 + (int)(rng() % 70), H = rep % 7 == 0 ? 1 : 1 + (int)(rng() % 50), n = rep % 3 == 0 ? 2 + (int)(rng() % 6) : rep % 3 == 1 ? 40 : 5000;
    std::vector<int> own((size_t)W * H);
    int run = 0, cur = -1;
    for (auto& o : own) {                                                                  // runs of one owner, or an owner per site
      if (run == 0) { cur = (int)(rng() % (unsigned)(n + 1)) - 1; run = rep % 2 ? 1 : 1 + (int)(rng() % 5); }
      o = cur; --run;
    }
    compare(own, W, H, n, "a random map");
  }
  {
    std::vector<int> board(17 * 17), line(601, 0), back(601, 300);
    for (int k = 0; k < 17 * 17; ++k) board[k] = (k % 17 + k / 17) % 2;
    for (int k = 1; k <= 300; ++k) { line[2 * k - 1] = k; back[2 * k - 1] = 300 - k; }
    compare(board, 17, 17, 2, "the checkerboard");
    const Graph g = chain(board, 17, 17, 2);
    expect(g.shared.size() == 1 && g.shared[0] == 544 && g.records == 3, "one edge, shared 544, from three tiles (the corner tile's one site has no pair)");
    compare(line, 601, 1, 301, "a row with 300 neighbours");
    compare(line, 1, 601, 301, "the same, upright");
    compare(back, 601, 1, 301, "the same, renumbered");
    std::vector<int> full(64 * 64);
    for (auto& o : full) o = (int)(rng() % 2000u);
    compare(full, 64, 64, 2000, "a full tile table");
    full[77] = 2000;
    expect(chain(full, 64, 64, 2000).bad, "an owner n is seen");
    full[77] = -2;
    expect(chain(full, 64, 64, 2000).bad, "an owner -2 is seen");
  }
  if (bad) std::printf("%d FAILED\n", bad); else std::printf("celladjacency host check ok\n");
  return bad ? 1 : 0;
}
