// Host check of the plain-C++ parts of the cellular neighbourhoods (nuhtc_amd/csrc/cellhood_host.h: the generator of the seeding draws,
// the pick rule on a prefix sum, both squared distances, the rounding of a centre, the packing of a window and the limits), meant to be
// built with a sanitizer and run on the host -- it never touches a GPU, and the kernel code itself (cellhood.hip) is NOT sanitized:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I nuhtc_amd/csrc tools/dev/cellhood_host_check.cpp \
//       -o /tmp/cellhood_host_check && /tmp/cellhood_host_check
//
// Six parts.  The generator: values written out by hand from the definition, distinct over j and over seeds, wrapping mod 2^32.  The
// packing: every class at every count round-trips and leaves the other bytes alone; a label outside the classes is counted nowhere.  The
// pick: against a direct search on random prefix arrays with zeros, at every t, both sides of every boundary.  The distances: against
// plain loops at the extremes (33 in one class against 34000 everywhere: past 2^33).  The rounding: exactly one half goes up (1025 over
// 2048 gives 513), against __int128 arithmetic at the largest sums, an empty type keeps its centre.  The limits at their last accepted
// and first refused values.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "cellhood_host.h"

int main() {
  int bad = 0;
  auto expect = [&](bool ok, const char* what) { if (!ok) { std::printf("FAIL %s\n", what); ++bad; } };

  // ---- the generator
  {
    const uint32_t b = ce_fmix(0x9E3779B9u);
    expect(hood_draw(0u, 0) == (((unsigned long long)ce_fmix(b + 0x7F4A7C15u) << 32) | ce_fmix(b + 2u * 0x7F4A7C15u)), "u_0 of seed 0");
    expect(hood_draw(0u, 0) == 17234813504040894259ull && hood_draw(0u, 1) == 6590020050189462346ull, "u_0, u_1 of seed 0 (neighbourhoods.draws)");
    const uint32_t w = ce_fmix(0xFFFFFFFFu + 0x9E3779B9u * 32u);         // wraps
    expect(hood_draw(0xFFFFFFFFu, 31) == (((unsigned long long)ce_fmix(w + 0x7F4A7C15u) << 32) | ce_fmix(w + 2u * 0x7F4A7C15u)), "u_31 of the last seed");
    std::vector<unsigned long long> seen;
    for (uint32_t seed : {0u, 1u, 2024u, 0xFFFFFFFFu})
      for (int j = 0; j < HOOD_MAX_TYPES; ++j) seen.push_back(hood_draw(seed, j));
    bool distinct = true;
    for (size_t i = 0; i < seen.size(); ++i)
      for (size_t k = i + 1; k < seen.size(); ++k) distinct &= seen[i] != seen[k];
    expect(distinct, "the draws differ over j and over seeds");
  }

  // ---- the packing
  for (int C = 1; C <= CELL_MAX_CLASSES; ++C)
    for (int c = 0; c < C; ++c) {
      HoodWin w{0, 0};
      for (int o = 0; o < C; ++o)
        if (o != c) hood_win_add(w, o, C);                               // one in every other class
      bool ok = true;
      for (int count = 1; count <= 33; ++count) {
        hood_win_add(w, c, C);
        ok &= hood_win_at(w, c) == count;
        for (int o = 0; o < CELL_MAX_CLASSES + 2; ++o)
          if (o != c) ok &= hood_win_at(w, o) == (o < C ? 1 : 0);
      }
      const HoodWin before = w;
      hood_win_add(w, -1, C); hood_win_add(w, C, C); hood_win_add(w, 14, C); hood_win_add(w, 1 << 30, C); hood_win_add(w, INT32_MIN, C);
      ok &= w.lo == before.lo && w.hi == before.hi;
      expect(ok, "pack / unpack");
    }
  expect(sizeof(HoodWin) == 16 && alignof(HoodWin) == 16, "a window is one 128-bit word");

  // ---- the pick
  {
    std::mt19937 rng(5);
    for (int round = 0; round < 200; ++round) {
      const int n = 1 + (int)(rng() % 40);
      std::vector<int64_t> g(n), incl(n);
      int64_t run = 0;
      for (int i = 0; i < n; ++i) { g[i] = (rng() % 3 == 0) ? 0 : (int64_t)(rng() % 2179); run += g[i]; incl[i] = run; }
      bool ok = true;
      int64_t at = 0;
      for (int i = 0; i < n && ok; ++i) {                                // both sides of every boundary, and every t of a short set
        for (int64_t t : {at, at + g[i] - 1, at + g[i]}) {
          if (t < 0 || t >= run) continue;
          int64_t want = 0;
          while (incl[want] <= t) ++want;                                // the smallest i with incl[i] > t
          ok &= hood_pick_row(incl.data(), n, t) == want && g[want] > 0;
          int hits = 0;
          for (int k = 0; k < n; ++k) hits += hood_picks(k ? incl[k - 1] : 0, g[k], t);
          ok &= hits == 1;                                               // exactly one element claims t
        }
        at += g[i];
      }
      ok &= hood_pick_row(incl.data(), n, run) == n;                    // no such row
      expect(ok, "pick");
    }
    const int64_t big[3] = {((int64_t)1 << 36) - 5, ((int64_t)1 << 36) - 5, (int64_t)1 << 36};
    expect(hood_pick_row(big, 3, ((int64_t)1 << 36) - 6) == 0 && hood_pick_row(big, 3, ((int64_t)1 << 36) - 5) == 2, "pick near 2^36");
  }

  // ---- the distances
  {
    std::mt19937 rng(9);
    bool ok = true;
    for (int round = 0; round < 2000; ++round) {
      const int C = 1 + (int)(rng() % CELL_MAX_CLASSES);
      HoodWin a{0, 0}, b{0, 0};
      int wa[CELL_MAX_CLASSES] = {0}, wb[CELL_MAX_CLASSES] = {0}, q[HOOD_LANES] = {0};
      for (int k = 0; k < 33; ++k) { const int c = (int)(rng() % C); hood_win_add(a, c, C); ++wa[c]; }
      for (int k = 0; k < (int)(rng() % 34); ++k) { const int c = (int)(rng() % C); hood_win_add(b, c, C); ++wb[c]; }
      for (int c = 0; c < C; ++c) q[c] = (int)(rng() % (HOOD_MAX_CENTRE + 1));
      long long d2 = 0, D = 0;
      for (int c = 0; c < C; ++c) {
        d2 += (long long)(wa[c] - wb[c]) * (wa[c] - wb[c]);
        D += (long long)(HOOD_ONE * wa[c] - q[c]) * (HOOD_ONE * wa[c] - q[c]);
      }
      ok &= hood_win_d2(a, b) == d2 && d2 <= 2 * 33 * 33 && (long long)hood_distance(a, q) == D;
    }
    expect(ok, "distances against plain loops");
    HoodWin far{0, 0}, other{0, 0};
    int q[HOOD_LANES] = {0};
    for (int k = 0; k < 33; ++k) { hood_win_add(far, 0, 14); hood_win_add(other, 13, 14); }
    for (int c = 1; c < CELL_MAX_CLASSES; ++c) q[c] = HOOD_MAX_CENTRE;
    expect(hood_win_d2(far, other) == 2178, "the largest seeding distance");
    expect(hood_distance(far, q) == 33792ull * 33792ull + 13ull * 34000ull * 34000ull && hood_distance(far, q) > (1ull << 33), "the largest D: past 2^33");
    q[0] = HOOD_MAX_CENTRE;
    HoodWin none{0, 0};
    expect(hood_distance(none, q) == 14ull * 34000ull * 34000ull, "the zero window against the largest centres");
  }

  // ---- the rounding
  {
    expect(hood_round(1025, 2048, 0) == 513 && hood_round(1023, 2048, 0) == 512 && hood_round(1024, 2048, 0) == 512, "one half goes up");
    expect(hood_round(1, 2, 0) == 512 && hood_round(1, 3, 0) == 341 && hood_round(2, 3, 0) == 683 && hood_round(0, 7, 9) == 0, "thirds and zero");
    expect(hood_round(0, 0, 777) == 777 && hood_round(5, 0, 12) == 12, "an empty type keeps its centre");
    std::mt19937_64 rng(3);
    bool ok = true;
    for (int round = 0; round < 20000; ++round) {
      const long long m = 1 + (long long)(rng() % (uint64_t)HOOD_MAX_POINTS), s = (long long)(rng() % (uint64_t)(33 * m + 1));
      const __int128 want = ((__int128)2048 * s + m) / (2 * (__int128)m);
      ok &= hood_round(s, m, -1) == (int)want && want >= 0 && want <= 33792;
    }
    expect(ok, "rounding against 128-bit arithmetic");
    expect(hood_round(33LL * HOOD_MAX_POINTS, HOOD_MAX_POINTS, 0) == 33792, "the largest sum");
  }

  // ---- the limits
  expect(hood_call_ok(0, 1, 1, 1, 1) && hood_call_ok(HOOD_MAX_POINTS, 32, 14, 32, 1000), "the extremes are accepted");
  expect(!hood_call_ok(-1, 1, 1, 1, 1) && !hood_call_ok(HOOD_MAX_POINTS + 1, 1, 1, 1, 1), "n");
  expect(!hood_call_ok(5, 0, 1, 1, 1) && !hood_call_ok(5, 33, 1, 1, 1), "k");
  expect(!hood_call_ok(5, 1, 0, 1, 1) && !hood_call_ok(5, 1, 15, 1, 1), "classes");
  expect(!hood_call_ok(5, 1, 1, 0, 1) && !hood_call_ok(5, 1, 1, 33, 1), "types");
  expect(!hood_call_ok(5, 1, 1, 1, 0) && !hood_call_ok(5, 1, 1, 1, 1001), "iterations");
  expect(hood_neighbour_ok(-1, 5) && hood_neighbour_ok(4, 5) && !hood_neighbour_ok(5, 5) && !hood_neighbour_ok(-2, 5) && !hood_neighbour_ok(INT32_MIN, 5), "neighbour index");
  expect(hood_centre_ok(0) && hood_centre_ok(34000) && !hood_centre_ok(34001) && !hood_centre_ok(-1), "given centre");
  expect(hood_blocks(1) == 1 && hood_blocks(256) == 1 && hood_blocks(257) == 2 && hood_blocks(HOOD_MAX_POINTS) == 65536, "blocks");
  expect(hood_pick_chunk(1) == 1 && hood_pick_chunk(1024) == 1 && hood_pick_chunk(1025) == 2 && hood_pick_chunk(65536) == 64 &&
         (long long)hood_pick_chunk(65536) * HOOD_PICK_NT >= 65536, "the chunks of the pick cover every block");
  expect(HOOD_ONE * 33 <= HOOD_MAX_CENTRE && (long long)HOOD_MAX_CENTRE * HOOD_MAX_CENTRE < (1LL << 31), "a squared term fits 31 bits");

  if (bad) std::printf("%d FAILED\n", bad); else std::printf("cellhood host check ok\n");
  return bad ? 1 : 0;
}
