// Host check of the plain-C++ parts of the neighbourhood enrichment (nuhtc_amd/csrc/cellenrich_host.h: the generator -- fmix, the round
// keys, the Feistel network and the cycle-walk --, the nibble packing, the LDS table index, the flush interval and the limits), meant to
// be built with a sanitizer and run on the host -- it never touches a GPU, and the kernel code itself (cellenrich.hip) is NOT sanitized:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I nuhtc_amd/csrc tools/dev/cellenrich_host_check.cpp \
//       -o /tmp/cellenrich_host_check && /tmp/cellenrich_host_check
//
// Five parts.  The generator: F is a bijection of 0 .. 4^h - 1 for every h that fits a loop; pi is a bijection of 0 .. n - 1 for every
// n in 1 .. 2050 and for 4097, 65536, 65537, 70000, 500000 and 2^24 at several (seed, p), the identity for n <= 1, different for
// different p and seeds, every walk ends (the longest is printed), and a few values written out by hand from the definition
// (nuhtc_amd/enrichment.py gives the same).  The packing: every class in every slot round-trips and leaves the other slots alone.  The
// table: ce_table_at is a bijection onto 0 .. slots x (C + 1)^2 - 1 inside CE_TABLE_WORDS, and the counts a sweep would take through it
// on a small point set, decoded the way the flush decodes them, equal the counts taken directly.  The flush interval: never past
// 2^32 - 1 adds to one entry, and at least one block.  The limits at their last accepted and first refused values.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "cellenrich_host.h"

int main() {
  int bad = 0;
  auto expect = [&](bool ok, const char* what) { if (!ok) { std::printf("FAIL %s\n", what); ++bad; } };

  // ---- fmix and the keys: values worked out from the definition
  expect(ce_fmix(0u) == 0u && ce_fmix(1u) == 0x514E28B7u && ce_fmix(0xFFFFFFFFu) == 0x81F16F39u, "fmix at 0, 1 and 2^32 - 1");
  {
    uint32_t key[CE_ROUNDS], again[CE_ROUNDS];
    ce_keys(0u, 1u, key);
    expect(key[0] == ce_fmix(ce_fmix(0x9E3779B9u) + 0x7F4A7C15u) && key[5] == ce_fmix(ce_fmix(0x9E3779B9u) + 6u * 0x7F4A7C15u), "keys of (0, 1)");
    ce_keys(0xFFFFFFFFu, 1024u, again);                  // seed + 0x9E3779B9 * p wraps
    expect(again[0] == ce_fmix(ce_fmix(0xFFFFFFFFu + 0x9E3779B9u * 1024u) + 0x7F4A7C15u) && again[0] != key[0], "keys wrap mod 2^32");
  }
  expect(ce_half_bits(2) == 1 && ce_half_bits(4) == 1 && ce_half_bits(5) == 2 && ce_half_bits(16) == 2 && ce_half_bits(17) == 3 &&
         ce_half_bits(1025) == 6 && ce_half_bits(4097) == 7 && ce_half_bits(1u << 24) == 12, "half bits");

  // ---- F is a bijection of 0 .. 4^h - 1
  for (int h = 1; h <= 10; ++h) {
    uint32_t key[CE_ROUNDS];
    ce_keys(77u + h, 3u, key);
    const uint32_t size = 1u << (2 * h);
    std::vector<char> hit(size, 0);
    bool ok = true;
    for (uint32_t x = 0; x < size; ++x) {
      const uint32_t y = ce_feistel(x, h, key);
      if (y >= size || hit[y]) { ok = false; break; }
      hit[y] = 1;
    }
    expect(ok, "F is a bijection");
  }

  // ---- pi is a bijection, the walk ends
  const uint32_t seeds[3] = {0u, 2024u, 0xFFFFFFFFu};
  const int perms[3] = {1, 2, 1024};
  int longest = 0;
  auto bijection = [&](int64_t n, uint32_t seed, int p) {
    std::vector<int32_t> out((size_t)std::max<int64_t>(n, 1), -1);
    if (!ce_fill_permutation(n, seed, p, out.data())) return false;
    std::vector<char> hit((size_t)n, 0);
    uint32_t key[CE_ROUNDS];
    ce_keys(seed, (uint32_t)p, key);
    const int h = n > 1 ? ce_half_bits((uint32_t)n) : 1;
    if (n > 1 && ((int64_t)1 << (2 * h)) >= 4 * n) return false;       // 4^h < 4 n: the expected walk is under four steps
    for (int64_t i = 0; i < n; ++i) {
      int steps = 0;
      const uint32_t v = ce_permute((uint32_t)i, (uint32_t)n, h, key, &steps);
      longest = std::max(longest, steps);
      if ((int32_t)v != out[i] || v >= n || hit[v]) return false;
      hit[v] = 1;
    }
    return true;
  };
  for (int64_t n = 1; n <= 2050; ++n)
    for (int c = 0; c < 3; ++c) expect(bijection(n, seeds[c], perms[c]), "pi is a bijection, n <= 2050");
  for (int64_t n : {(int64_t)4097, (int64_t)65536, (int64_t)65537, (int64_t)70000, (int64_t)500000, CE_MAX_POINTS})
    for (int c = 0; c < (n > 500000 ? 1 : 3); ++c) expect(bijection(n, seeds[c], perms[c]), "pi is a bijection, larger n");
  std::printf("longest walk: %d applications of F\n", longest);
  {
    int32_t one = 7, a[300], b[300], c[300];
    expect(ce_fill_permutation(0, 5u, 1, nullptr) && ce_fill_permutation(1, 5u, 9, &one) && one == 0, "identity for n <= 1");
    ce_fill_permutation(300, 5u, 1, a); ce_fill_permutation(300, 5u, 2, b); ce_fill_permutation(300, 6u, 1, c);
    expect(!std::equal(a, a + 300, b) && !std::equal(a, a + 300, c) && !std::equal(b, b + 300, c), "different p and seeds differ");
    bool identity = true;
    for (int i = 0; i < 300; ++i) identity &= a[i] == i;
    expect(!identity, "a shuffle is not the identity");
  }

  // ---- the nibble packing
  for (int slot = 0; slot < CE_BATCH; ++slot)
    for (int cls = 0; cls <= CE_MAX_CLASSES; ++cls) {
      const unsigned long long full = 0x3333333333333333ull & ~(15ull << (4 * slot));      // class 3 in every other slot
      const unsigned long long w = ce_pack(full, slot, cls);
      bool ok = ce_unpack(w, slot) == cls && ce_unpack(ce_pack(0, slot, cls), slot) == cls;
      for (int other = 0; other < CE_BATCH; ++other)
        if (other != slot) ok &= ce_unpack(w, other) == 3 && ce_unpack(ce_pack(0, slot, cls), other) == 0;
      expect(ok, "pack / unpack");
    }

  // ---- the table index
  for (int C = 1; C <= CE_MAX_CLASSES; ++C) {
    const int K = ce_slot_words(C), total = (CE_BATCH + 1) * K;
    std::vector<char> hit((size_t)total, 0);
    bool ok = total <= CE_TABLE_WORDS;
    for (int s = 0; s <= CE_BATCH && ok; ++s)
      for (int a = 0; a <= C && ok; ++a)
        for (int b = 0; b <= C && ok; ++b) {
          const int at = ce_table_at(s, a, b, C);
          ok = at >= 0 && at < total && !hit[at] && at / K == s && (at - s * K) / (C + 1) == a && (at - s * K) % (C + 1) == b;
          if (ok) hit[at] = 1;
        }
    expect(ok, "table index");
  }
  expect(CE_TABLE_WORDS == 17 * 15 * 15 && CE_OBS_SLOT == 16, "table size");

  // ---- a sweep on the host through the packing and the table against direct counts
  {
    std::mt19937 rng(11);
    const int n = 90, C = 3, r = 9, ns = 5, K = ce_slot_words(C);
    std::vector<int> x(n), y(n), lab(n);
    for (int i = 0; i < n; ++i) { x[i] = (int)(rng() % 40); y[i] = (int)(rng() % 40); lab[i] = (int)(rng() % 5) - 1; }      // -1 and 3: no class
    const int h = ce_half_bits(n);
    std::vector<unsigned long long> nib(n, 0);
    std::vector<std::vector<int>> shuffled(ns, std::vector<int>(n));
    for (int s = 0; s < ns; ++s) {
      uint32_t key[CE_ROUNDS];
      ce_keys(3u, (uint32_t)(s + 1), key);
      for (int i = 0; i < n; ++i) {
        shuffled[s][i] = lab[ce_permute((uint32_t)i, n, h, key)];
        nib[i] = ce_pack(nib[i], s, cs_class(shuffled[s][i], C));
      }
    }
    std::vector<unsigned> table(CE_TABLE_WORDS, 0);
    std::vector<long long> direct((size_t)(ns + 1) * C * C, 0), decoded((size_t)(ns + 1) * C * C, 0);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        if (i == j || cell_pair_d2(x[j] - x[i], y[j] - y[i], r, r * r) < 0) continue;
        for (int s = 0; s < ns; ++s) {
          table[ce_table_at(s, ce_unpack(nib[i], s), ce_unpack(nib[j], s), C)] += 1;
          const int a = shuffled[s][i], b = shuffled[s][j];
          if (a >= 0 && a < C && b >= 0 && b < C) direct[(size_t)(s * C + a) * C + b] += 1;
        }
        table[ce_table_at(CE_OBS_SLOT, cs_class(lab[i], C), cs_class(lab[j], C), C)] += 1;
        if (lab[i] >= 0 && lab[i] < C && lab[j] >= 0 && lab[j] < C) direct[(size_t)(ns * C + lab[i]) * C + lab[j]] += 1;
      }
    long long kept = 0;
    for (int i = 0; i < (CE_BATCH + 1) * K; ++i) {       // the flush's decoding
      const int s = i / K, rem = i - s * K, a = rem / (C + 1), b = rem - a * (C + 1);
      if (!table[i] || a >= C || b >= C) continue;
      expect(s < ns || s == CE_OBS_SLOT, "an idle slot stays empty");
      decoded[(size_t)((s == CE_OBS_SLOT ? ns : s) * C + a) * C + b] += table[i];
      kept += table[i];
    }
    expect(decoded == direct && kept > 0, "the table's counts equal the direct counts");
  }

  // ---- the flush interval: blocks x 256 x (n - 1) <= 2^32 - 1, at least one block
  for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)257, (int64_t)70000, (int64_t)500000, (int64_t)262144, (int64_t)262145, CE_MAX_POINTS - 1,
                    CE_MAX_POINTS}) {
    const int k = ce_flush_blocks(n);
    expect(k >= 1 && k <= CE_MAX_FLUSH_BLOCKS && (n <= 1 || (int64_t)k * CE_NT * (n - 1) <= 0xFFFFFFFFLL), "flush interval");
  }
  expect(ce_flush_blocks(CE_MAX_POINTS) == 1 && (int64_t)CE_NT * (CE_MAX_POINTS - 1) == 0x100000000LL - 256, "one block at the largest n");

  // ---- the limits at their last accepted and first refused values
  expect(ce_perms_ok(1) && ce_perms_ok(1024) && !ce_perms_ok(0) && !ce_perms_ok(1025) && !ce_perms_ok(-1), "perms");
  expect(ce_batches(1) == 1 && ce_batches(16) == 1 && ce_batches(17) == 2 && ce_batches(1000) == 63 && ce_batches(1024) == 64, "batches");
  const int L = CELL_COORD_LIMIT;
  expect(cell_call_ok(CE_MAX_POINTS, CE_MAX_POINTS, 14, 16384, -(L - 1), -(L - 1), L - 1, L - 1), "largest accepted call");
  expect(!cell_call_ok(CE_MAX_POINTS + 1, CE_MAX_POINTS, 14, 16384, 0, 0, 1, 1) && !cell_call_ok(-1, CE_MAX_POINTS, 1, 1, 0, 0, 1, 1), "n");
  expect(cell_call_ok(3, CE_MAX_POINTS, 1, 1, 0, 0, 1, 1) && !cell_call_ok(3, CE_MAX_POINTS, 0, 1, 0, 0, 1, 1) && !cell_call_ok(3, CE_MAX_POINTS, 15, 1, 0, 0, 1, 1), "classes");
  expect(!cell_call_ok(3, CE_MAX_POINTS, 1, 0, 0, 0, 1, 1) && !cell_call_ok(3, CE_MAX_POINTS, 1, 16385, 0, 0, 1, 1), "radius");
  expect(!cell_call_ok(3, CE_MAX_POINTS, 1, 1, -L, 0, 1, 1) && !cell_call_ok(3, CE_MAX_POINTS, 1, 1, 0, 0, 1, L) && !cell_call_ok(3, CE_MAX_POINTS, 1, 1, 2, 0, 1, 1), "box");
  {
    int32_t out[4];
    expect(ce_fill_permutation(4, 0u, 1024, out) && !ce_fill_permutation(4, 0u, 0, out) && !ce_fill_permutation(4, 0u, 1025, out) &&
           !ce_fill_permutation(-1, 0u, 1, out) && !ce_fill_permutation(CE_MAX_POINTS + 1, 0u, 1, out) && !ce_fill_permutation(4, 0u, 1, nullptr), "generator arguments");
  }

  if (bad) std::printf("%d FAILED\n", bad); else std::printf("cellenrich host check ok\n");
  return bad ? 1 : 0;
}
