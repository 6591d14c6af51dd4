// Host check of the plain-C++ parts of the per-nucleus texture counts (nuhtc_amd/csrc/nucleus_list.h: the limits of the entry points;
// nuctex_host.h: nuctex_cell, the index the kernel adds at), meant to be built with a sanitizer and run on the host -- it never touches a GPU:
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I nuhtc_amd/csrc tools/dev/nuctex_host_check.cpp -o /tmp/nuctex_host_check && /tmp/nuctex_host_check
//
// The counts of a small masked level image are taken the way the kernel takes them (the pair words R and D of bit-packed rows, the
// padding bits of the last word masked, one add per set bit at nuctex_cell) into an exactly sized heap array of NUCTEX_ROW counters, so an
// index past a record is reported, and compared with a count over all pixel pairs.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

#include "nuctex_host.h"

static int check_image(int H, int W, std::mt19937& rng, int density, const char* what) {
  const int wpr = (W + 31) / 32;
  std::vector<uint32_t> m((size_t)H * wpr);
  std::vector<uint8_t> q((size_t)H * W);
  for (auto& v : m) v = density >= 100 ? ~0u : (uint32_t)rng() | (density > 50 ? (uint32_t)rng() : 0u);   // padding bits set too: they must not count
  for (auto& v : q) v = (uint8_t)(rng() % NUCTEX_LEVELS);
  const unsigned last = (W & 31) ? (1u << (W & 31)) - 1u : ~0u;
  auto word = [&](int y, int w) -> uint32_t {
    if (y >= H || w >= wpr) return 0u;
    const uint32_t v = m[(size_t)y * wpr + w];
    return w == wpr - 1 ? v & last : v;
  };
  std::unique_ptr<int32_t[]> got(new int32_t[NUCTEX_ROW]()), want(new int32_t[NUCTEX_ROW]());
  for (int y = 0; y < H; ++y)
    for (int w = 0; w < wpr; ++w) {
      const uint32_t v = word(y, w), R = v & ((v >> 1) | (word(y, w + 1) << 31)), D = v & word(y + 1, w);
      for (int bit = 0; bit < 32; ++bit) {
        const int x = w * 32 + bit;
        if ((R >> bit) & 1u) ++got[nuctex_cell(q[(size_t)y * W + x], q[(size_t)y * W + x + 1])];
        if ((D >> bit) & 1u) ++got[NUCTEX_CELLS + nuctex_cell(q[(size_t)y * W + x], q[(size_t)(y + 1) * W + x])];
      }
    }
  auto set = [&](int y, int x) { return y < H && x < W && ((m[(size_t)y * wpr + (x >> 5)] >> (x & 31)) & 1u); };
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      if (!set(y, x)) continue;
      const int a = q[(size_t)y * W + x];
      if (set(y, x + 1)) { const int b = q[(size_t)y * W + x + 1]; ++want[(a < b ? a : b) * NUCTEX_LEVELS - (a < b ? a : b) * ((a < b ? a : b) - 1) / 2 + abs(a - b)]; }
      if (set(y + 1, x)) { const int b = q[(size_t)(y + 1) * W + x]; ++want[NUCTEX_CELLS + (a < b ? a : b) * NUCTEX_LEVELS - (a < b ? a : b) * ((a < b ? a : b) - 1) / 2 + abs(a - b)]; }
    }
  for (int i = 0; i < NUCTEX_ROW; ++i)
    if (got[i] != want[i]) { std::printf("FAIL %s %d x %d: cell %d holds %d, all pairs give %d\n", what, H, W, i, got[i], want[i]); return 1; }
  return 0;
}

int main() {
  int bad = 0;
  // ---- limits
  struct { int B, K, H, W, pitch, n, mode; bool ok; } cases[] = {
      {1, 1, 1, 1, 1, 1, 0, true},         {4096, 65536, 1024, 1024, 1024, 1 << 24, 1, true}, {0, 1, 8, 8, 8, 1, 0, false},
      {4097, 1, 8, 8, 8, 1, 0, false},     {1, 0, 8, 8, 8, 1, 0, false},                      {1, 65537, 8, 8, 8, 1, 0, false},
      {1, 1, 0, 8, 8, 1, 0, false},        {1, 1, 1025, 8, 8, 1, 0, false},                   {1, 1, 8, 0, 8, 1, 0, false},
      {1, 1, 8, 1025, 1025, 1, 0, false},  {1, 1, 8, 8, 7, 1, 0, false},                      {1, 1, 8, 8, 1025, 1, 0, false},
      {1, 1, 8, 8, 8, 0, 0, false},        {1, 1, 8, 8, 8, (1 << 24) + 1, 0, false},          {1, 1, 8, 8, 8, 1, 2, false},
      {1, 1, 8, 8, 8, 1, -1, false},       {-2147483647 - 1, 1, 8, 8, 8, 1, 0, false},        {1, 1, 2147483647, 2147483647, 2147483647, 1, 0, false}};
  for (const auto& c : cases)
    if (nucleus_sizes_error("nucleus_texture", c.B, c.K, c.H, c.W, c.pitch, c.n, c.mode).empty() != c.ok) { std::printf("FAIL limits B %d K %d H %d W %d\n", c.B, c.K, c.H, c.W); ++bad; }
  // ---- the triangle index: every unordered pair of levels has its own cell, in row-major order, and none lies past the triangle
  {
    int next = 0;
    for (int a = 0; a < NUCTEX_LEVELS; ++a)
      for (int b = a; b < NUCTEX_LEVELS; ++b) {
        if (nuctex_cell(a, b) != next || nuctex_cell(b, a) != next) { std::printf("FAIL cell (%d, %d) = %d, expected %d\n", a, b, nuctex_cell(a, b), next); ++bad; }
        ++next;
      }
    if (next != NUCTEX_CELLS) { std::printf("FAIL %d cells\n", next); ++bad; }
  }
  // ---- the pair words against a count over all pixel pairs: widths around the word boundary, one row, one column, the full frame
  std::mt19937 rng(11);
  const int sizes[][2] = {{1, 1}, {1, 2}, {2, 1}, {1, 33}, {64, 40}, {7, 31}, {7, 32}, {7, 33}, {5, 64}, {3, 65}, {40, 1}, {33, 96}};
  for (const auto& s : sizes)
    for (int density : {50, 75, 100}) bad += check_image(s[0], s[1], rng, density, density == 100 ? "full" : "random");
  if (bad) std::printf("%d FAILED\n", bad); else std::printf("nuctex host check ok\n");
  return bad ? 1 : 0;
}
