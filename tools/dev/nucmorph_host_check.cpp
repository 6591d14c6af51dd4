// Host check of the plain-C++ parts of the per-nucleus morphometry (nuhtc_amd/csrc/nucleus_list.h: the limits of the entry
// points; nucmorph_host.h: hull_chain2, the hull code the kernel runs), meant to be built with a sanitizer and run on the host -- it never touches a GPU:
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I nuhtc_amd/csrc tools/dev/nucmorph_host_check.cpp -o /tmp/nucmorph_host_check && /tmp/nucmorph_host_check
//
// hull_chain2 runs on exactly sized heap arrays (rows extents, rows + 1 stack entries), so a read or write past either is reported;
// its result is compared with a monotone chain over ALL pixel corners in 64-bit arithmetic.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <utility>
#include <vector>

#include "nucmorph_host.h"

typedef std::pair<long long, long long> Pt;

static long long cross(const Pt& o, const Pt& a, const Pt& b) { return (a.first - o.first) * (b.second - o.second) - (a.second - o.second) * (b.first - o.first); }

static long long hull2_brute(std::vector<Pt> p) {
  std::sort(p.begin(), p.end());
  p.erase(std::unique(p.begin(), p.end()), p.end());
  if (p.size() < 3) return 0;
  std::vector<Pt> h(2 * p.size());
  size_t k = 0;
  for (size_t i = 0; i < p.size(); ++i) { while (k >= 2 && cross(h[k - 2], h[k - 1], p[i]) <= 0) --k; h[k++] = p[i]; }
  for (size_t i = p.size() - 1, t = k + 1; i > 0; --i) { while (k >= t && cross(h[k - 2], h[k - 1], p[i - 1]) <= 0) --k; h[k++] = p[i - 1]; }
  long long a = 0;
  for (size_t i = 0; i + 1 < k; ++i) a += h[i].first * h[i + 1].second - h[i + 1].first * h[i].second;
  return a < 0 ? -a : a;
}

static int check_mask(const std::vector<std::vector<int>>& rows_px, int y_first, const char* what) {
  // rows_px[i]: the set x of pixel row y_first + i (first and last row non-empty)
  const int rows = (int)rows_px.size();
  std::unique_ptr<uint32_t[]> ext(new uint32_t[rows]), st(new uint32_t[rows + 1]);
  std::vector<Pt> corners;
  for (int i = 0; i < rows; ++i) {
    if (rows_px[i].empty()) { ext[i] = NUCMORPH_EMPTY_ROW; continue; }
    const int lo = *std::min_element(rows_px[i].begin(), rows_px[i].end()), hi = *std::max_element(rows_px[i].begin(), rows_px[i].end());
    ext[i] = (uint32_t)lo | ((uint32_t)hi << 16);
    for (int x : rows_px[i])
      for (int dx = 0; dx < 2; ++dx)
        for (int dy = 0; dy < 2; ++dy) corners.push_back(Pt(x + dx, y_first + i + dy));
  }
  const long long got = hull_chain2<true>(ext.get(), rows, st.get()) - hull_chain2<false>(ext.get(), rows, st.get());
  const long long want = hull2_brute(corners);
  if (got != want) { std::printf("FAIL %s: hull2 %lld, brute force %lld\n", what, got, want); return 1; }
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
    if (nucleus_sizes_error("nucleus_morph", c.B, c.K, c.H, c.W, c.pitch, c.n, c.mode).empty() != c.ok) { std::printf("FAIL limits B %d K %d H %d W %d\n", c.B, c.K, c.H, c.W); ++bad; }
  // ---- the hull: designed rows, then random masks up to the largest frame
  bad += check_mask({{5}}, 3, "one pixel");
  bad += check_mask({{0}, {}, {}, {1023}}, 0, "two pixels, empty rows between");
  bad += check_mask({{0, 1023}}, 1023, "one row, both ends");
  {
    std::vector<std::vector<int>> full(1024, std::vector<int>{0, 1023});
    bad += check_mask(full, 0, "full 1024 frame");
    std::vector<std::vector<int>> diag(1024);
    for (int i = 0; i < 1024; ++i) diag[i] = {i};
    bad += check_mask(diag, 0, "diagonal of 1024");
    std::vector<std::vector<int>> disc(1024);                                // a digital disc: every row on the hull's arc
    for (int i = 0; i < 1024; ++i) {
      const double dy = i - 511.5, w = 511.5 * 511.5 - dy * dy;
      const int half = (int)__builtin_sqrt(w > 0 ? w : 0);
      disc[i] = {511 - half, 512 + half};
    }
    bad += check_mask(disc, 0, "disc of 1024");
  }
  std::mt19937 rng(7);
  for (int t = 0; t < 400; ++t) {
    const int rows = 1 + (int)(rng() % (t < 300 ? 40 : 1024)), width = 1 + (int)(rng() % 1024);
    std::vector<std::vector<int>> m(rows);
    for (int i = 0; i < rows; ++i) {
      const int cnt = (i == 0 || i == rows - 1) ? 1 + (int)(rng() % 3) : (int)(rng() % 4);
      for (int k = 0; k < cnt; ++k) m[i].push_back((int)(rng() % width));
    }
    bad += check_mask(m, (int)(rng() % 8), "random");
  }
  if (bad) std::printf("%d FAILED\n", bad); else std::printf("nucmorph host check ok\n");
  return bad ? 1 : 0;
}
