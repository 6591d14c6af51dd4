// Host check of the plain-C++ parts of the per-nucleus shape integers (nuhtc_amd/csrc/nucleus_list.h: the limits of the entry point;
// nucshape_host.h: the geometry of the box pyramid, the aligned read of a mask word, the pair-compress, the two front levels, a further
// level from its four children), meant to be built with a sanitizer and run on the host -- it never touches a GPU:
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I nuhtc_amd/csrc tools/dev/nucshape_host_check.cpp -o /tmp/nucshape_host_check && /tmp/nucshape_host_check
//
// The ten box counts of a mask are taken the way the kernel takes them (the rectangle, then one level-2 word at a time from four mask
// rows read through nucshape_aligned_word out of an exactly sized heap array, the kept levels in planes of exactly NUCSHAPE_PLANE words
// at nucshape_base, every further level from its four children), so a read past the mask or an index past a level is reported, and
// compared with a count that visits every position of every box.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

#include "nucshape_host.h"

struct Mask {
  int H, W, wpr;
  std::unique_ptr<uint32_t[]> w;       // exactly H * wpr words
  Mask(int H_, int W_) : H(H_), W(W_), wpr((W_ + 31) / 32), w(new uint32_t[(size_t)H_ * ((W_ + 31) / 32)]()) {}
  bool at(int x, int y) const { return x < W && ((w[(size_t)y * wpr + (x >> 5)] >> (x & 31)) & 1u) != 0; }
  void set(int x, int y) { w[(size_t)y * wpr + (x >> 5)] |= 1u << (x & 31); }
  void dirty_padding() { if (W & 31) for (int y = 0; y < H; ++y) w[(size_t)y * wpr + wpr - 1] |= ~0u << (W & 31); }
};

// the kernel's way: -> false when the mask is empty
static bool kernel_way(const Mask& M, long long n[NUCSHAPE_LEVELS], int rect[4]) {
  const uint32_t last = (M.W & 31) ? (1u << (M.W & 31)) - 1u : ~0u;
  int x0 = 1 << 30, y0 = 1 << 30, x1 = -1, y1 = -1;
  for (int y = 0; y < M.H; ++y)
    for (int cw = 0; cw < M.wpr; ++cw) {
      uint32_t v = M.w[(size_t)y * M.wpr + cw];
      if (cw == M.wpr - 1) v &= last;
      if (!v) continue;
      y0 = y < y0 ? y : y0; y1 = y > y1 ? y : y1;
      const int lo = cw * 32 + __builtin_ctz(v), hi = cw * 32 + 31 - __builtin_clz(v);
      x0 = lo < x0 ? lo : x0; x1 = hi > x1 ? hi : x1;
    }
  for (int k = 0; k < NUCSHAPE_LEVELS; ++k) n[k] = 0;
  if (x1 < 0) return false;
  const int w = x1 - x0 + 1, h = y1 - y0 + 1, wx1 = x1 >> 5;
  rect[0] = x0; rect[1] = y0; rect[2] = x0 + w; rect[3] = y0 + h;
  std::unique_ptr<uint32_t[]> any_pl(new uint32_t[NUCSHAPE_PLANE]), all_pl(new uint32_t[NUCSHAPE_PLANE]);
  {
    const int R = nucshape_rows(h, 2), P = nucshape_words(w, 2);
    if (R * P > nucshape_level_words(2)) { std::printf("FAIL level 2 of %d x %d does not fit\n", w, h); std::exit(1); }
    for (int i = 0; i < R * P; ++i) {
      const int r2 = i / P, k2 = i - r2 * P;
      uint32_t px[4][4];
      for (int t = 0; t < 4; ++t)
        for (int a = 0; a < 4; ++a) {
          const int v = 4 * r2 + t;
          px[t][a] = v < h ? nucshape_aligned_word(M.w.get() + (size_t)(y0 + v) * M.wpr, x0, 4 * k2 + a, wx1, M.wpr, last) : 0u;
        }
      uint32_t any2, all2;
      int n1, n2;
      nucshape_front(px, any2, all2, n1, n2);
      n[0] += n1; n[1] += n2;
      any_pl[i] = any2; all_pl[i] = all2;
    }
  }
  for (int L = 3; L <= NUCSHAPE_LEVELS; ++L) {
    const int Rc = nucshape_rows(h, L - 1), Pc = nucshape_words(w, L - 1), R = nucshape_rows(h, L), P = nucshape_words(w, L);
    if (R * P > nucshape_level_words(L)) { std::printf("FAIL level %d of %d x %d does not fit\n", L, w, h); std::exit(1); }
    const uint32_t* ca = any_pl.get() + nucshape_base(L - 1);
    const uint32_t* cl = all_pl.get() + nucshape_base(L - 1);
    for (int i = 0; i < R * P; ++i) {
      const int rr = i / P, k = i - rr * P, r0 = 2 * rr, r1 = r0 + 1, k0 = 2 * k, k1 = k0 + 1;
      if (r0 >= Rc || k0 >= Pc) { std::printf("FAIL level %d of %d x %d: a first child outside its level\n", L, w, h); std::exit(1); }
      const bool hr = r1 < Rc, hk = k1 < Pc;
      uint32_t any, all;
      nucshape_parent(ca[r0 * Pc + k0], hk ? ca[r0 * Pc + k1] : 0u, hr ? ca[r1 * Pc + k0] : 0u, hr && hk ? ca[r1 * Pc + k1] : 0u,
                      cl[r0 * Pc + k0], hk ? cl[r0 * Pc + k1] : 0u, hr ? cl[r1 * Pc + k0] : 0u, hr && hk ? cl[r1 * Pc + k1] : 0u, any, all);
      n[L - 1] += nucshape_mixed(any, all);
      any_pl[nucshape_base(L) + i] = any; all_pl[nucshape_base(L) + i] = all;
    }
  }
  return true;
}

// the definition: every position of every box
static void plain_way(const Mask& M, const int rect[4], long long n[NUCSHAPE_LEVELS]) {
  for (int j = 1; j <= NUCSHAPE_LEVELS; ++j) {
    const int s = 1 << j;
    n[j - 1] = 0;
    for (int by = rect[1]; by < rect[3]; by += s)
      for (int bx = rect[0]; bx < rect[2]; bx += s) {
        long long got = 0;
        for (int y = by; y < by + s && y < rect[3]; ++y)
          for (int x = bx; x < bx + s && x < rect[2]; ++x) got += M.at(x, y) ? 1 : 0;
        if (got > 0 && got < (long long)s * s) ++n[j - 1];
      }
  }
}

static int check_mask(Mask& M, const char* what, const long long* by_hand = nullptr) {
  M.dirty_padding();                                   // the padding bits of a row's last word must not count
  long long got[NUCSHAPE_LEVELS], want[NUCSHAPE_LEVELS];
  int rect[4] = {0, 0, 0, 0};
  if (!kernel_way(M, got, rect)) {
    for (int y = 0; y < M.H; ++y)
      for (int x = 0; x < M.W; ++x)
        if (M.at(x, y)) { std::printf("FAIL %s: a set pixel and no rectangle\n", what); return 1; }
    return 0;
  }
  plain_way(M, rect, want);
  for (int k = 0; k < NUCSHAPE_LEVELS; ++k) {
    if (got[k] != want[k]) { std::printf("FAIL %s %d x %d: N_%d is %lld, all positions give %lld\n", what, M.H, M.W, k + 1, got[k], want[k]); return 1; }
    if (by_hand && got[k] != by_hand[k]) { std::printf("FAIL %s: N_%d is %lld, by hand %lld\n", what, k + 1, got[k], by_hand[k]); return 1; }
  }
  return 0;
}

int main() {
  int bad = 0;
  // ---- limits: those of the other per-nucleus entries
  struct { int B, K, H, W, n; bool ok; } lim[] = {
      {1, 1, 1, 1, 1, true},      {4096, 65536, 1024, 1024, 1 << 24, true}, {0, 1, 8, 8, 1, false},    {4097, 1, 8, 8, 1, false},
      {1, 0, 8, 8, 1, false},     {1, 65537, 8, 8, 1, false},               {1, 1, 0, 8, 1, false},    {1, 1, 1025, 8, 1, false},
      {1, 1, 8, 0, 1, false},     {1, 1, 8, 1025, 1, false},                {1, 1, 8, 8, 0, false},    {1, 1, 8, 8, (1 << 24) + 1, false},
      {1, 1, 2147483647, 2147483647, 1, false}, {1, 1, 8, -1, 1, false}};
  for (const auto& c : lim)
    if (nucshape_args_error(c.B, c.K, c.H, c.W, c.n).empty() != c.ok) { std::printf("FAIL limits B %d K %d H %d W %d n %d\n", c.B, c.K, c.H, c.W, c.n); ++bad; }
  // ---- the pair-compress against a loop over the bits
  std::mt19937_64 r64(7);
  for (int it = 0; it < 20000; ++it) {
    const uint64_t v = it == 0 ? 0 : it == 1 ? ~0ull : it == 2 ? 0x5555555555555555ull : it == 3 ? 0xaaaaaaaaaaaaaaaaull : r64() & (it & 1 ? r64() : ~0ull);
    uint32_t any = 0, all = 0;
    for (int i = 0; i < 32; ++i) {
      const int a = (int)((v >> (2 * i)) & 1), b = (int)((v >> (2 * i + 1)) & 1);
      any |= (uint32_t)(a | b) << i; all |= (uint32_t)(a & b) << i;
    }
    if (nucshape_pair_any(v) != any || nucshape_pair_all(v) != all) { std::printf("FAIL pair-compress of %llx\n", (unsigned long long)v); ++bad; break; }
  }
  // ---- the geometry: every level of every side fits its place, and the places do not overlap
  for (int L = 2; L <= NUCSHAPE_LEVELS; ++L) {
    if (nucshape_rows(1024, L) * nucshape_words(1024, L) != nucshape_level_words(L)) { std::printf("FAIL level %d words\n", L); ++bad; }
    if (L > 2 && nucshape_base(L) != nucshape_base(L - 1) + nucshape_level_words(L - 1)) { std::printf("FAIL level %d base\n", L); ++bad; }
    for (int s = 1; s <= 1024; ++s)
      if (nucshape_rows(s, L) < 1 || nucshape_rows(s, L) > nucshape_rows(1024, L) || nucshape_words(s, L) < 1 || nucshape_words(s, L) > nucshape_words(1024, L)) {
        std::printf("FAIL level %d of side %d\n", L, s); ++bad; break;
      }
  }
  // ---- designed masks with their counts by hand
  {
    Mask m(5, 7); m.set(4, 3);
    const long long n[10] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
    bad += check_mask(m, "one pixel", n);
  }
  {
    Mask m(12, 40); for (int y = 2; y < 10; ++y) for (int x = 29; x < 37; ++x) m.set(x, y);       // straddles the word boundary
    const long long n[10] = {0, 0, 0, 1, 1, 1, 1, 1, 1, 1};
    bad += check_mask(m, "solid 8 x 8", n);
  }
  {
    Mask m(9, 9); for (int y = 4; y < 7; ++y) for (int x = 2; x < 7; ++x) m.set(x, y);
    const long long n[10] = {4, 2, 1, 1, 1, 1, 1, 1, 1, 1};
    bad += check_mask(m, "solid 5 x 3", n);
  }
  {
    Mask m(20, 24); for (int y = 0; y < 16; ++y) for (int x = 0; x < 16; ++x) if (((x + y) & 1) == 0) m.set(3 + x, 2 + y);
    const long long n[10] = {64, 16, 4, 1, 1, 1, 1, 1, 1, 1};
    bad += check_mask(m, "checkerboard 16 x 16", n);
  }
  { Mask m(1, 1); m.set(0, 0); bad += check_mask(m, "1 x 1 frame"); }
  { Mask m(3, 33); bad += check_mask(m, "empty"); }
  for (int side : {64, 1024}) {                        // the full frame: a solid square of side 2^j counts from level j + 1 on
    Mask m(side, side);
    for (size_t i = 0; i < (size_t)side * m.wpr; ++i) m.w[i] = ~0u;
    long long n[10];
    for (int j = 1; j <= 10; ++j) n[j - 1] = (1 << j) > side ? 1 : 0;
    bad += check_mask(m, "full frame", n);
  }
  // ---- random masks: widths round the word boundary, one row, one column, a rectangle that starts anywhere in a word, the largest frame
  std::mt19937 rng(13);
  const int sizes[][2] = {{1, 2}, {2, 1}, {1, 33}, {64, 40}, {7, 31}, {7, 32}, {7, 33}, {5, 64}, {3, 65}, {40, 1}, {33, 96}, {2, 2}, {130, 257}, {260, 129}};
  for (const auto& s : sizes)
    for (int density : {3, 50, 97})
      for (int rep = 0; rep < 4; ++rep) {
        Mask m(s[0], s[1]);
        const int xa = (int)(rng() % s[1]), xb = (int)(rng() % s[1]), ya = (int)(rng() % s[0]), yb = (int)(rng() % s[0]);
        for (int y = ya < yb ? ya : yb; y <= (ya < yb ? yb : ya); ++y)
          for (int x = xa < xb ? xa : xb; x <= (xa < xb ? xb : xa); ++x)
            if (rep == 0 || (int)(rng() % 100) < density) m.set(x, y);
        bad += check_mask(m, "random");
      }
  {
    Mask m(1024, 1024);
    for (int y = 0; y < 1024; ++y)
      for (int x = 33; x < 1024; ++x) {
        const double dx = (x - 528.5) / 495.5, dy = (y - 511.5) / 512.0, d = dx * dx + dy * dy;
        if ((d <= 1.0 && d > 0.16) || y == 0 || x == 33) m.set(x, y);
      }
    m.set(1023, 1023);
    bad += check_mask(m, "holed ellipse 1024");
  }
  if (bad) std::printf("%d FAILED\n", bad); else std::printf("nucshape host check ok\n");
  return bad ? 1 : 0;
}
