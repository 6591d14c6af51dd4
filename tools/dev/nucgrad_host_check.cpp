// Host check of the plain-C++ parts of the per-nucleus gradient integers (nuhtc_amd/csrc/nucleus_list.h: the limits of the entry points;
// nucgrad_host.h: the clamped reads of a difference, the integer root, the sector and its step, the bin, the threshold's limits), meant to
// be built with a sanitizer and run on the host -- it never touches a GPU:
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I nuhtc_amd/csrc tools/dev/nucgrad_host_check.cpp -o /tmp/nucgrad_host_check && /tmp/nucgrad_host_check
//
// The row of a small masked image of h values is taken the way the kernel takes it (one bit-packed word at a time, the padding bits of the
// last word masked, a set-bit loop, every read of h through nucgrad_lo / nucgrad_hi into an exactly sized heap array, the bins into an
// exactly sized row), so a read past the frame or an index past the row is reported, and compared with a count over all pixels that
// writes the definition out case by case.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

#include "nucgrad_host.h"

static int plain_root(long long v) {
  int r = 0;
  while ((long long)(r + 1) * (r + 1) <= v) ++r;
  return r;
}

static int check_image(int H, int W, std::mt19937& rng, int density, int kind, int thr, const char* what) {
  const int wpr = (W + 31) / 32;
  std::vector<uint32_t> m((size_t)H * wpr);
  std::unique_ptr<uint8_t[]> h(new uint8_t[(size_t)H * W]);
  for (auto& v : m) v = density >= 100 ? ~0u : (uint32_t)rng() | (density > 50 ? (uint32_t)rng() : 0u);   // padding bits set too: they must not count
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x)
      h[(size_t)y * W + x] = kind == 0 ? (uint8_t)(rng() & 255) : kind == 1 ? (uint8_t)(((x + y) & 1) * 255) : kind == 2 ? (uint8_t)(((x >> 1) & 1) * 200) : (uint8_t)77;
  const unsigned last = (W & 31) ? (1u << (W & 31)) - 1u : ~0u;
  auto at = [&](int x, int y) { return (int)h[(size_t)y * W + x]; };
  // ---- the kernel's way
  auto q_of = [&](int x, int y, int& gx2, int& gy2) {
    gx2 = (at(nucgrad_hi(x, W), y) - at(nucgrad_lo(x), y)) * nucgrad_weight(x, W);
    gy2 = (at(x, nucgrad_hi(y, H)) - at(x, nucgrad_lo(y))) * nucgrad_weight(y, H);
    return gx2 * gx2 + gy2 * gy2;
  };
  auto q_or_zero = [&](int x, int y) {
    if (x < 0 || x >= W || y < 0 || y >= H) return 0;
    int a, b;
    return q_of(x, y, a, b);
  };
  std::unique_ptr<long long[]> got(new long long[NUCGRAD_ROW]()), want(new long long[NUCGRAD_ROW]());
  int mn = NUCGRAD_M_MAX, mx = 0;
  for (int pass = 0; pass < 2; ++pass)
    for (int y = 0; y < H; ++y)
      for (int w = 0; w < wpr; ++w) {
        uint32_t v = m[(size_t)y * wpr + w];
        if (w == wpr - 1) v &= last;
        for (; v; v &= v - 1) {
          const int x = w * 32 + __builtin_ctz(v);
          int gx2, gy2;
          const int q = q_of(x, y, gx2, gy2), mag = nucgrad_mag(q);
          if (q < 0 || q > NUCGRAD_Q_MAX || mag > NUCGRAD_M_MAX) { std::printf("FAIL %s: q %d m %d out of range\n", what, q, mag); return 1; }
          if (pass == 1) { ++got[NUCGRAD_HIST + nucgrad_bin(mag, mn, mx)]; continue; }
          const long long m1 = mag;
          ++got[0]; got[1] += m1; got[2] += m1 * m1; got[3] += m1 * m1 * m1; got[4] += m1 * m1 * m1 * m1;
          mn = mag < mn ? mag : mn; mx = mag > mx ? mag : mx;
          if (mag >= thr) {
            int dx, dy;
            nucgrad_step(nucgrad_sector(gx2, gy2), dx, dy);
            if (q > q_or_zero(x + dx, y + dy) && q >= q_or_zero(x - dx, y - dy)) ++got[7];
          }
        }
      }
  if (got[0]) { got[5] = mn; got[6] = mx; }
  // ---- the definition over all pixels
  std::vector<int> Q((size_t)H * W), GX((size_t)H * W), GY((size_t)H * W), M((size_t)H * W);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      int gx, gy;
      if (W == 1) gx = 0; else if (x == 0) gx = 2 * (at(1, y) - at(0, y)); else if (x == W - 1) gx = 2 * (at(W - 1, y) - at(W - 2, y)); else gx = at(x + 1, y) - at(x - 1, y);
      if (H == 1) gy = 0; else if (y == 0) gy = 2 * (at(x, 1) - at(x, 0)); else if (y == H - 1) gy = 2 * (at(x, H - 1) - at(x, H - 2)); else gy = at(x, y + 1) - at(x, y - 1);
      const size_t i = (size_t)y * W + x;
      GX[i] = gx; GY[i] = gy; Q[i] = gx * gx + gy * gy; M[i] = plain_root(4ll * Q[i]);
    }
  auto set = [&](int y, int x) { return ((m[(size_t)y * wpr + (x >> 5)] >> (x & 31)) & 1u) != 0; };
  auto Qz = [&](int x, int y) { return x < 0 || x >= W || y < 0 || y >= H ? 0 : Q[(size_t)y * W + x]; };
  int lo = 1 << 30, hi = -1;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      if (!set(y, x)) continue;
      const size_t i = (size_t)y * W + x;
      const long long m1 = M[i];
      ++want[0]; want[1] += m1; want[2] += m1 * m1; want[3] += m1 * m1 * m1; want[4] += m1 * m1 * m1 * m1;
      lo = M[i] < lo ? M[i] : lo; hi = M[i] > hi ? M[i] : hi;
      if (M[i] < thr) continue;
      const long long ax = std::abs(GX[i]), ay = std::abs(GY[i]);
      int x1, y1, x2, y2;
      if (ay * 32768 < ax * 13573) { x1 = x - 1; y1 = y; x2 = x + 1; y2 = y; }
      else if (ay * 32768 > ax * 13573 + ax * 65536) { x1 = x; y1 = y - 1; x2 = x; y2 = y + 1; }
      else if ((long long)GX[i] * GY[i] > 0) { x1 = x - 1; y1 = y - 1; x2 = x + 1; y2 = y + 1; }
      else { x1 = x + 1; y1 = y - 1; x2 = x - 1; y2 = y + 1; }
      if (Q[i] > Qz(x1, y1) && Q[i] >= Qz(x2, y2)) ++want[7];
    }
  if (want[0]) {
    want[5] = lo; want[6] = hi;
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        if (!set(y, x)) continue;
        const int v = M[(size_t)y * W + x];
        int bin = 5;
        if (hi > lo) { bin = (v - lo) * 10 / (hi - lo); if (bin > 9) bin = 9; }
        ++want[8 + bin];
      }
  }
  for (int i = 0; i < NUCGRAD_ROW; ++i)
    if (got[i] != want[i]) { std::printf("FAIL %s %d x %d thr %d: word %d holds %lld, all pixels give %lld\n", what, H, W, thr, i, got[i], want[i]); return 1; }
  return 0;
}

int main() {
  int bad = 0;
  // ---- limits: those of the other readers of tile pixels, and the threshold
  struct { int B, K, H, W, pitch, n, mode, thr; bool ok; } cases[] = {
      {1, 1, 1, 1, 1, 1, 0, 1, true},          {4096, 65536, 1024, 1024, 1024, 1 << 24, 1, 1442, true}, {0, 1, 8, 8, 8, 1, 0, 1, false},
      {4097, 1, 8, 8, 8, 1, 0, 1, false},      {1, 0, 8, 8, 8, 1, 0, 1, false},                         {1, 65537, 8, 8, 8, 1, 0, 1, false},
      {1, 1, 0, 8, 8, 1, 0, 1, false},         {1, 1, 1025, 8, 8, 1, 0, 1, false},                      {1, 1, 8, 0, 8, 1, 0, 1, false},
      {1, 1, 8, 1025, 1025, 1, 0, 1, false},   {1, 1, 8, 8, 7, 1, 0, 1, false},                         {1, 1, 8, 8, 8, 0, 0, 1, false},
      {1, 1, 8, 8, 8, (1 << 24) + 1, 0, 1, false}, {1, 1, 8, 8, 8, 1, 2, 1, false},                     {1, 1, 8, 8, 8, 1, -1, 1, false},
      {1, 1, 8, 8, 8, 1, 0, 0, false},         {1, 1, 8, 8, 8, 1, 0, 1443, false},                      {1, 1, 8, 8, 8, 1, 0, -2147483647 - 1, false},
      {1, 1, 8, 8, 8, 1, 0, 2147483647, false}, {1, 1, 8, 8, 8, 1, 0, 700, true},                       {1, 1, 2147483647, 2147483647, 2147483647, 1, 0, 1, false}};
  for (const auto& c : cases)
    if (nucgrad_args_error(c.B, c.K, c.H, c.W, c.pitch, c.n, c.mode, c.thr).empty() != c.ok) { std::printf("FAIL limits B %d K %d H %d W %d thr %d\n", c.B, c.K, c.H, c.W, c.thr); ++bad; }
  // ---- the root: the exact floor for every q a pixel can have
  for (int q = 0; q <= NUCGRAD_Q_MAX; ++q) {
    const long long r = nucgrad_mag(q);
    if (r * r > 4ll * q || (r + 1) * (r + 1) <= 4ll * q) { std::printf("FAIL root of 4 x %d = %lld\n", q, r); ++bad; break; }
  }
  if (nucgrad_mag(NUCGRAD_Q_MAX) != NUCGRAD_M_MAX) { std::printf("FAIL the largest magnitude\n"); ++bad; }
  // ---- the bin: inside the row for every range and value, first and last bin reached
  for (int mn = 0; mn <= NUCGRAD_M_MAX; mn += 103)
    for (int mx = mn; mx <= NUCGRAD_M_MAX; ++mx)
      for (int v = mn; v <= mx; ++v) {
        const int b = nucgrad_bin(v, mn, mx);
        if (b < 0 || b >= NUCGRAD_BINS || (mx > mn && ((v == mn && b != 0) || (v == mx && b != NUCGRAD_BINS - 1))) || (mx == mn && b != 5)) {
          std::printf("FAIL bin of %d in [%d, %d] = %d\n", v, mn, mx, b); ++bad; mx = NUCGRAD_M_MAX; break;
        }
      }
  // ---- the sector: every doubled gradient a pixel can have gives one of four, and the steps are the listed ones
  for (int gx = -510; gx <= 510; ++gx)
    for (int gy = -510; gy <= 510; ++gy) {
      const int s = nucgrad_sector(gx, gy);
      int dx, dy;
      nucgrad_step(s, dx, dy);
      const int ex[4] = {-1, 0, -1, 1}, ey[4] = {0, -1, -1, -1};
      if (s < 0 || s > 3 || dx != ex[s] || dy != ey[s]) { std::printf("FAIL sector of (%d, %d) = %d, step (%d, %d)\n", gx, gy, s, dx, dy); ++bad; gx = 511; break; }
    }
  if (nucgrad_sector(10, 0) != 0 || nucgrad_sector(-10, 4) != 0 || nucgrad_sector(0, 7) != 1 || nucgrad_sector(3, -10) != 1 || nucgrad_sector(5, 5) != 2 ||
      nucgrad_sector(-5, -6) != 2 || nucgrad_sector(5, -5) != 3 || nucgrad_sector(-6, 5) != 3) { std::printf("FAIL sectors by hand\n"); ++bad; }
  // ---- rows of small images against a count over all pixels: widths round the word boundary, one row, one column, one pixel
  std::mt19937 rng(13);
  const int sizes[][2] = {{1, 1}, {1, 2}, {2, 1}, {1, 33}, {64, 40}, {7, 31}, {7, 32}, {7, 33}, {5, 64}, {3, 65}, {40, 1}, {33, 96}, {2, 2}};
  for (const auto& s : sizes)
    for (int density : {50, 75, 100})
      for (int kind = 0; kind < 4; ++kind)
        for (int thr : {1, 300, 1442}) bad += check_image(s[0], s[1], rng, density, kind, thr, density == 100 ? "full" : "random");
  if (bad) std::printf("%d FAILED\n", bad); else std::printf("nucgrad host check ok\n");
  return bad ? 1 : 0;
}
