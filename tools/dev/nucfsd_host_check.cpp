// Host check of the plain-C++ parts of the per-nucleus Fourier-descriptor integers (nuhtc_amd/csrc/nucfsd_host.h: the edge classifier,
// the exact sign of p + q sqrt 2, the search of a sample's edge in one chunk, the limits of the entry point), meant to be built with a
// sanitizer and run on the host -- it never touches a GPU:
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I nuhtc_amd/csrc tools/dev/nucfsd_host_check.cpp -o /tmp/nucfsd_host_check && /tmp/nucfsd_host_check
//
// The sign is compared with the same decision in __int128 over the Pell convergents of sqrt 2 (p^2 - 2 q^2 = +-1: the pairs nearest to
// zero), their neighbours and random pairs up to the limit 2^7 (2^24 - 1), where a signed overflow would be reported.  The rows of rings
// are taken the way the kernel takes them (the totals, then chunk after chunk of NUCFSD_CHUNK edges with a running carry, the cumulative
// pairs of a chunk in heap arrays of exactly the chunk's length, a sample placed in the chunk whose successor starts beyond it), so a read
// past a chunk is reported, and compared with a plain loop over all edges.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

#include "nucfsd_host.h"

static int sign128(int64_t p, int64_t q) {
  if (p == 0 && q == 0) return 0;
  const __int128 pp = (__int128)p * p, qq = (__int128)2 * q * q;
  if (p >= 0 && q >= 0) return 1;
  if (p <= 0 && q <= 0) return -1;
  return p > 0 ? (pp > qq ? 1 : -1) : (qq > pp ? 1 : -1);
}

static const int DX[8] = {1, 1, 0, -1, -1, -1, 0, 1}, DY[8] = {0, -1, -1, -1, 0, 1, 1, 1};
typedef std::vector<int32_t> Ring;       // x0 y0 x1 y1 ..

struct Row { int status; int64_t A, B; int n; std::vector<int> s; };       // s: five numbers a sample

static void edge_of(const Ring& r, int n, int e, int& x, int& y, int64_t& steps, bool& diag, int& code, bool& on) {
  const int nx = e + 1 < n ? e + 1 : 0;
  x = r[2 * e]; y = r[2 * e + 1];
  on = nucfsd_edge((int64_t)r[2 * nx] - x, (int64_t)r[2 * nx + 1] - y, steps, diag, code);
}

// the kernel's way
static Row kernel_way(const Ring& r) {
  const int n = (int)(r.size() / 2);
  Row out{0, 0, 0, 0, std::vector<int>(NUCFSD_PER * NUCFSD_K, 0)};
  bool bad = false;
  int64_t A = 0, B = 0;
  for (int e = 0; e < n; ++e) {
    int x, y, code; int64_t steps; bool diag, on;
    edge_of(r, n, e, x, y, steps, diag, code, on);
    bad |= !on;
    (diag ? B : A) += steps;
  }
  out.status = bad ? NUCFSD_NOT_TRACED : A + B == 0 ? NUCFSD_DEGENERATE : A + B > NUCFSD_MAX_STEPS ? NUCFSD_TOO_LONG : NUCFSD_OK;
  if (out.status != NUCFSD_OK) return out;
  out.A = A; out.B = B; out.n = n;
  int carry_a = 0, carry_b = 0;
  std::vector<bool> placed(NUCFSD_K, false);
  for (int c0 = 0; c0 < n; c0 += NUCFSD_CHUNK) {
    const int m = n - c0 < NUCFSD_CHUNK ? n - c0 : NUCFSD_CHUNK;
    std::unique_ptr<int[]> ca(new int[m]), cb(new int[m]);               // exactly the chunk
    for (int t = 0; t < m; ++t) {
      int x, y, code; int64_t steps; bool diag, on;
      edge_of(r, n, c0 + t, x, y, steps, diag, code, on);
      ca[t] = carry_a; cb[t] = carry_b;
      (diag ? carry_b : carry_a) += (int)steps;
    }
    for (int k = 0; k < NUCFSD_K; ++k) {
      if (placed[k] || !(c0 + NUCFSD_CHUNK >= n || !nucfsd_at_or_before(carry_a, carry_b, k, A, B))) continue;
      const int j = nucfsd_search(ca.get(), cb.get(), m, k, A, B);
      int x, y, code; int64_t steps; bool diag, on;
      edge_of(r, n, c0 + j, x, y, steps, diag, code, on);
      int* s = &out.s[NUCFSD_PER * k];
      s[0] = x; s[1] = y; s[2] = code; s[3] = ca[j]; s[4] = cb[j];
      placed[k] = true;
    }
  }
  for (int k = 0; k < NUCFSD_K; ++k) if (!placed[k]) { std::printf("FAIL sample %d of a ring of %d vertices was not placed\n", k, n); std::exit(1); }
  return out;
}

// the definition: all edges, the comparison in __int128
static Row plain_way(const Ring& r) {
  const int n = (int)(r.size() / 2);
  Row out{0, 0, 0, 0, std::vector<int>(NUCFSD_PER * NUCFSD_K, 0)};
  std::vector<int64_t> a(n + 1, 0), b(n + 1, 0);
  std::vector<int> code(n, 0);
  bool bad = false;
  for (int e = 0; e < n; ++e) {
    const int nx = (e + 1) % n;
    const int64_t dx = (int64_t)r[2 * nx] - r[2 * e], dy = (int64_t)r[2 * nx + 1] - r[2 * e + 1], ax = std::llabs(dx), ay = std::llabs(dy);
    if (ax && ay && ax != ay) bad = true;
    a[e + 1] = a[e] + (ax && ay ? 0 : ax + ay); b[e + 1] = b[e] + (ax && ay ? ax : 0);
    for (int d = 0; d < 8; ++d) if ((dx > 0) - (dx < 0) == DX[d] && (dy > 0) - (dy < 0) == DY[d]) code[e] = d;
  }
  const int64_t A = a[n], B = b[n];
  out.status = bad ? NUCFSD_NOT_TRACED : A + B == 0 ? NUCFSD_DEGENERATE : A + B > NUCFSD_MAX_STEPS ? NUCFSD_TOO_LONG : NUCFSD_OK;
  if (out.status != NUCFSD_OK) return out;
  out.A = A; out.B = B; out.n = n;
  for (int k = 0; k < NUCFSD_K; ++k) {
    int best = -1;
    for (int e = 0; e < n; ++e) if (sign128(NUCFSD_K * a[e] - k * A, NUCFSD_K * b[e] - k * B) <= 0) best = e;
    int* s = &out.s[NUCFSD_PER * k];
    s[0] = r[2 * best]; s[1] = r[2 * best + 1]; s[2] = code[best]; s[3] = (int)a[best]; s[4] = (int)b[best];
  }
  return out;
}

static int check_ring(const Ring& r, const char* what, int want_status = -1) {
  const Row g = kernel_way(r), w = plain_way(r);
  if (g.status != w.status || g.A != w.A || g.B != w.B || g.n != w.n || g.s != w.s) {
    std::printf("FAIL %s (%zu vertices): status %d / %d, A %lld / %lld, B %lld / %lld\n", what, r.size() / 2, g.status, w.status, (long long)g.A,
                (long long)w.A, (long long)g.B, (long long)w.B);
    return 1;
  }
  if (want_status >= 0 && g.status != want_status) { std::printf("FAIL %s: status %d, expected %d\n", what, g.status, want_status); return 1; }
  return 0;
}

// a closed ring of about n vertices: a random walk along the chain directions and the same way back, some vertices repeated
static Ring walk(std::mt19937& rng, int n, int longest, int repeat_pct) {
  std::vector<int32_t> out_x{1000}, out_y{-500};
  const int half = n / 2 + 1;
  for (int i = 1; i < half; ++i) {
    const int d = (int)(rng() % 8), len = (int)(rng() % 100) < repeat_pct ? 0 : 1 + (int)(rng() % longest);
    out_x.push_back(out_x.back() + DX[d] * len); out_y.push_back(out_y.back() + DY[d] * len);
  }
  Ring r;
  for (int i = 0; i < half; ++i) { r.push_back(out_x[i]); r.push_back(out_y[i]); }
  for (int i = half - 2; i >= 1 && (int)(r.size() / 2) < n; --i) { r.push_back(out_x[i]); r.push_back(out_y[i]); }
  return r;
}

int main() {
  int bad = 0;
  // ---- limits
  struct { int64_t nv; int n; bool ok; } lim[] = {{1, 1, true}, {NUCFSD_MAX_VERTS, 4096, true}, {0, 1, false}, {-1, 1, false}, {NUCFSD_MAX_VERTS + 1, 1, false},
                                                  {1, 0, false}, {1, 4097, false}, {1, -1, false}};
  for (const auto& c : lim)
    if (nucfsd_args_ok(c.nv, c.n) != c.ok) { std::printf("FAIL limits nv %lld n %d\n", (long long)c.nv, c.n); ++bad; }
  // ---- the edge classifier: every small edge against the direction table, and the longest edges an int32 ring can hold
  for (int64_t dy = -6; dy <= 6; ++dy)
    for (int64_t dx = -6; dx <= 6; ++dx) {
      int64_t steps; bool diag; int code;
      const bool on = nucfsd_edge(dx, dy, steps, diag, code);
      const int64_t ax = std::llabs(dx), ay = std::llabs(dy);
      const bool want_on = !dx || !dy || ax == ay;
      int want_code = 0;
      for (int d = 0; d < 8; ++d) if ((dx > 0) - (dx < 0) == DX[d] && (dy > 0) - (dy < 0) == DY[d]) want_code = d;
      if (on != want_on || steps != (ax > ay ? ax : ay) || diag != (ax && ay) || code != want_code) { std::printf("FAIL edge %lld %lld\n", (long long)dx, (long long)dy); ++bad; }
    }
  {
    int64_t steps; bool diag; int code;
    const int64_t big = 4294967295ll;
    if (!nucfsd_edge(-big, big, steps, diag, code) || steps != big || !diag || code != 5) { std::printf("FAIL longest diagonal\n"); ++bad; }
    if (!nucfsd_edge(0, -big, steps, diag, code) || steps != big || diag || code != 2) { std::printf("FAIL longest axial\n"); ++bad; }
    if (nucfsd_edge(big, big - 1, steps, diag, code)) { std::printf("FAIL longest off-chain\n"); ++bad; }
  }
  // ---- the sign: Pell convergents and their neighbours, then random pairs, all within the limit
  const int64_t LIM = (int64_t)NUCFSD_K * (NUCFSD_MAX_STEPS - 1);
  long long checked = 0;
  auto one = [&](int64_t p, int64_t q) {
    if (std::llabs(p) > LIM || std::llabs(q) > LIM) return;
    ++checked;
    if (nucfsd_sign(p, q) != sign128(p, q)) { std::printf("FAIL sign of %lld + %lld sqrt 2\n", (long long)p, (long long)q); ++bad; }
  };
  for (int64_t p = 1, q = 1; p <= LIM; ) {
    for (int64_t dp = -2; dp <= 2; ++dp)
      for (int64_t dq = -2; dq <= 2; ++dq)
        for (int sp : {-1, 1})
          for (int sq : {-1, 1}) one(sp * (p + dp), sq * (q + dq));
    const int64_t np = p + 2 * q, nq = p + q;
    p = np; q = nq;
  }
  for (int64_t v : {(int64_t)0, (int64_t)1, LIM - 1, LIM})
    for (int64_t w : {(int64_t)0, (int64_t)1, LIM - 1, LIM})
      for (int sp : {-1, 1})
        for (int sq : {-1, 1}) one(sp * v, sq * w);
  std::mt19937_64 r64(11);
  for (int it = 0; it < 400000; ++it) {
    const int shift = (int)(r64() % 32);
    const int64_t q = ((int64_t)(r64() % (uint64_t)(2 * LIM + 1)) - LIM) >> shift;
    // p near -q sqrt 2, where the decision is closest, and anywhere
    const int64_t near = (int64_t)(-(long double)q * 1.41421356237309504880L) + (int64_t)(r64() % 5) - 2;
    one(near, q);
    one(((int64_t)(r64() % (uint64_t)(2 * LIM + 1)) - LIM) >> shift, q);
  }
  if (checked < 500000) { std::printf("FAIL only %lld signs were checked\n", checked); ++bad; }
  // ---- rings: designed ones with their status, then walks round the chunk boundaries
  bad += check_ring(Ring{}, "no vertex", NUCFSD_DEGENERATE);
  bad += check_ring(Ring{5, 7}, "one vertex", NUCFSD_DEGENERATE);
  bad += check_ring(Ring{5, 7, 5, 7, 5, 7}, "one point three times", NUCFSD_DEGENERATE);
  bad += check_ring(Ring{0, 0, 9, 0}, "out and back, axial", NUCFSD_OK);
  bad += check_ring(Ring{0, 0, -9, 9}, "out and back, diagonal", NUCFSD_OK);
  bad += check_ring(Ring{0, 0, 32, 0, 32, 32, 0, 32}, "square of perimeter 128", NUCFSD_OK);
  bad += check_ring(Ring{0, 0, 64, 0, 64, 64, 0, 64}, "square of perimeter 256", NUCFSD_OK);
  bad += check_ring(Ring{0, 0, 7, 7, 14, 0, 7, -7}, "diamond", NUCFSD_OK);
  bad += check_ring(Ring{0, 0, 3, 1, 3, 3, 0, 3}, "off the chain", NUCFSD_NOT_TRACED);
  bad += check_ring(Ring{0, 0, 8388608, 0, 8388608, 1, 0, 1}, "2^24 + 2 steps", NUCFSD_TOO_LONG);
  bad += check_ring(Ring{0, 0, 8388607, 0, 8388607, 1, 0, 1}, "2^24 steps", NUCFSD_OK);
  bad += check_ring(Ring{0, 0, 8388608, 8388608}, "2^24 diagonal steps", NUCFSD_OK);
  bad += check_ring(Ring{-1073741823, -1073741823, 1073741823, 1073741823}, "the longest diagonal", NUCFSD_TOO_LONG);
  std::mt19937 rng(5);
  for (int n : {2, 3, 63, 64, 65, 255, 256, 257, 258, 511, 512, 513, 767, 768, 769, 1025, 3001})
    for (int longest : {1, 3, 40})
      for (int repeat_pct : {0, 30, 90}) bad += check_ring(walk(rng, n, longest, repeat_pct), "walk");
  if (bad) std::printf("%d FAILED\n", bad); else std::printf("nucfsd host check ok (%lld signs)\n", checked);
  return bad ? 1 : 0;
}
