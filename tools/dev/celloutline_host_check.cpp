// Host check of the plain-C++ parts of the alpha-shape outline (nuhtc_amd/csrc/cellgrid_host.h: outline_turn_class, outline_turn_before,
// outline_better, outline_side, outline_rounds, outline_call_ok), meant to be built with a sanitizer and run on the host -- it never
// touches a GPU, and the kernel code itself (celloutline.hip) is NOT sanitized:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I nuhtc_amd/csrc tools/dev/celloutline_host_check.cpp \
//       -o /tmp/celloutline_host_check && /tmp/celloutline_host_check
//
// Three parts.  The angular predicate over direction pairs up to length 1024 -- every pair of a sample of directions, among them the
// axes, the diagonals, the longest vectors and neighbours that differ by one half pixel at full length -- against a comparison that uses
// no cross product of the two candidates: each candidate is turned into the frame of a (x' = a . b, y' = a x b, 128 bits), placed in a
// quadrant of the clockwise turn, and two candidates of one quadrant are compared by their exact rational slopes.  The successor choice:
// outline_better folded over the out-half-edges of a vertex in several orders against the smallest candidate of that comparison.  And
// the extremes of the bit budget: vectors between the corners of the coordinate range (|v| < 2^28, products at 2^56), where UBSan would
// report a signed overflow.
#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

#include "cellgrid_host.h"

typedef __int128 wide;
struct Vec { int64_t x, y; };

// the clockwise turn from a to b as (quadrant 0..3, slope num / den within the quadrant), from the frame of a: x' = a . b, y' = -(a x b)
// (y' > 0: clockwise of a).  Quadrant 0: x' > 0, y' >= 0 (angle in [0, pi/2)); 1: x' <= 0, y' > 0; 2: x' < 0, y' <= 0; 3: x' >= 0, y' < 0.
// Within a quadrant the angle grows with the slope (the leg left behind over the leg ahead).
struct Turn { int quad; wide num, den; };
static Turn turn_of(Vec a, Vec b) {
  const wide x = (wide)a.x * b.x + (wide)a.y * b.y, y = -((wide)a.x * b.y - (wide)a.y * b.x);
  if (x > 0 && y >= 0) return Turn{0, y, x};
  if (x <= 0 && y > 0) return Turn{1, -x, y};
  if (x < 0 && y <= 0) return Turn{2, -y, -x};
  return Turn{3, x, -y};
}
// is the turn to b1 strictly smaller than the turn to b2?  (slopes compared as rationals with positive denominators)
static bool turn_less(Vec a, Vec b1, Vec b2) {
  const Turn s = turn_of(a, b1), t = turn_of(a, b2);
  if (s.quad != t.quad) return s.quad < t.quad;
  return s.num * t.den < t.num * s.den;
}

static int fails = 0;
static void expect(bool ok, const char* what, Vec a, Vec b1, Vec b2) {
  if (ok) return;
  if (++fails <= 10) std::printf("FAIL %s: a (%lld, %lld) b1 (%lld, %lld) b2 (%lld, %lld)\n", what, (long long)a.x, (long long)a.y, (long long)b1.x, (long long)b1.y, (long long)b2.x, (long long)b2.y);
}

static void check_triple(Vec a, Vec b1, Vec b2) {
  expect(outline_turn_before(a.x, a.y, b1.x, b1.y, b2.x, b2.y) == turn_less(a, b1, b2), "turn_before", a, b1, b2);
  const bool same = !turn_less(a, b1, b2) && !turn_less(a, b2, b1);
  expect(outline_better(a.x, a.y, b1.x, b1.y, 5, b2.x, b2.y, 9) == (turn_less(a, b1, b2) || same), "better, smaller id", a, b1, b2);
  expect(outline_better(a.x, a.y, b1.x, b1.y, 9, b2.x, b2.y, 5) == turn_less(a, b1, b2), "better, larger id", a, b1, b2);
}

// the successor choice at one vertex: the fold, in the given order and reversed and shuffled, against the minimum of turn_less
static void check_fan(Vec a, std::vector<Vec> out, std::mt19937& rng) {
  std::vector<int> id(out.size());
  for (size_t k = 0; k < id.size(); ++k) id[k] = (int)k;
  int want = 0;
  for (size_t k = 1; k < out.size(); ++k)
    if (turn_less(a, out[k], out[want])) want = (int)k;
  for (int pass = 0; pass < 3; ++pass) {
    if (pass == 1) std::reverse(id.begin(), id.end());
    if (pass == 2) std::shuffle(id.begin(), id.end(), rng);
    int best = -1;
    Vec bb{0, 0};
    for (int k : id)
      if (outline_better(a.x, a.y, out[k].x, out[k].y, k, bb.x, bb.y, best)) { best = k; bb = out[k]; }
    expect(best == want, "fold", a, out[want], out[best < 0 ? 0 : best]);
  }
}

int main() {
  std::mt19937 rng(2026);
  // ---- 1: directions up to length 1024
  std::vector<Vec> dirs = {{1, 0}, {0, 1}, {-1, 0}, {0, -1}, {1, 1}, {-1, 1}, {-1, -1}, {1, -1}, {1024, 0}, {0, 1024}, {-1024, 0}, {0, -1024},
                           {724, 724}, {-724, 724}, {724, -724}, {-724, -724}, {1023, 1}, {1023, -1}, {1, 1023}, {-1, 1023}, {1024, 1}, {1023, 2},
                           {-1023, 1}, {-1023, -1}, {1, -1023}, {-1, -1023}, {3, 4}, {6, 8}, {-3, -4}, {4, -3}, {-4, 3}, {600, 800}, {-600, -800}, {800, -600}};
  std::uniform_int_distribution<int> coord(-1024, 1024);
  while (dirs.size() < 150) {
    const Vec v{coord(rng), coord(rng)};
    if ((v.x || v.y) && v.x * v.x + v.y * v.y <= 1024 * 1024) dirs.push_back(v);
  }
  long long triples = 0;
  for (const Vec& a : dirs)
    for (const Vec& b1 : dirs)
      for (const Vec& b2 : dirs) { check_triple(a, b1, b2); ++triples; }
  // the four classes by name
  if (outline_turn_class(1, 0, 2, 0) != 0 || outline_turn_class(1, 0, 1, -1) != 1 || outline_turn_class(1, 0, -3, 0) != 2 || outline_turn_class(1, 0, 1, 1) != 3) { ++fails; std::printf("FAIL turn_class\n"); }
  // ---- 2: the successor choice on fans of distinct directions
  long long fans = 0;
  for (int rep = 0; rep < 20000; ++rep) {
    const Vec a = dirs[rng() % dirs.size()];
    std::vector<Vec> out;
    const int k = 1 + (int)(rng() % 6);
    while ((int)out.size() < k) {
      const Vec b = dirs[rng() % dirs.size()];
      bool fresh = (wide)a.x * b.y - (wide)a.y * b.x != 0 || (wide)a.x * b.x + (wide)a.y * b.y < 0;       // not the direction of a
      for (const Vec& o : out) fresh = fresh && !((wide)o.x * b.y - (wide)o.y * b.x == 0 && (wide)o.x * b.x + (wide)o.y * b.y > 0);
      if (fresh) out.push_back(b);
    }
    check_fan(a, out, rng);
    ++fans;
  }
  // ---- 3: the extremes of the bit budget: differences of points with |p| < 2^27
  const int64_t L = ((int64_t)1 << 28) - 2;
  const std::vector<Vec> far = {{L, L}, {-L, L}, {L, -L}, {-L, -L}, {L, 0}, {0, L}, {-L, 0}, {0, -L}, {L, L - 1}, {L - 1, L}, {-L, -L + 1}, {L, -L + 1}, {1, 0}, {-1, L}};
  for (const Vec& a : far)
    for (const Vec& b1 : far)
      for (const Vec& b2 : far) { check_triple(a, b1, b2); ++triples; }
  if (!(outline_side(L, 0, 0, L) > 0 && outline_side(L, 0, 0, -L) < 0 && outline_side(L, L, L, L) == 0)) { ++fails; std::printf("FAIL side\n"); }
  // ---- the small functions
  const bool small = outline_rounds(0) == 0 && outline_rounds(1) == 0 && outline_rounds(2) == 1 && outline_rounds(3) == 2 && outline_rounds(16384) == 14 &&
                     outline_rounds(16385) == 15 && outline_rounds(20000) == 15 && outline_rounds((int64_t)1 << 24) == 24 && outline_call_ok(0, 0, 0) &&
                     outline_call_ok((int64_t)1 << 24, (int64_t)1 << 24, 1) && !outline_call_ok(-1, 0, 0) && !outline_call_ok(0, -1, 0) &&
                     !outline_call_ok(((int64_t)1 << 24) + 1, 0, 0) && !outline_call_ok(0, ((int64_t)1 << 24) + 1, 0) && !outline_call_ok(3, 3, 2) &&
                     outline_coord_ok((1 << 27) - 1, -(1 << 27) + 1) && !outline_coord_ok(1 << 27, 0) && !outline_coord_ok(0, -(1 << 27));
  if (!small) { ++fails; std::printf("FAIL rounds / call_ok / coord_ok\n"); }
  std::printf("celloutline_host_check: %lld triples, %lld fans, %d failures\n", triples, fans, fails);
  return fails ? 1 : 0;
}
