// Host check of the plain-C++ parts of the per-slide point kernels (nuhtc_amd/csrc/cellgrid_host.h: the grid geometry, the (cell, class)
// key, the pair distance within reach, the front checks of the entry points; cellspatial_host.h: the bin lookup, the LDS carve and the
// rotated column of the row sums, the check of the bin edges), meant to be built with a sanitizer and run on the host -- it never touches a GPU, and the kernel code itself (cellspatial.hip, cellbin.h) is NOT sanitized:
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I nuhtc_amd/csrc tools/dev/cellspatial_host_check.cpp -o /tmp/cellspatial_host_check && /tmp/cellspatial_host_check
//
// Small point sets are taken the way the kernels take them: the grid from cell_grid_side, a counting sort on cell_key into a start table
// of exactly keys + 1 entries, then for every record, class by class, the runs of its 3 x 3 cells, the bin from cs_bin_of, the private
// counter at cs_priv_at inside a heap block of exactly cs_lds_bytes(C, B) bytes carved by the cs_lds_*_off functions, the row sums over
// cs_rotated_column into the table at cs_table_at, every pair through cell_pair_d2 -- so an index past a table, a run or the carve is reported -- and compared with plain
// counts over all pairs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "cellspatial_host.h"

struct Result { std::vector<long long> hist; std::vector<int> nn; std::vector<long long> cn; };

// the front of nuhtc_cell_spatial: the edges, then the shared limits with e_B as the reach (no points: no box)
static bool cs_args_ok(int64_t n, int C, const int* edges, int B, int e2[CS_MAX_BINS]) {
  return cs_edges_ok(edges, B, e2) && cell_call_ok(n, CELL_MAX_POINTS, C, edges[B - 1], 0, 0, 0, 0);
}

static Result plain_way(const std::vector<int>& p, const std::vector<int>& lab, int C, const std::vector<int>& e) {
  const int n = (int)lab.size(), B = (int)e.size();
  Result r{std::vector<long long>(C * C * B, 0), std::vector<int>((size_t)n * C, -1), std::vector<long long>(C, 0)};
  for (int i = 0; i < n; ++i) {
    if (lab[i] >= 0 && lab[i] < C) r.cn[lab[i]]++;
    for (int j = 0; j < n; ++j) {
      if (i == j) continue;
      const long long dx = (long long)p[2 * j] - p[2 * i], dy = (long long)p[2 * j + 1] - p[2 * i + 1], d2 = dx * dx + dy * dy;
      if (d2 > (long long)e[B - 1] * e[B - 1]) continue;
      int t = 0;
      while (d2 > (long long)e[t] * e[t]) ++t;
      if (lab[j] < 0 || lab[j] >= C) continue;
      int& best = r.nn[(size_t)i * C + lab[j]];
      if (best < 0 || d2 < best) best = (int)d2;
      if (lab[i] >= 0 && lab[i] < C) r.hist[(lab[i] * C + lab[j]) * B + t]++;
    }
  }
  return r;
}

static Result kernel_way(const std::vector<int>& p, const std::vector<int>& lab, int C, const std::vector<int>& e, int max_cells) {
  const int n = (int)lab.size(), B = (int)e.size(), sub = C + 1;
  int e2[CS_MAX_BINS];
  if (!cs_args_ok(n, C, e.data(), B, e2)) { std::printf("FAIL arguments refused\n"); std::exit(1); }
  Result r{std::vector<long long>(C * C * B, 0), std::vector<int>((size_t)n * C, -1), std::vector<long long>(C, 0)};
  if (!n) return r;
  int x_min = p[0], x_max = p[0], y_min = p[1], y_max = p[1];
  for (int i = 0; i < n; ++i) {
    x_min = std::min(x_min, p[2 * i]); x_max = std::max(x_max, p[2 * i]); y_min = std::min(y_min, p[2 * i + 1]); y_max = std::max(y_max, p[2 * i + 1]);
  }
  if (!cell_box_ok(x_min, y_min, x_max, y_max)) { std::printf("FAIL box refused\n"); std::exit(1); }
  const int reach = e[B - 1], side = cell_grid_side(x_min, y_min, x_max, y_max, reach, max_cells);
  const int ncx = (int)cell_cells_along(x_min, x_max, side), ncy = (int)cell_cells_along(y_min, y_max, side);
  if (side % reach || (long long)ncx * ncy > max_cells) { std::printf("FAIL grid side %d of reach %d: %d x %d cells\n", side, reach, ncx, ncy); std::exit(1); }
  const int nkey = ncx * ncy * sub;
  std::unique_ptr<int[]> start(new int[nkey + 1]), fill(new int[nkey]);               // exactly the keys and the total behind them
  std::memset(start.get(), 0, sizeof(int) * (nkey + 1)); std::memset(fill.get(), 0, sizeof(int) * nkey);
  auto key_of = [&](int i) { return cell_key(cell_index(p[2 * i], p[2 * i + 1], x_min, y_min, side, ncx), lab[i], sub); };
  for (int i = 0; i < n; ++i) start[key_of(i) + 1]++;
  for (int k = 0; k < nkey; ++k) start[k + 1] += start[k];
  std::unique_ptr<int[]> recs(new int[4 * (size_t)n]);
  for (int i = 0; i < n; ++i) {
    const int k = key_of(i), pos = start[k] + fill[k]++;
    recs[4 * pos] = p[2 * i]; recs[4 * pos + 1] = p[2 * i + 1]; recs[4 * pos + 2] = lab[i]; recs[4 * pos + 3] = i;
  }
  // one workgroup's LDS, exactly as large as the launch asks for
  const int bytes = cs_lds_bytes(C, B);
  std::unique_ptr<unsigned char[]> lds(new unsigned char[bytes]);
  unsigned long long* table = reinterpret_cast<unsigned long long*>(lds.get());
  unsigned* priv = reinterpret_cast<unsigned*>(lds.get() + cs_lds_priv_off(C, B));
  int* e2l = reinterpret_cast<int*>(lds.get() + cs_lds_e2_off(C, B));
  int* cls = reinterpret_cast<int*>(lds.get() + cs_lds_cls_off(C, B));
  unsigned* cn = reinterpret_cast<unsigned*>(lds.get() + cs_lds_cn_off(C, B));
  for (int i = 0; i < C * C * B; ++i) table[i] = 0;
  for (int t = 0; t < CS_MAX_BINS; ++t) e2l[t] = e2[t];
  for (int c = 0; c < 16; ++c) cn[c] = 0;
  const int reach2 = reach * reach;
  for (int blk = 0; blk * CS_NT < n; ++blk) {
    for (int tid = 0; tid < CS_NT; ++tid) {
      const int q = blk * CS_NT + tid;
      cls[tid] = q < n ? cs_class(recs[4 * q + 2], C) : C;
      if (cls[tid] < C) cn[cls[tid]]++;
    }
    for (int b = 0; b < C; ++b) {
      for (int tid = 0; tid < CS_NT; ++tid) {
        for (int t = 0; t < B; ++t) priv[cs_priv_at(t, tid)] = 0;
        const int q = blk * CS_NT + tid;
        if (q >= n) continue;
        const int mx = recs[4 * q], my = recs[4 * q + 1], mi = recs[4 * q + 3];
        const int cx = (mx - x_min) / side, cy = (my - y_min) / side;
        int best = CS_NO_EDGE;
        for (int gy = std::max(cy - 1, 0); gy <= std::min(cy + 1, ncy - 1); ++gy)
          for (int gx = std::max(cx - 1, 0); gx <= std::min(cx + 1, ncx - 1); ++gx) {
            const int key = cell_key(gy * ncx + gx, b, sub);
            for (int j = start[key]; j < start[key + 1]; ++j) {
              const int dd = cell_pair_d2(recs[4 * j] - mx, recs[4 * j + 1] - my, reach, reach2);
              if (dd < 0 || recs[4 * j + 3] == mi) continue;
              best = std::min(best, dd);
              priv[cs_priv_at(cs_bin_of(e2l, dd), tid)] += 1;
            }
          }
        r.nn[(size_t)mi * C + b] = best == CS_NO_EDGE ? -1 : best;
      }
      for (int wbase = 0; wbase < CS_NT; wbase += 64)
        for (int lane = 0; lane < B; ++lane) {
          int cur = C;
          unsigned long long acc = 0;
          bool seen[64] = {};
          for (int jj = 0; jj < 64; ++jj) {
            const int c64 = cs_rotated_column(jj, lane), col = wbase + c64;
            if (seen[c64]) { std::printf("FAIL the rotated column repeats\n"); std::exit(1); }
            seen[c64] = true;
            if (cls[col] != cur) {
              if (acc && cur < C) table[cs_table_at(cur, b, lane, C, B)] += acc;
              cur = cls[col]; acc = 0;
            }
            acc += priv[cs_priv_at(lane, col)];
          }
          if (acc && cur < C) table[cs_table_at(cur, b, lane, C, B)] += acc;
        }
    }
  }
  for (int i = 0; i < C * C * B; ++i) r.hist[i] = (long long)table[i];
  for (int c = 0; c < C; ++c) r.cn[c] = cn[c];
  return r;
}

static int check(const std::vector<int>& p, const std::vector<int>& lab, int C, const std::vector<int>& e, int max_cells, const char* what) {
  const Result g = kernel_way(p, lab, C, e, max_cells), w = plain_way(p, lab, C, e);
  if (g.hist != w.hist || g.nn != w.nn || g.cn != w.cn) { std::printf("FAIL %s (%zu points, C %d, B %zu)\n", what, lab.size(), C, e.size()); return 1; }
  return 0;
}

int main() {
  int bad = 0;
  // ---- limits
  {
    int e2[CS_MAX_BINS];
    std::vector<int> e33(33);
    for (int t = 0; t < 33; ++t) e33[t] = t + 1;
    const int inc[] = {3, 5, 9}, flat[] = {3, 3}, zero[] = {0, 4}, big[] = {7, 16385}, top[] = {16384};
    struct { int64_t n; int C; const int* e; int B; bool ok; } lim[] = {
        {0, 1, inc, 3, true}, {CELL_MAX_POINTS, 14, e33.data(), 32, true}, {CELL_MAX_POINTS + 1, 3, inc, 3, false}, {-1, 3, inc, 3, false},
        {5, 0, inc, 3, false}, {5, 15, inc, 3, false}, {5, 3, inc, 0, false}, {5, 3, e33.data(), 33, false}, {5, 3, flat, 2, false},
        {5, 3, zero, 2, false}, {5, 3, big, 2, false}, {5, 3, top, 1, true}, {5, 3, nullptr, 1, false}};
    for (const auto& c : lim)
      if (cs_args_ok(c.n, c.C, c.e, c.B, e2) != c.ok) { std::printf("FAIL limits n %lld C %d B %d\n", (long long)c.n, c.C, c.B); ++bad; }
    if (!cs_args_ok(1, 1, top, 1, e2) || e2[0] != 16384 * 16384 || e2[1] != CS_NO_EDGE || e2[31] != CS_NO_EDGE) { std::printf("FAIL squared edges\n"); ++bad; }
    const int L = CELL_COORD_LIMIT;
    if (!cell_box_ok(-L + 1, -L + 1, L - 1, L - 1) || cell_box_ok(-L, 0, 0, 0) || cell_box_ok(0, 0, L, 0) || cell_box_ok(0, 0, 0, L) || cell_box_ok(0, -L, 0, 0) ||
        cell_box_ok(1, 0, 0, 0) || cell_box_ok(0, 1, 0, 0)) { std::printf("FAIL box limits\n"); ++bad; }
  }
  // ---- the pair distance at the limits, against 64-bit arithmetic: differences up to 2^28 - 1, the reach at both ends of its range
  for (int reach : {1, CELL_MAX_REACH}) {
    const int big = (1 << 28) - 1, at[] = {0, 1, reach - 1, reach, reach + 1, big};
    for (int ax : at) for (int ay : at) for (int sx : {-1, 1}) for (int sy : {-1, 1}) {
      const int dx = sx * ax, dy = sy * ay;
      const long long d2 = (long long)dx * dx + (long long)dy * dy, want = d2 <= (long long)reach * reach ? d2 : -1;
      if (cell_pair_d2(dx, dy, reach, reach * reach) != want) { std::printf("FAIL pair d2 dx %d dy %d reach %d\n", dx, dy, reach); ++bad; }
    }
  }
  // ---- the front checks the entry points share
  {
    const int L = CELL_COORD_LIMIT;
    struct { int64_t n, max_n; int C, reach, x0, y0, x1, y1; bool ok; } call[] = {
        {0, 1 << 24, 1, 1, 5, 5, 0, 0, true}, {1, 1 << 24, 14, 16384, -L + 1, -L + 1, L - 1, L - 1, true}, {1, 1 << 24, 1, 1, 5, 5, 0, 0, false},
        {(1 << 24) + 1, 1 << 24, 1, 1, 0, 0, 0, 0, false}, {-1, 1 << 24, 1, 1, 0, 0, 0, 0, false}, {1, 1, 0, 1, 0, 0, 0, 0, false},
        {1, 1, 15, 1, 0, 0, 0, 0, false}, {1, 1, 1, 0, 0, 0, 0, 0, false}, {1, 1, 1, 16385, 0, 0, 0, 0, false}, {1, 1, 1, 1, -L, 0, 0, 0, false}};
    for (const auto& c : call)
      if (cell_call_ok(c.n, c.max_n, c.C, c.reach, c.x0, c.y0, c.x1, c.y1) != c.ok) { std::printf("FAIL call limits n %lld C %d reach %d\n", (long long)c.n, c.C, c.reach); ++bad; }
  }
  // ---- the LDS carve: aligned, in order, nothing overlaps, the last index of every part inside the block, within a CU's 160 KiB
  for (int C = 1; C <= CS_MAX_CLASSES; ++C)
    for (int B = 1; B <= CS_MAX_BINS; ++B) {
      const int po = cs_lds_priv_off(C, B), eo = cs_lds_e2_off(C, B), co = cs_lds_cls_off(C, B), no = cs_lds_cn_off(C, B), end = cs_lds_bytes(C, B);
      const bool ok = po % 16 == 0 && eo % 16 == 0 && co % 16 == 0 && no % 16 == 0 && 8 * (cs_table_at(C - 1, C - 1, B - 1, C, B) + 1) <= po &&
                      po + 4 * (cs_priv_at(B - 1, CS_NT - 1) + 1) <= eo && eo + 4 * 32 <= co && co + 4 * CS_NT <= no && no + 4 * 16 <= end && end <= 160 * 1024;
      if (!ok) { std::printf("FAIL LDS carve C %d B %d\n", C, B); ++bad; }
    }
  // ---- the grid at the extremes of the box: the cap holds, the side is a multiple of the reach, the bisection is the smallest multiple
  for (int reach : {1, 7, 512, 16384})
    for (int cap : {1, 2, 1000, CS_MAX_CELLS, 1 << 22}) {
      const int L = CELL_COORD_LIMIT - 1;
      for (int span : {0, 1, reach, 12345, L, 2 * L}) {
        const int side = cell_grid_side(-L, -L, -L + span, -L + span / 2, reach, cap);
        const long long cells = cell_cells_along(-L, -L + span, side) * cell_cells_along(-L, -L + span / 2, side);
        const bool smaller_fits = side > reach && cell_cells_along(-L, -L + span, side - reach) * cell_cells_along(-L, -L + span / 2, side - reach) <= cap;
        if (side < reach || side % reach || cells > cap || smaller_fits) { std::printf("FAIL grid reach %d cap %d span %d\n", reach, cap, span); ++bad; }
      }
    }
  // ---- the bin lookup against the definition, on every edge, one below and one above
  std::mt19937 rng(3);
  for (int B = 1; B <= CS_MAX_BINS; ++B)
    for (int rep = 0; rep < 20; ++rep) {
      std::vector<int> e(B);
      int v = 0;
      for (int t = 0; t < B; ++t) { v += 1 + (int)(rng() % (rep < 10 ? 3 : 500)); e[t] = v; }
      if (rep == 0) e[B - 1] = CS_MAX_EDGE;
      int e2[CS_MAX_BINS];
      if (!cs_args_ok(1, 1, e.data(), B, e2)) { std::printf("FAIL edges refused\n"); ++bad; continue; }
      auto one = [&](int d2) {
        if (d2 < 0 || d2 > e2[B - 1]) return;
        int t = 0;
        while (d2 > e2[t]) ++t;
        if (cs_bin_of(e2, d2) != t) { std::printf("FAIL bin of %d with %d edges\n", d2, B); ++bad; }
      };
      for (int t = 0; t < B; ++t) { one(e2[t] - 1); one(e2[t]); one(e2[t] + 1); }
      one(0);
      for (int k = 0; k < 200; ++k) one((int)(rng() % (unsigned)(e2[B - 1] + 1)));
    }
  // ---- point sets: the kernel's way against all pairs
  {
    std::vector<int> p, lab;                                        // the 12 x 12 lattice of the tests, edges on and beside lattice distances
    for (int y = 0; y < 12; ++y) for (int x = 0; x < 12; ++x) { p.push_back(x * 12 + 40); p.push_back(y * 12 + 24); lab.push_back((y * 12 + x) % 4); }
    bad += check(p, lab, 4, {12, 17, 24, 34}, CS_MAX_CELLS, "lattice");
    bad += check(p, lab, 4, {12, 17, 24, 34}, 4, "lattice, four cells");
    bad += check(p, lab, 3, {12}, CS_MAX_CELLS, "lattice, a label out of range");
  }
  {
    std::vector<int> p, lab;                                        // more coincident points than a workgroup has threads
    for (int i = 0; i < 300; ++i) { p.push_back(5000); p.push_back(5000); lab.push_back(i % 3 == 2 ? -1 : i % 3); }
    for (int k = 0; k < 5; ++k) { p.push_back(5000 + 3 * k); p.push_back(4990 + 5 * k); lab.push_back(k % 2); }
    bad += check(p, lab, 2, {1, 4, 16}, CS_MAX_CELLS, "coincident");
  }
  for (int rep = 0; rep < 40; ++rep) {
    const int n = 1 + (int)(rng() % 700), C = 1 + (int)(rng() % CS_MAX_CLASSES), B = 1 + (int)(rng() % CS_MAX_BINS);
    const int extent = rep % 4 == 0 ? 60 : rep % 4 == 1 ? 900 : 6000, far = rep % 5 == 0 ? (1 << 22) : 0;
    const int ox = rep % 3 == 0 ? -(CELL_COORD_LIMIT - 1) : rep % 3 == 1 ? 300000 : CELL_COORD_LIMIT - 1 - extent - far;
    std::vector<int> e(B), p, lab;
    int v = 0;
    for (int t = 0; t < B; ++t) { v += 1 + (int)(rng() % 12); e[t] = v; }
    for (int i = 0; i < n; ++i) {
      const int shift = far && i % 2 ? far : 0;
      p.push_back(ox + shift + (int)(rng() % (unsigned)(extent + 1))); p.push_back(ox + shift + (int)(rng() % (unsigned)(extent + 1)));
      lab.push_back((int)(rng() % (unsigned)(C + 2)) - 1);         // -1 and C among them
    }
    bad += check(p, lab, C, e, rep % 2 ? CS_MAX_CELLS : 50, "random");
  }
  if (bad) std::printf("%d FAILED\n", bad); else std::printf("cellspatial host check ok\n");
  return bad ? 1 : 0;
}
