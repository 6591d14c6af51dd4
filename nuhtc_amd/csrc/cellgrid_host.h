// The uniform grid over half-pixel points that the per-slide analyses share (cellbin.h; cellgraph.hip, cellspatial.hip, cellcluster.hip,
// cellmst.hip, cellprox.hip, celldensity.hip, cellterritory.hip, celladjacency.hip, cellalpha.hip, celloutline.hip, cellregion.hip, cellmargin.hip, cellenrich.hip; celledgelist.h, the frame of the edge-list analyses; cellsites.h, the lattice and the sweep of the site rasters): the parts that are plain C++ and run on the host as well -- the limits, the grid geometry over the bounding box, the cell
// and the (cell, class) key of a point, the squared distance of a pair within reach, the rank of an edge in its row's segment, and the edge key of the spanning forest.  Header-only,
// so a host program can exercise them under a sanitizer (tools/dev/cellspatial_host_check.cpp, tools/dev/cellmst_host_check.cpp, tools/dev/cellprox_host_check.cpp,
// tools/dev/celldensity_host_check.cpp, tools/dev/cellregion_host_check.cpp, tools/dev/cellmargin_host_check.cpp, tools/dev/cellenrich_host_check.cpp, tools/dev/cellterritory_host_check.cpp, tools/dev/celladjacency_host_check.cpp, tools/dev/cellalpha_host_check.cpp, tools/dev/celloutline_host_check.cpp); the kernels call the same functions.  nuhtc_amd/cellpoints.py states the same limits.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define CELL_HD __host__ __device__
#else
#define CELL_HD
#endif

constexpr int CELL_COORD_LIMIT = 1 << 27;              // |p| < 2^27 half pixels
constexpr int64_t CELL_MAX_POINTS = (int64_t)1 << 28;
constexpr int CELL_MAX_REACH = 16384;                  // half pixels: the largest radius or bin edge
constexpr int CELL_MAX_CLASSES = 14;

// ---- grid geometry over the inclusive bounding box
CELL_HD inline long long cell_cells_along(int lo, int hi, long long side) { return ((long long)hi - lo) / side + 1; }

// the cell side: the smallest multiple m * r of the reach r whose grid over the box has at most max_cells cells, so side >= r and the
// 3 x 3 cells around a point hold its whole disc.  The cell count does not grow with m: bisection; at hi the grid is one cell.
inline int cell_grid_side(int x_min, int y_min, int x_max, int y_max, int r, int max_cells) {
  long long lo = 1, hi = (1LL << 29) / r + 1;
  while (lo < hi) {
    const long long m = (lo + hi) / 2;
    if (cell_cells_along(x_min, x_max, m * r) * cell_cells_along(y_min, y_max, m * r) <= max_cells) hi = m; else lo = m + 1;
  }
  return (int)(lo * r);
}

// the cell of a point INSIDE the box (the caller has compared it with the box)
CELL_HD inline int cell_index(int x, int y, int x_min, int y_min, int side, int ncx) { return ((y - y_min) / side) * ncx + (x - x_min) / side; }

// ---- the class of a label among C classes: itself, or C for a label outside 0 .. C - 1 (counted in no row and no column)
CELL_HD inline int cs_class(int label, int C) { return (unsigned)label < (unsigned)C ? label : C; }

// the counting-sort key: `sub` keys per cell.  sub == 1: the cell alone; sub == C + 1: (cell, class)
CELL_HD inline int cell_key(int cell, int label, int sub) { return sub == 1 ? cell : cell * sub + cs_class(label, sub - 1); }

// ---- the squared distance of a pair, dx = x_j - x_i and dy = y_j - y_i, or -1 when the pair is out of reach (reach2 = reach * reach;
// the reach is inclusive).  Why nothing overflows, stated here once: |p| < 2^27 makes |dx|, |dy| < 2^28, so the differences are exact
// int32; the box test against the reach comes BEFORE the products, so they are taken only of |dx|, |dy| <= reach <= 16384 = 2^14, and
// d2 <= 2 * 2^28 = 2^29 < 2^31.
CELL_HD inline int cell_pair_d2(int dx, int dy, int reach, int reach2) {
  if (dx > reach || dx < -reach || dy > reach || dy < -reach) return -1;
  const int d2 = dx * dx + dy * dy;
  return d2 > reach2 ? -1 : d2;
}

// ---- the place of an edge in the segment of its smaller row, for the analyses that return an edge list in ascending (i, j) order
// (cellprox.hip, cellalpha.hip, celladjacency.hip, cellmst.hip: their place kernels, one thread per edge).  s_hi[j0 .. j1) holds the
// larger row of every edge of the segment in ARRIVAL order (the order inside a cell or a hash table is atomic arrival order and must
// not survive); the edge with the larger row `hi` belongs at j0 + the number of edges there with a smaller one.  Counting, not sorting:
// j is distinct within a segment, so the places of a segment are a permutation of j0 .. j1 - 1, and the work is linear in the segment
// for every edge, whatever its length.  An empty segment gives j0.
CELL_HD inline long long cell_rank_in_segment(const int* s_hi, long long j0, long long j1, int hi) {
  long long at = j0;
  for (long long j = j0; j < j1; ++j) at += s_hi[j] < hi;
  return at;
}

// ---- the edge key of the minimum spanning forest (cellmst.hip): edges are ordered by (d2, lo, hi) with lo < hi the two rows.  The bit
// budget, stated here once: an edge has d2 <= reach^2 <= 16384^2 = 2^28, which takes 29 bits (0 .. 2^28 inclusive), and rows are
// < 2^24 (MST_MAX_POINTS), 24 bits each: 29 + 24 + 24 = 77 bits, more than one 64-bit atomic holds.  The front (d2, lo) is 53 bits and
// fits: mst_key packs it so that the unsigned order of the packed words IS the lexicographic order of (d2, lo); hi is compared apart.
// MST_NO_KEY, all ones, is above every key (a key is < 2^53).
constexpr int MST_ROW_BITS = 24;
constexpr int64_t MST_MAX_POINTS = (int64_t)1 << MST_ROW_BITS;
constexpr int MST_MAX_D2 = CELL_MAX_REACH * CELL_MAX_REACH;        // 2^28
constexpr unsigned long long MST_NO_KEY = ~0ull;
CELL_HD inline unsigned long long mst_key(int d2, int lo) { return ((unsigned long long)(unsigned)d2 << MST_ROW_BITS) | (unsigned long long)(unsigned)lo; }
CELL_HD inline int mst_key_d2(unsigned long long key) { return (int)(key >> MST_ROW_BITS); }
CELL_HD inline int mst_key_lo(unsigned long long key) { return (int)(key & (((unsigned long long)1 << MST_ROW_BITS) - 1)); }
// is the edge (key a, hi a) in front of the edge (key b, hi b)?  The strict total order of the definition
CELL_HD inline bool mst_edge_less(unsigned long long ka, int ha, unsigned long long kb, int hb) { return ka < kb || (ka == kb && ha < hb); }

// ---- the two emptiness tests of the proximity graphs (cellprox.hip): does the witness k block the candidate pair (i, j)?  Functions of
// the three squared distances alone.  dij = d2(i, j) >= 0 is the candidate's (within reach), dik = d2(i, k) >= 0 the witness's from the
// end the sweep runs around, and djk = cell_pair_d2 of (j, k): -1 when k is out of j's reach, and then k blocks in neither test -- it is
// farther from j than the reach, hence farther than dij.  Why nothing overflows, stated here once: every d2 that is not -1 is at most
// reach^2 <= 16384^2 = 2^28, so dik + djk <= 2^29 < 2^31.  Both tests are STRICT: a witness on the circle with diameter ij (a right
// angle at k: dik + djk == dij) and a witness as far from an end as the other end is (max == dij) do not block; a witness coincident
// with an end never blocks (dik == 0 gives djk == dij, and dik == dij is not < dij), so neither end needs to be told from a witness.
// Gabriel-blocked implies RNG-blocked (two non-negative terms with a sum below dij are each below it): every RNG edge is a Gabriel edge.
CELL_HD inline bool prox_gabriel_blocked(int dik, int djk, int dij) { return djk >= 0 && dik + djk < dij; }
CELL_HD inline bool prox_rng_blocked(int dik, int djk, int dij) { return djk >= 0 && dik < dij && djk < dij; }
// an edge's d2 (<= 2^28) and its RNG bit in one int while the segments are put in order
constexpr int PROX_RNG_BIT = 1 << 30;

// ---- the site rasters (cellsites.h; celldensity.hip first): the queries are lattice SITES q = (g * s), not points, and a site may lie outside the box on
// every side.  The bit budget, stated here once: a site has |q| < 2^28 (checked on the host in 64 bits) and a point |p| < 2^27, so
// |q - p| < 2^28 + 2^27 < 2^31 and the differences are exact int32 -- the same holds for q - x_min and for q +- h - x_min (h <= 2^14).
// The box test against h comes BEFORE the products (cell_pair_d2), so d2 <= h * h <= 2^28 and each term h * h - d2 lies in 0 .. 2^28.
// With n <= 2^24 points a weight stays below 2^24 * 2^28 = 2^52: `weight` is int64; `count` <= 2^24 is int32.
constexpr int SITE_LIMIT = 1 << 28;                    // |g * s| < 2^28 half pixels
constexpr int SITE_MAX_PITCH = 1 << 20;
constexpr int SITE_TILE = 16;                          // a workgroup owns SITE_TILE x SITE_TILE sites
constexpr int64_t DENS_MAX_SITES = (int64_t)1 << 24;

// floor(a / b) for b > 0 (the / of C++ truncates toward zero, which is not the floor left of the origin)
CELL_HD inline int cell_floor_div(int a, int b) { return a / b - (a % b < 0); }

// the cell a coordinate falls in along one axis of a grid that starts at `origin`: the floor, so negative left of the box and >= the
// number of cells right of it (|v - origin| < 2^31 by the budget above)
CELL_HD inline int site_cell(int v, int origin, int side) { return cell_floor_div(v - origin, side); }

// the cells of one axis (nc of them) that the interval lo .. hi can touch, clamped to the grid: c0 .. c1, EMPTY (c0 > c1) when the interval
// lies wholly outside.  For a site q with lo = q - h and hi = q + h these are at most three cells (side >= h), the site's own and its
// neighbours as far as they exist; for a tile of sites it is the tile's footprint grown by h.
CELL_HD inline void site_cell_range(int lo, int hi, int origin, int side, int nc, int* c0, int* c1) {
  const int a = site_cell(lo, origin, side), b = site_cell(hi, origin, side);
  *c0 = a > 0 ? a : 0;
  *c1 = b < nc - 1 ? b : nc - 1;
}

// the cells a footprint x_lo .. x_hi, y_lo .. y_hi can touch on a grid of ncx x ncy cells that starts at (x_min, y_min): the rows cy0 .. cy1 and
// in each the cells cx0 .. cx1.  A footprint beside the grid has NO ROW (cy0 > cy1), whichever axis it misses the grid on: the one loop
// over the rows then reads nothing, and cx0 .. cx1 is never turned into an index.  The one place this rule is written: both forms of
// site_sweep (cellsites.h) and the walk of the host checks (tools/dev/cellsites_check.h) call it.
struct SiteCells { int cx0, cx1, cy0, cy1; };
CELL_HD inline SiteCells site_cells(int x_lo, int x_hi, int y_lo, int y_hi, int x_min, int y_min, int side, int ncx, int ncy) {
  SiteCells c;
  site_cell_range(x_lo, x_hi, x_min, side, ncx, &c.cx0, &c.cx1);
  site_cell_range(y_lo, y_hi, y_min, side, ncy, &c.cy0, &c.cy1);
  if (c.cx0 > c.cx1) c.cy1 = c.cy0 - 1;
  return c;
}

// the site (u, v) that thread tid of tile `tile` takes in a window with tiles_x tiles to a row: tiles in row-major order, and so are the
// 16 x 16 sites of a tile.  (u, v) may lie past the window's edge in the last tile of a row or column.
CELL_HD inline void site_uv(unsigned tile, int tiles_x, int tid, int* u, int* v) {
  *u = (int)(tile % tiles_x) * SITE_TILE + (tid & (SITE_TILE - 1));
  *v = (int)(tile / tiles_x) * SITE_TILE + tid / SITE_TILE;
}

// what a point at (dx, dy) from a site adds to the site's weight, h * h - d2, or -1 when it is out of reach (h2 = h * h; inclusive: a
// point exactly at distance h adds 0 and is counted)
CELL_HD inline int dens_term(int dx, int dy, int h, int h2) {
  const int d2 = cell_pair_d2(dx, dy, h, h2);
  return d2 < 0 ? -1 : h2 - d2;
}

// which kernel takes the sites, for every raster on this lattice.  A tile of 16 x 16 sites staged through LDS tests every record of its
// footprint, about 15 s + 2 r + side along each axis, against every site; a site on its own tests the records of its (at most) three cells,
// about 2 r + side along each axis.  The staged test is cheaper (a broadcast LDS read against a global load), the direct one tests fewer
// records as soon as the sites of a tile are far apart: the tile is taken while its footprint is at most twice as long as one site's
// (measured on both sides of the rule: profiles/cell_density.json, profiles/cell_territory.json).
CELL_HD inline bool site_route_staged(int s, int reach, int side) { return (long long)(SITE_TILE - 1) * s <= 2LL * reach + side; }

// the window of sites: W, H >= 1, W * H <= max_sites (DENS_MAX_SITES or TERR_MAX_SITES), and every site coordinate within +-2^28, all in
// 64 bits
inline bool site_window_ok(int s, int gx0, int gy0, int W, int H, int64_t max_sites) {
  if (s < 1 || s > SITE_MAX_PITCH || W < 1 || H < 1 || (int64_t)W * H > max_sites) return false;
  const int64_t lim = SITE_LIMIT;
  const int64_t xa = (int64_t)gx0 * s, xb = ((int64_t)gx0 + W - 1) * s, ya = (int64_t)gy0 * s, yb = ((int64_t)gy0 + H - 1) * s;
  return xa > -lim && xa < lim && xb > -lim && xb < lim && ya > -lim && ya < lim && yb > -lim && yb < lim;
}

// ---- nucleus territories (cellterritory.hip): the sites of the density rasters again, but each site keeps ONE point -- the argmin of
// (d2, row) over the points with a label in 0 .. C - 1 within the reach R (inclusive) -- instead of a sum over all of them.  The bit budget,
// stated here once: the differences q - p are exact int32 as above; the box test against R comes BEFORE the products (cell_pair_d2), so
// d2 <= R * R <= 2^28, 29 bits; a row is < 2^24.  (d2, row) packs into one 64-bit word with d2 in the high half, so the unsigned order of
// the words IS the lexicographic order of the pairs and the argmin is one compare; TERR_NO_KEY, all ones, is above every key.  One int32
// per site and map, so the window may hold 2^28 sites (density: 12 C bytes per site, 2^24); `area` <= 2^28 is int32.  The tally of a
// workgroup is a 32-bit table [(C + 1)][(C + 1)], class C being "none": a site adds at most 4 to one entry (its four neighbours) and 1 to
// its census entry, so a workgroup that took EVERY site of the largest window holds at most 4 * 2^28 = 2^30 in an entry: the table is
// flushed once, at the end, and cannot overflow (terr_table_fits); the int64 outputs hold 4 * 2^28 with room to spare.
constexpr int64_t TERR_MAX_SITES = (int64_t)1 << 28;
constexpr unsigned long long TERR_NO_KEY = ~0ull;
constexpr int TERR_TABLE_WORDS = (CELL_MAX_CLASSES + 1) * (CELL_MAX_CLASSES + 1);
constexpr int TERR_PER_SITE = 4;                       // the most one site adds to one entry of the tally table

CELL_HD inline unsigned long long terr_key(int d2, int row) { return ((unsigned long long)(unsigned)d2 << 32) | (unsigned long long)(unsigned)row; }
CELL_HD inline int terr_key_d2(unsigned long long key) { return key == TERR_NO_KEY ? -1 : (int)(key >> 32); }
CELL_HD inline int terr_key_row(unsigned long long key) { return key == TERR_NO_KEY ? -1 : (int)(key & 0xffffffffull); }

// the key a point at (dx, dy) from a site offers, or TERR_NO_KEY when it does not compete (its label is outside 0 .. C - 1) or is out
// of reach (R2 = R * R; inclusive)
CELL_HD inline unsigned long long terr_offer(int dx, int dy, int label, int row, int C, int R, int R2) {
  if ((unsigned)label >= (unsigned)C) return TERR_NO_KEY;
  const int d2 = cell_pair_d2(dx, dy, R, R2);
  return d2 < 0 ? TERR_NO_KEY : terr_key(d2, row);
}

// the tally table of a workgroup: entry [a][b] with a, b < C counts the ordered (site, 4-neighbour) pairs whose owners differ and have the
// classes a and b; column C ("none") holds the census of the sites: [a][C] the sites owned by class a, [C][C] the sites nobody owns.
// Row C is otherwise unused: a site nobody owns is in no contact.
CELL_HD inline int terr_table_at(int a, int b, int C) { return a * (C + 1) + b; }
CELL_HD inline bool terr_table_fits(int64_t sites_of_a_workgroup) { return sites_of_a_workgroup * TERR_PER_SITE <= (int64_t)0xffffffffll; }
static_assert(TERR_MAX_SITES * TERR_PER_SITE <= (int64_t)0xffffffffll, "one flush at the end of the tally kernel is enough");

// ---- territory adjacency (celladjacency.hip): the discrete Delaunay graph read off a finished owner map.  A SITE PAIR is an unordered pair
// of 4-adjacent sites inside the window, counted once: from its left or upper site, as that site's RIGHT or LOWER pair (adj_site_pairs).
// It is an edge when the two owners differ and both are rows (adj_is_edge); its key holds the smaller row in the high word, so the
// unsigned order of the keys IS the ascending (i, j) order of the edges, and no key is all ones (rows are below 2^24): ADJ_NO_KEY marks an
// empty slot.  The bit budget, stated here once: a window has at most 2 * 2^28 = 2^29 site pairs, so the records M of a call, the edges m
// and every entry of `shared` are at most 2^29 and fit an int32; a tile of 16 x 16 sites takes 2 * 256 = 512 of them, so its table of 1024
// slots is at most half full; the call's table has next_pow2(2 M) >= 2 M slots (at least ADJ_MIN_SLOTS, at most 2^30) and holds at most M
// keys, so it is at most half full as well: linear probing from adj_slot_of always meets the key or an empty slot.
constexpr unsigned long long ADJ_NO_KEY = ~0ull;
constexpr int ADJ_TILE_PAIRS = 2 * SITE_TILE * SITE_TILE;          // the site pairs a tile takes: a right and a lower one per site
constexpr int ADJ_TILE_SLOTS = 1024;
constexpr int64_t ADJ_MAX_RECORDS = 2 * TERR_MAX_SITES;           // 2^29
constexpr int64_t ADJ_MIN_SLOTS = 1024;
static_assert(2 * ADJ_TILE_PAIRS <= ADJ_TILE_SLOTS && (ADJ_TILE_SLOTS & (ADJ_TILE_SLOTS - 1)) == 0, "the tile table is at most half full: it cannot fill");
static_assert(ADJ_MAX_RECORDS <= (int64_t)1 << 29, "M, m and shared fit an int32; the call's table has at most 2^30 slots");

CELL_HD inline unsigned long long adj_key(int a, int b) {          // a != b, both rows
  const unsigned lo = (unsigned)(a < b ? a : b), hi = (unsigned)(a < b ? b : a);
  return ((unsigned long long)lo << 32) | (unsigned long long)hi;
}
CELL_HD inline int adj_key_lo(unsigned long long key) { return (int)(key >> 32); }
CELL_HD inline int adj_key_hi(unsigned long long key) { return (int)(key & 0xffffffffull); }

// an owner is -1 (nobody) or a row; two owners make an edge when they differ and both are rows.  A value outside -1 .. n - 1 makes none
// (and the call is refused: adj_owner_ok is the check, and it comes before any owner is used as an index)
CELL_HD inline bool adj_owner_ok(int o, int n) { return o >= -1 && o < n; }
CELL_HD inline bool adj_is_edge(int a, int b, int n) { return a != b && (unsigned)a < (unsigned)n && (unsigned)b < (unsigned)n; }

// the site pairs site (u, v) takes inside a window of W x H sites: bit 0 its right pair, bit 1 its lower one.  Over all sites every pair
// of the window comes up exactly once
CELL_HD inline int adj_site_pairs(int u, int v, int W, int H) { return (int)(u + 1 < W) | ((int)(v + 1 < H) << 1); }

// where the probe of a key starts in a table of `slots` (a power of two) slots: the finaliser of MurmurHash3 over the 64 bits
CELL_HD inline unsigned long long adj_slot_hash(unsigned long long key) {
  key ^= key >> 33; key *= 0xff51afd7ed558ccdull;
  key ^= key >> 33; key *= 0xc4ceb9fe1a85ec53ull;
  return key ^ (key >> 33);
}
CELL_HD inline unsigned long long adj_slot_of(unsigned long long key, unsigned long long slots) { return adj_slot_hash(key) & (slots - 1); }

// the slots of the call's table for M records: the power of two at or above 2 M, at least ADJ_MIN_SLOTS.  0 <= M <= 2^29
CELL_HD inline int64_t adj_table_slots(int64_t M) {
  int64_t slots = ADJ_MIN_SLOTS;
  while (slots < 2 * M) slots <<= 1;
  return slots;
}

inline bool adj_call_ok(int W, int H, int64_t n, int64_t edge_cap) {
  return W >= 1 && H >= 1 && (int64_t)W * H <= TERR_MAX_SITES && n >= 0 && n <= MST_MAX_POINTS && edge_cap >= 0 && edge_cap <= (int64_t)INT32_MAX;
}

// ---- the alpha complex (cellalpha.hip): the exact Delaunay edges within a radius r (1 .. 512 half pixels, D = 2 r the diameter).  For a
// candidate pair with q = p_j - p_i and d2 = |q|^2 <= D^2, the circles through both ends have the centres (q + t q_perp) / 2 and the squared
// radius d2 (1 + t^2) / 4: radius <= r exactly when t^2 <= (D^2 - d2) / d2 = T^2.  A witness at rho = p_k - p_i has s = q x rho and
// m = rho . (rho - q) and lies strictly inside circle t exactly when t s > m: s > 0 allows t <= m / s (the bound `hi` is the smallest such),
// s < 0 allows t >= m / s (`lo`, the largest), s == 0 blocks the pair outright when m < 0 (strictly between the ends) and does not bind
// otherwise (a witness coincident with an end has s = m = 0, so an end needs not be told from a witness).  The pair is an edge when it is
// not blocked, hi >= -T, lo <= T and lo <= hi, all inclusive; it is Gabriel when no witness has m < 0 (m < 0 is d2(i, k) + d2(j, k) < d2(i, j)).
// The bit budget, stated here once: a witness that binds within [-T, T] or kills the pair lies on or inside a circle of radius <= r
// through both ends, hence within D of i and of j; alpha_witness skips every other one BEFORE any product of s or m is formed (two box
// tests, then two squared distances of differences <= D = 2^10, each <= 2^21).  For the rest |rho| <= D and |rho - q| <= D give
// |s| <= D^2 = 2^20 and |m| <= D^2 (Cauchy-Schwarz), exact in int32 (each a sum of two products below 2^20).  A bound is the fraction
// (num, den) with den > 0, |num|, den <= 2^20: comparing two cross-multiplies to below 2^40 (alpha_frac_cmp), and comparing one with +-T is
// a sign test followed by num^2 d2 <= den^2 (D^2 - d2), both sides below 2^40 * 2^20 = 2^60 (alpha_within_T): int64 throughout.
constexpr int ALPHA_MAX_R = 512;                       // half pixels; the reach of the binning is D = 2 r <= 1024
constexpr int ALPHA_GABRIEL_BIT = 1 << 30;             // an edge's d2 (<= 2^20) and its Gabriel bit in one int while the segments are put in order

// the sign of a / b - c / d for b, d > 0
CELL_HD inline int alpha_frac_cmp(int64_t a, int64_t b, int64_t c, int64_t d) {
  const int64_t l = a * d, r = c * b;
  return (l > r) - (l < r);
}
// |a / b| <= T, b > 0: a^2 d2 <= b^2 (D^2 - d2).  0 < d2 <= D2
CELL_HD inline bool alpha_within_T(int64_t a, int64_t b, int d2, int D2) { return a * a * d2 <= b * b * (int64_t)(D2 - d2); }
CELL_HD inline bool alpha_le_T(int64_t a, int64_t b, int d2, int D2) { return a <= 0 || alpha_within_T(a, b, d2, D2); }         // a / b <= T
CELL_HD inline bool alpha_ge_neg_T(int64_t a, int64_t b, int d2, int D2) { return a >= 0 || alpha_within_T(a, b, d2, D2); }     // a / b >= -T

// what the witnesses seen so far leave of a candidate: hi = hn / hd attained by row hk (hd == 0: open), lo = ln / ld by row lk
struct AlphaState {
  int hn, hd, hk, ln, ld, lk;
  bool blocked, gabriel;
};
CELL_HD inline AlphaState alpha_open() { return AlphaState{0, 0, -1, 0, 0, -1, false, true}; }

// one witness, row `row` at (rx, ry) from i, against the candidate with q = (qx, qy) and the diameter D (D2 = D * D).  -> whether a bound
// moved or the pair was blocked (then alpha_dead is worth asking).  The smallest row that attains a bound is kept
CELL_HD inline bool alpha_witness(AlphaState& st, int qx, int qy, int rx, int ry, int row, int D, int D2) {
  const int ux = rx - qx, uy = ry - qy;                // from j: |p| < 2^27 keeps every difference an exact int32
  if (rx > D || rx < -D || ry > D || ry < -D || ux > D || ux < -D || uy > D || uy < -D) return false;
  if (rx * rx + ry * ry > D2 || ux * ux + uy * uy > D2) return false;
  const int s = qx * ry - qy * rx, m = rx * ux + ry * uy;
  if (m < 0) st.gabriel = false;
  if (s == 0) {
    if (m >= 0) return false;
    st.blocked = true;
    return true;
  }
  if (s > 0) {
    const int c = st.hd ? alpha_frac_cmp(m, s, st.hn, st.hd) : -1;
    if (c < 0) { st.hn = m; st.hd = s; st.hk = row; return true; }
    if (c == 0 && row < st.hk) st.hk = row;
    return false;
  }
  const int c = st.ld ? alpha_frac_cmp(-m, -s, st.ln, st.ld) : 1;
  if (c > 0) { st.ln = -m; st.ld = -s; st.lk = row; return true; }
  if (c == 0 && row < st.lk) st.lk = row;
  return false;
}

// can no further witness make the candidate an edge?  (d2 > 0)
CELL_HD inline bool alpha_dead(const AlphaState& st, int d2, int D2) {
  if (st.blocked) return true;
  if (st.hd && !alpha_ge_neg_T(st.hn, st.hd, d2, D2)) return true;
  if (st.ld && !alpha_le_T(st.ln, st.ld, d2, D2)) return true;
  return st.hd && st.ld && alpha_frac_cmp(st.ln, st.ld, st.hn, st.hd) > 0;
}

// the verdict once every witness is in: bit 0 the pair is an edge, bit 1 it is Gabriel as well; apex[0] the row that attains hi when
// hi <= T, apex[1] the one that attains lo when lo >= -T, else -1 (written for an edge only)
CELL_HD inline int alpha_verdict(const AlphaState& st, int d2, int D2, int* apex) {
  if (alpha_dead(st, d2, D2)) return 0;
  apex[0] = st.hd && alpha_le_T(st.hn, st.hd, d2, D2) ? st.hk : -1;
  apex[1] = st.ld && alpha_ge_neg_T(st.ln, st.ld, d2, D2) ? st.lk : -1;
  return 1 | ((int)st.gabriel << 1);
}

// ---- the alpha-shape outline (celloutline.hip): the rings of the alpha complex, traced by a successor map on the half-edges.  The
// successor of the half-edge u -> v is the out-half-edge v -> w met first when turning CLOCKWISE from the direction a = u - v (through
// the material, which lies on the left of u -> v); b = w - v is a candidate.  The clockwise angle from a to b falls in one of four
// classes, told by the signs of a x b and a . b: 0 (the same direction: a x b == 0, a . b >= 0 -- no out-half-edge of an alpha complex has
// it, the farther end would be blocked by the nearer), 1 (strictly between 0 and pi: a x b < 0), 2 (pi: a x b == 0, a . b < 0) and 3
// (beyond pi: a x b > 0).  Two candidates of one class 1 or 3 lie within one open half-turn, where b1 comes first exactly when
// b1 x b2 < 0.  The bit budget, stated here once: the vectors of an alpha complex are no longer than D = 2 r <= 1024, so every product is
// at most 2^20 and every cross or dot product below 2^21; the entry point accepts ANY edge list between points with |p| < 2^27, and then
// the differences are below 2^28, the products below 2^56 and their sums below 2^57: exact in int64 either way.
constexpr int64_t OUTLINE_MAX_EDGES = (int64_t)1 << 24;            // the scans over the edges take 1024 chunks of 16384
CELL_HD inline int outline_turn_class(int64_t ax, int64_t ay, int64_t bx, int64_t by) {
  const int64_t cr = ax * by - ay * bx;
  if (cr < 0) return 1;
  if (cr > 0) return 3;
  return ax * bx + ay * by < 0 ? 2 : 0;
}
// is b1 met strictly before b2 when turning clockwise from a?  (false for two candidates of one direction)
CELL_HD inline bool outline_turn_before(int64_t ax, int64_t ay, int64_t b1x, int64_t b1y, int64_t b2x, int64_t b2y) {
  const int c1 = outline_turn_class(ax, ay, b1x, b1y), c2 = outline_turn_class(ax, ay, b2x, b2y);
  if (c1 != c2) return c1 < c2;
  return (c1 & 1) && b1x * b2y - b1y * b2x < 0;
}
// one step of the successor choice, a fold over the out-half-edges at v in ANY order: does the candidate (b, id) replace the best so
// far?  Two candidates of one direction (none in an alpha complex) are told apart by the smaller id, so the choice is a strict total
// order and the fold's result does not depend on the order of the candidates.
CELL_HD inline bool outline_better(int64_t ax, int64_t ay, int64_t bx, int64_t by, int id, int64_t best_x, int64_t best_y, int best_id) {
  if (best_id < 0) return true;
  if (outline_turn_before(ax, ay, bx, by, best_x, best_y)) return true;
  if (outline_turn_before(ax, ay, best_x, best_y, bx, by)) return false;
  return id < best_id;
}
// the side of the apex at rho = p_k - p_i of the edge q = p_j - p_i: > 0 on the left (apex[0]'s side), < 0 on the right (apex[1]'s)
CELL_HD inline int64_t outline_side(int64_t qx, int64_t qy, int64_t rx, int64_t ry) { return qx * ry - qy * rx; }
CELL_HD inline bool outline_coord_ok(int x, int y) { return x > -CELL_COORD_LIMIT && x < CELL_COORD_LIMIT && y > -CELL_COORD_LIMIT && y < CELL_COORD_LIMIT; }
// the doubling rounds after which a jump covers h half-edges: the smallest k with 2^k >= h
CELL_HD inline int outline_rounds(int64_t h) { int k = 0; while (((int64_t)1 << k) < h) ++k; return k; }
inline bool outline_call_ok(int64_t n, int64_t m, int by_class) {
  return n >= 0 && n <= ((int64_t)1 << 24) && m >= 0 && m <= OUTLINE_MAX_EDGES && (by_class == 0 || by_class == 1);
}

// ---- nuclei by region (cellregion.hip): the second input is not the points but polygon EDGES (ax, ay, bx, by), and the test is a
// point against an edge.  The bit budget, stated here once: a point and a vertex both have |v| < 2^27, so every difference (hi - lo,
// p - lo, b - a, p - a) is below 2^28 in magnitude and exact in int32; a product of two of them is below 2^56 and the difference of two
// products below 2^57: the cross product is exact in int64 (float64 holds 53 bits and decides the side of a long thin edge wrongly).
// The slab of a y inside the box is (y - y_min) / side with 0 <= y - y_min < 2^28.
constexpr int64_t REGION_MAX_EDGES = (int64_t)1 << 22;
constexpr int64_t REGION_MAX_REGIONS = (int64_t)1 << 16;
constexpr int64_t REGION_MAX_SLOTS = (int64_t)1 << 28;  // (edge, slab) records of one call: the cap a caller may state
constexpr int REGION_MAX_CELLS = 1 << 22;
constexpr int REGION_STAGE = 256;                      // edge records staged through LDS at a time = threads of a workgroup

// is the edge a -> b crossed by the ray from p towards +x?  Half-open in y: the edge straddles p when exactly one end has y <= p.y; the
// straddling edge is oriented upward (lo the end with the smaller y) and crossed when p lies strictly on its -x side.
CELL_HD inline bool region_crossed(int ax, int ay, int bx, int by, int px, int py) {
  if ((ay <= py) == (by <= py)) return false;
  const bool up = ay < by;
  const int lx = up ? ax : bx, ly = up ? ay : by, hx = up ? bx : ax, hy = up ? by : ay;
  return (int64_t)(hx - lx) * (py - ly) - (int64_t)(hy - ly) * (px - lx) > 0;
}

// does p lie ON the edge a -> b?  The cross product on a -> b is 0 and p is in the closed bounding box of the edge (a zero-length edge:
// p == a).  The box comes first: it spares the products for nearly every edge.
CELL_HD inline bool region_on_edge(int ax, int ay, int bx, int by, int px, int py) {
  if (px < (ax < bx ? ax : bx) || px > (ax < bx ? bx : ax) || py < (ay < by ? ay : by) || py > (ay < by ? by : ay)) return false;
  return (int64_t)(bx - ax) * (py - ay) - (int64_t)(by - ay) * (px - ax) == 0;
}

// the slabs (rows of the points' grid: slab k holds y_min + k * side .. y_min + (k + 1) * side - 1) that the closed y-range of an edge,
// GROWN by R, meets, clipped to the points' box: s0 .. s1, or false for none.  R == 0 (the census): false when no point of the box can
// cross or touch the edge -- it lies wholly above, below or LEFT of the box (a crossed edge lies beyond p towards +x, a touched one
// holds p in its bounding box).  R = the largest threshold (the margin bands): the slabs whose points can cross the edge or lie within
// R of it; false when the grown range misses the box in y or the edge lies wholly left of x_min - R (it can be neither crossed nor
// near).  An edge wholly right of the box stays: every ray runs that way.  |v| < 2^27 and R <= 2^14: no sum overflows.
CELL_HD inline bool edge_slab_range(int ax, int ay, int bx, int by, int R, int x_min, int y_min, int y_max, int side, int* s0, int* s1) {
  const int ylo = (ay < by ? ay : by) - R, yhi = (ay < by ? by : ay) + R;
  if (yhi < y_min || ylo > y_max || (ax < x_min - R && bx < x_min - R)) return false;
  *s0 = ((ylo > y_min ? ylo : y_min) - y_min) / side;
  *s1 = ((yhi < y_max ? yhi : y_max) - y_min) / side;
  return true;
}

// an edge the entry point accepts: both ends within the coordinate range, its region among the G regions and not below the region of
// the edge in front of it (prev_region; 0 in front of the first edge)
CELL_HD inline bool region_edge_ok(int ax, int ay, int bx, int by, int region, int prev_region, int G) {
  const int L = CELL_COORD_LIMIT;
  return ax > -L && ax < L && ay > -L && ay < L && bx > -L && bx < L && by > -L && by < L && region >= 0 && region < G && prev_region <= region;
}

inline bool region_call_ok(int64_t E, int64_t G, int slab, int64_t slot_cap) {
  return E >= 0 && E <= REGION_MAX_EDGES && G >= 0 && G <= REGION_MAX_REGIONS && slab >= 1 && slab <= CELL_MAX_REACH && slot_cap >= 0 &&
         slot_cap <= REGION_MAX_SLOTS;
}

// ---- margin bands (cellmargin.hip): "is p within e half pixels of the edge a -> b", for thresholds 1 <= e <= 16384.  The bit budget,
// stated here once: with d = b - a and w = p - a (every difference below 2^28), L2 = d.d, s = w.d, |w|^2 and |p - b|^2 are sums of two
// products below 2^56 each, below 2^57 and exact in int64, and so is the cross product d x w.  Past either end of the edge the question
// is |w|^2 <= e^2 (or |p - b|^2), an int64 compare.  Beside the edge the squared distance is the rational cross^2 / L2 and the question
// is cross^2 <= e^2 * L2: cross^2 < 2^114, and e^2 <= 2^28 times L2 < 2^57 is below 2^85 -- both sides fit 128 bits, held as two
// 64-bit words.  Float64 decides about 1 % of designed exact-threshold pairs wrongly (tests/margin_cases.py has one).
constexpr int MARGIN_MAX_BANDS = 32;

// the full product a * b of two 64-bit words: the one place the 128-bit arithmetic is written
CELL_HD inline void margin_mul_wide(uint64_t a, uint64_t b, uint64_t* hi, uint64_t* lo) {
#if defined(__HIP_DEVICE_COMPILE__)
  *hi = __umul64hi(a, b);
  *lo = a * b;
#else
  const unsigned __int128 p = (unsigned __int128)a * b;
  *hi = (uint64_t)(p >> 64);
  *lo = (uint64_t)p;
#endif
}

// what the edge a -> b measures of p, once for every threshold: past an end (or on a zero-length edge) *q = the squared distance to
// that end and *l2 = 0; beside the edge *q = |d x w| and *l2 = L2 > 0, the squared distance being q^2 / l2
CELL_HD inline void margin_measure(int ax, int ay, int bx, int by, int px, int py, uint64_t* q, uint64_t* l2) {
  const int64_t dx = bx - ax, dy = by - ay, wx = px - ax, wy = py - ay;
  const int64_t L2 = dx * dx + dy * dy, s = wx * dx + wy * dy;
  *l2 = 0;
  if (L2 == 0 || s <= 0) { *q = (uint64_t)(wx * wx + wy * wy); return; }
  if (s >= L2) {
    const int64_t vx = px - bx, vy = py - by;
    *q = (uint64_t)(vx * vx + vy * vy);
    return;
  }
  const int64_t cr = dx * wy - dy * wx;
  *q = (uint64_t)(cr < 0 ? -cr : cr);
  *l2 = (uint64_t)L2;
}

// is the measured (q, l2) within e?  Inclusive.  l2 == 0: q <= e^2; else q^2 <= e^2 * l2 as (hi, lo) words
CELL_HD inline bool margin_within(uint64_t q, uint64_t l2, int e) {
  const uint64_t e2 = (uint64_t)((int64_t)e * e);
  if (l2 == 0) return q <= e2;
  uint64_t lh, ll, rh, rl;
  margin_mul_wide(q, q, &lh, &ll);
  margin_mul_wide(e2, l2, &rh, &rl);
  return lh < rh || (lh == rh && ll <= rl);
}

CELL_HD inline bool margin_near(int ax, int ay, int bx, int by, int px, int py, int e) {
  uint64_t q, l2;
  margin_measure(ax, ay, bx, by, px, py, &q, &l2);
  return margin_within(q, l2, e);
}

// can p be within r of an edge with the bounding box x0 .. x1, y0 .. y1?  Four compares, before any product
CELL_HD inline bool margin_box_near(int x0, int y0, int x1, int y1, int px, int py, int r) {
  return px >= x0 - r && px <= x1 + r && py >= y0 - r && py <= y1 + r;
}

// the thresholds row: 1 .. 32 of them, strictly increasing, within 1 .. 16384 half pixels
inline bool margin_thresholds_ok(const int32_t* t, int B) {
  if (!t || B < 1 || B > MARGIN_MAX_BANDS || t[0] < 1 || t[B - 1] > CELL_MAX_REACH) return false;
  for (int k = 1; k < B; ++k)
    if (t[k] <= t[k - 1]) return false;
  return true;
}

inline bool margin_call_ok(int64_t E, int64_t G, int slab, int64_t slot_cap, const int32_t* thresholds, int B) {
  return region_call_ok(E, G, slab, slot_cap) && margin_thresholds_ok(thresholds, B);
}

// ---- the front checks of an entry point, before anything is launched: the limits every analysis shares (its own n limit passed in),
// and, when there are points, the bounding box
inline bool cell_box_ok(int x_min, int y_min, int x_max, int y_max) {
  return x_min <= x_max && y_min <= y_max && x_min > -CELL_COORD_LIMIT && y_min > -CELL_COORD_LIMIT && x_max < CELL_COORD_LIMIT && y_max < CELL_COORD_LIMIT;
}
inline bool cell_call_ok(int64_t n, int64_t max_n, int C, int reach, int x_min, int y_min, int x_max, int y_max) {
  if (n < 0 || n > max_n || C < 1 || C > CELL_MAX_CLASSES || reach < 1 || reach > CELL_MAX_REACH) return false;
  return n == 0 || cell_box_ok(x_min, y_min, x_max, y_max);
}
inline bool alpha_call_ok(int64_t n, int C, int r, int by_class, int64_t edge_cap, int x_min, int y_min, int x_max, int y_max) {
  return r >= 1 && r <= ALPHA_MAX_R && (by_class == 0 || by_class == 1) && edge_cap >= 0 && edge_cap <= (int64_t)INT32_MAX &&
         cell_call_ok(n, MST_MAX_POINTS, C, 2 * r, x_min, y_min, x_max, y_max);
}
