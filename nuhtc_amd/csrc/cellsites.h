// What the site rasters share on the device (gfx950) -- the density maps (celldensity.hip), the territories (cellterritory.hip) and, for
// the tile arithmetic alone, the adjacency that reads the territory map (celladjacency.hip): the analyses whose queries are the SITES of
// a lattice anchored at the slide's origin, one workgroup per tile of 16 x 16 sites and one thread per site, over the points binned by
// cellbin.h with one key per cell.  One copy of the lattice, of a thread's site and of the sweep; a file keeps its own argument block
// (CellBin b, then SiteLattice t, then its own fields), what a site does with a record (`take`), its write and its entry point.
//
// A site may lie outside the points' box on any side: its cell is a floor and the cells its footprint touches are clamped and may be none
// (site_cells of cellgrid_host.h, where the bit budget is stated); cell_sweep of cellbin.h assumes a query inside the box and is not used.
// Everything here that decides an index -- site_uv, site_cells, the window check and the route -- is plain C++ in cellgrid_host.h, and the
// host checks (tools/dev/cellsites_check.h) call those functions under -fsanitize=address,undefined.  The kernel code is not sanitized.
#pragma once
#include "cellbin.h"

namespace {

constexpr int SITE_NT = SITE_TILE * SITE_TILE;          // 256 sites, one thread each
constexpr int SITE_STAGE_BYTES = SITE_NT * (int)sizeof(int4);

struct SiteLattice { int reach, s, gx0, gy0, W, H, tiles_x; };     // site (u, v) lies at ((gx0 + u) * s, (gy0 + v) * s) half pixels

inline SiteLattice site_lattice(int reach, int s, int gx0, int gy0, int W, int H) {
  return SiteLattice{reach, s, gx0, gy0, W, H, (W + SITE_TILE - 1) / SITE_TILE};
}

// the site of this thread: (u, v) in the window, whether it exists, and its position in half pixels.  A thread past the window's edge
// takes the last site of its row or column (a valid coordinate) and writes nothing.
struct Site { int u, v, qx, qy; bool active; };
__device__ __forceinline__ Site site_of(const SiteLattice& t) {
  Site me;
  int u, v;
  site_uv(blockIdx.x, t.tiles_x, threadIdx.x, &u, &v);
  me.active = u < t.W && v < t.H;
  me.u = min(u, t.W - 1); me.v = min(v, t.H - 1);
  me.qx = (t.gx0 + me.u) * t.s; me.qy = (t.gy0 + me.v) * t.s;
  return me;
}

// The sweep of one site: take(const int4&) on every record (x, y, label, row) of the cells a footprint grown by the reach can touch, row
// of cells by row of cells; the records of a row are one contiguous range.  The barrier contract, stated here once:
//   STAGED  the footprint is the TILE's, so every bound of both loops is uniform over the workgroup and every thread, active or not,
//           meets every barrier -- also when the range is empty (no row: no barrier for anyone).  Row by row the workgroup copies the
//           records into stage[SITE_NT] (LDS, one 16-byte load per record and thread) between the two barriers, and every thread then
//           takes each staged record against its own site: a broadcast LDS read, the record uniform over the workgroup.
//   direct  the footprint is the site's own disc (at most 3 x 3 cells), straight from global memory.  No barrier, so an inactive thread
//           returns first; `stage` is not used.
// The caller has tested the binning's flag.
template <bool STAGED, class Take>
__device__ __forceinline__ void site_sweep(const CellBin& g, const SiteLattice& t, const Site& me, int4* __restrict__ stage, Take&& take) {
  const int tid = threadIdx.x, r = t.reach;
  if (!STAGED && !me.active) return;
  int x_lo = me.qx, x_hi = me.qx, y_lo = me.qy, y_hi = me.qy;
  if (STAGED) {
    int u0, v0;
    site_uv(blockIdx.x, t.tiles_x, 0, &u0, &v0);         // the tile's first site
    const int u1 = min(u0 + SITE_TILE, t.W) - 1, v1 = min(v0 + SITE_TILE, t.H) - 1;
    x_lo = (t.gx0 + u0) * t.s; x_hi = (t.gx0 + u1) * t.s; y_lo = (t.gy0 + v0) * t.s; y_hi = (t.gy0 + v1) * t.s;
  }
  const SiteCells c = site_cells(x_lo - r, x_hi + r, y_lo - r, y_hi + r, g.x_min, g.y_min, g.side, g.ncx, g.ncy);
  for (int gy = c.cy0; gy <= c.cy1; ++gy) {
    int j0 = g.cell_start[gy * g.ncx + c.cx0], j1 = g.cell_start[gy * g.ncx + c.cx1 + 1];
    if (STAGED) {
      j0 = __builtin_amdgcn_readfirstlane(j0); j1 = __builtin_amdgcn_readfirstlane(j1);        // uniform: the chunk loop stays scalar
      for (int base = j0; base < j1; base += SITE_NT) {
        __syncthreads();                                 // the chunk before this one has been read by everyone
        if (base + tid < j1) stage[tid] = g.recs[base + tid];
        __syncthreads();
        const int m = min(SITE_NT, j1 - base);
        for (int k = 0; k < m; ++k) take(stage[k]);
      }
    } else {
      for (int j = j0; j < j1; ++j) take(g.recs[j]);
    }
  }
}

// ---- the host side of a call
// the workgroups of a window, one per tile.  H = 1 gives the most tiles: (2^28 + 15) / 16 < 2^25
inline unsigned site_tiles(int W, int H) { return (unsigned)((W + SITE_TILE - 1) / SITE_TILE) * (unsigned)((H + SITE_TILE - 1) / SITE_TILE); }

// staged or direct: site_route_staged of cellgrid_host.h, or what the dev probe says whatever the shape (-DNUHTC_SITE_ROUTE=1 staged,
// =2 direct; per file with NUHTC_EXTRA_CFLAGS_CELLDENSITY / _CELLTERRITORY of build.py)
inline bool site_route(int s, int reach, int side) {
#ifdef NUHTC_SITE_ROUTE
  return NUHTC_SITE_ROUTE == 1;
#else
  return site_route_staged(s, reach, side);
#endif
}

template <class Args>
inline void site_launch(bool staged, void (*tile_kernel)(Args), void (*site_kernel)(Args), unsigned tiles, int lds_bytes, hipStream_t st, const Args& a) {
  hipLaunchKernelGGL(staged ? tile_kernel : site_kernel, dim3(tiles), dim3(SITE_NT), lds_bytes, st, a);
}

}  // namespace
