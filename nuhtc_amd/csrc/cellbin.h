// What the per-slide analyses of half-pixel points share on the device (gfx950) -- the cell graph (cellgraph.hip), the pair histograms
// (cellspatial.hip), the clusters (cellcluster.hip), the minimum spanning forest (cellmst.hip), the proximity graphs (cellprox.hip), the alpha complex (cellalpha.hip), the density rasters (celldensity.hip), the territories (cellterritory.hip), the region census and the margin bands (cellregion.hip, cellmargin.hip: their edges are binned by celledges.h, on this scan) and the neighbourhood enrichment (cellenrich.hip); cellsites.h holds the lattice and the staged / direct sweep of the site rasters (celldensity.hip, cellterritory.hip), celledges.h the slab walk of the analyses against polygon edges (cellregion.hip, cellmargin.hip), celledgelist.h holds the count / scan / emit / place frame of the analyses that return an edge list (cellprox.hip, cellalpha.hip), celladjacency.hip uses the scan alone; cellgrid_host.h holds the plain-C++ side (limits, geometry, keys, pair distance).
//   binning   a histogram of the points per key (atomics), an exclusive scan of the keys, and a scatter of (x, y, label, index) records
//             into key order.  A key is a cell, or a (cell, class) pair (cell_key).  The order of the records INSIDE a key is atomic
//             arrival order; nothing downstream may depend on it.  A point outside the stated bounding box raises the flag and is left
//             out: the caller's later kernels test the flag and write nothing.
//   scan      exclusive scan of up to 1024 chunks of CB_CHUNK ints (ExScan, exscan_launch): block_exscan_1024 of block_prims.h on 16
//             ints per thread -- per-chunk totals, a scan of the totals, the chunks again with their base.
//   sweep     cell_sweep: the records within reach of a point, from the 3 x 3 cells around it (one key per cell).
//   witness   cell_rows and cell_pair_window: the three row ranges of those cells, and the window of them that can hold a witness of a
//             pair (the witness loops of cellprox.hip and cellalpha.hip).
//   epilogue  cellbin_finish: the flag read back, the stream synchronised, the return code.
#pragma once
#include "block_prims.h"
#include "cellgrid_host.h"
#include "common.h"

namespace {

constexpr int CB_SCAN_PER = 16;                       // ints per thread of the scan
constexpr int CB_CHUNK = 1024 * CB_SCAN_PER;          // ints per workgroup of the scan

struct ExScan {
  const int* in;            // [nchunk * CB_CHUNK], zero past the values
  int* out;                 // [nchunk * CB_CHUNK]: entry k = the sum of the values in front of k
  int* chunk_base;          // [1024]: the sum in front of each chunk
};

struct CellBin {
  const int32_t* points;    // [n][2] half pixels
  const int32_t* labels;    // [n]
  int n;
  int x_min, y_min, x_max, y_max, side, ncx, ncy;
  int sub;                  // keys per cell: 1, or C + 1 (the classes and one more for a label outside them)
  int* cell_count;          // [nchunk * CB_CHUNK], zero past the keys; counted up by the histogram, down again by the scatter
  int* cell_start;          // [nchunk * CB_CHUNK]: entry k = records in front of key k (entry ncx * ncy * sub: all of them)
  int* chunk_base;          // [1024]: records in front of each scan chunk
  int4* recs;               // [n] (x, y, label, index) in key order
  int* flag;                // != 0: a point lies outside the stated bounding box
};

// the key of a point, or -1 (and the flag) when it lies outside the box the grid was laid over
__device__ __forceinline__ int cb_key_of(const CellBin& a, int x, int y, int label) {
  if (x < a.x_min || x > a.x_max || y < a.y_min || y > a.y_max) { *a.flag = 1; return -1; }
  return cell_key(cell_index(x, y, a.x_min, a.y_min, a.side, a.ncx), label, a.sub);
}

__global__ __launch_bounds__(256) void cb_count_kernel(CellBin a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const int c = cb_key_of(a, a.points[2 * i], a.points[2 * i + 1], a.labels[i]);
  if (c >= 0) atomicAdd(&a.cell_count[c], 1);
}

// sum of the 16 ints of this thread (two 32-byte halves: 16-byte vector loads)
__device__ __forceinline__ int cb_load16(const int* __restrict__ src, int v[CB_SCAN_PER]) {
  int s = 0;
#pragma unroll
  for (int q = 0; q < CB_SCAN_PER / 4; ++q) {
    const int4 w = reinterpret_cast<const int4*>(src)[q];
    v[4 * q] = w.x; v[4 * q + 1] = w.y; v[4 * q + 2] = w.z; v[4 * q + 3] = w.w;
    s += w.x + w.y + w.z + w.w;
  }
  return s;
}

__global__ __launch_bounds__(1024) void cb_chunk_total_kernel(ExScan a) {
  __shared__ int lds16[17];
  int v[CB_SCAN_PER], total;
  const int s = cb_load16(a.in + (size_t)blockIdx.x * CB_CHUNK + threadIdx.x * CB_SCAN_PER, v);
  block_exscan_1024(s, lds16, &total);
  if (threadIdx.x == 0) a.chunk_base[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void cb_chunk_scan_kernel(ExScan a, int nchunk) {
  __shared__ int lds16[17];
  int total;
  const int v = (int)threadIdx.x < nchunk ? a.chunk_base[threadIdx.x] : 0;
  const int ex = block_exscan_1024(v, lds16, &total);
  if ((int)threadIdx.x < nchunk) a.chunk_base[threadIdx.x] = ex;
}

__global__ __launch_bounds__(1024) void cb_cell_scan_kernel(ExScan a) {
  __shared__ int lds16[17];
  int v[CB_SCAN_PER], total;
  const size_t at = (size_t)blockIdx.x * CB_CHUNK + threadIdx.x * CB_SCAN_PER;
  const int s = cb_load16(a.in + at, v);
  int acc = a.chunk_base[blockIdx.x] + block_exscan_1024(s, lds16, &total);
#pragma unroll
  for (int q = 0; q < CB_SCAN_PER / 4; ++q) {
    int4 w;
    w.x = acc; acc += v[4 * q];
    w.y = acc; acc += v[4 * q + 1];
    w.z = acc; acc += v[4 * q + 2];
    w.w = acc; acc += v[4 * q + 3];
    reinterpret_cast<int4*>(a.out + at)[q] = w;
  }
}

__global__ __launch_bounds__(256) void cb_scatter_kernel(CellBin a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const int x = a.points[2 * i], y = a.points[2 * i + 1], label = a.labels[i];
  const int c = cb_key_of(a, x, y, label);
  if (c < 0) return;
  const int pos = a.cell_start[c] + atomicSub(&a.cell_count[c], 1) - 1;       // the key fills from its end; the counts return to zero
  a.recs[pos] = make_int4(x, y, label, i);
}

// Lays the grid of `reach`-multiple cells (at most max_cells of them) over the box, allocates the tables and the records from `tmp` and
// clears the counts and the flag on s.  n >= 1, the box and the reach already checked.  Returns the number of scan chunks, or 0 when an
// allocation or a memset failed.
inline int cellbin_setup(CellBin& a, const int32_t* points, const int32_t* labels, int n, int x_min, int y_min, int x_max, int y_max, int reach,
                         int max_cells, int sub, DevScratch& tmp, hipStream_t s) {
  a.points = points; a.labels = labels; a.n = n; a.sub = sub;
  a.x_min = x_min; a.y_min = y_min; a.x_max = x_max; a.y_max = y_max;
  a.side = cell_grid_side(x_min, y_min, x_max, y_max, reach, max_cells);
  a.ncx = (int)cell_cells_along(x_min, x_max, a.side); a.ncy = (int)cell_cells_along(y_min, y_max, a.side);
  const int nkey = a.ncx * a.ncy * sub;                          // <= 2^22
  const int nchunk = (nkey + 1 + CB_CHUNK - 1) / CB_CHUNK;       // + 1: the entry behind the last key holds the total; at most 257
  const size_t keys_bytes = (size_t)nchunk * CB_CHUNK * sizeof(int);
  a.cell_count = tmp.alloc<int>(keys_bytes); a.cell_start = tmp.alloc<int>(keys_bytes);
  a.chunk_base = tmp.alloc<int>(1024 * sizeof(int)); a.flag = tmp.alloc<int>(sizeof(int));
  a.recs = tmp.alloc<int4>((size_t)n * sizeof(int4));
  if (!tmp.ok()) return 0;
  if (hipMemsetAsync(a.cell_count, 0, keys_bytes, s) != hipSuccess || hipMemsetAsync(a.flag, 0, sizeof(int), s) != hipSuccess) return 0;
  return nchunk;
}

// the three launches of the scan over nchunk * CB_CHUNK padded ints (nchunk <= 1024), on s
inline void exscan_launch(const ExScan& a, int nchunk, hipStream_t s) {
  hipLaunchKernelGGL(cb_chunk_total_kernel, dim3(nchunk), dim3(1024), 0, s, a);
  hipLaunchKernelGGL(cb_chunk_scan_kernel, dim3(1), dim3(1024), 0, s, a, nchunk);
  hipLaunchKernelGGL(cb_cell_scan_kernel, dim3(nchunk), dim3(1024), 0, s, a);
}

// the five launches of the binning, on s
inline void cellbin_launch(const CellBin& a, int nchunk, hipStream_t s) {
  const unsigned nb = (unsigned)((a.n + 255) / 256);
  hipLaunchKernelGGL(cb_count_kernel, dim3(nb), dim3(256), 0, s, a);
  exscan_launch(ExScan{a.cell_count, a.cell_start, a.chunk_base}, nchunk, s);
  hipLaunchKernelGGL(cb_scatter_kernel, dim3(nb), dim3(256), 0, s, a);
}

// f(j, o, d2) for every record o at position j that passes pre(o) and lies within `reach` of the record `me` -- me itself included
// (d2 == 0, o.w == me.w) unless pre refuses it -- on a grid with ONE key per cell: the three rows of the 3 x 3 cells around me, each one
// contiguous range of records.  The lanes of a wave sit in the same or adjacent cells and read the same records: one 16-byte load per
// record, the same address across most of the wave.  pre runs BEFORE the distance: a compare of two loaded words that spares the
// multiplies (with the test inside f instead, cc_degree_kernel compiled to 40 VGPRs for 22).
template <typename P, typename F>
__device__ __forceinline__ void cell_sweep(const CellBin& g, const int4 me, int reach, P&& pre, F&& f) {
  const int cx = (me.x - g.x_min) / g.side, cy = (me.y - g.y_min) / g.side;
  const int cx0 = max(cx - 1, 0), cx1 = min(cx + 1, g.ncx - 1), reach2 = reach * reach;
  for (int gy = max(cy - 1, 0); gy <= min(cy + 1, g.ncy - 1); ++gy) {
    const int j0 = g.cell_start[gy * g.ncx + cx0], j1 = g.cell_start[gy * g.ncx + cx1 + 1];
    for (int j = j0; j < j1; ++j) {
      const int4 o = g.recs[j];
      if (!pre(o)) continue;
      const int d2 = cell_pair_d2(o.x - me.x, o.y - me.y, reach, reach2);
      if (d2 >= 0) f(j, o, d2);
    }
  }
}

// ---- what the witness loops of cellprox.hip and cellalpha.hip share (the loops themselves differ in substance and stay apart)
// The three rows of the 3 x 3 cells around me (cell_sweep's), each one contiguous range of records: row t starts at position j0[t] and
// holds n[t] records, `total` in all; a row outside the grid is empty.
struct CellRows { int j0[3], n[3], total; };

__device__ __forceinline__ CellRows cell_rows(const CellBin& g, const int4& me) {
  const int cx = (me.x - g.x_min) / g.side, cy = (me.y - g.y_min) / g.side;
  const int cx0 = max(cx - 1, 0), cx1 = min(cx + 1, g.ncx - 1);
  CellRows w;
  w.total = 0;
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int gy = cy - 1 + t;
    const bool in = gy >= 0 && gy < g.ncy;                 // a row outside the grid is empty
    w.j0[t] = in ? g.cell_start[gy * g.ncx + cx0] : 0;
    w.n[t] = in ? g.cell_start[gy * g.ncx + cx1 + 1] - w.j0[t] : 0;
    w.total += w.n[t];
  }
  return w;
}

// The WINDOW of cells that can hold a witness of the pair (me, o) when a witness lies within d of BOTH ends: the overlap of the two boxes
// of half-width d around the ends, clipped to the box of the grid -- columns gx0 .. gx1 of rows gy0 .. gy1, inside the 3 x 3 cells around
// me when d <= side (at most three rows of at most three cells, each row one contiguous range of records).  gm is the row of the pair's
// midpoint, clamped to the window: the row to walk first, where the witnesses that decide a pair are likeliest.
struct CellWindow { int gx0, gx1, gy0, gy1, gm; };

__device__ __forceinline__ CellWindow cell_pair_window(const CellBin& g, const int4& me, const int4& o, int d) {
  const int xa = max(max(me.x, o.x) - d, g.x_min), xb = min(min(me.x, o.x) + d, g.x_max);
  const int ya = max(max(me.y, o.y) - d, g.y_min), yb = min(min(me.y, o.y) + d, g.y_max);
  CellWindow w;
  w.gx0 = (xa - g.x_min) / g.side; w.gx1 = (xb - g.x_min) / g.side; w.gy0 = (ya - g.y_min) / g.side; w.gy1 = (yb - g.y_min) / g.side;
  w.gm = min(max(((me.y + o.y) / 2 - g.y_min) / g.side, w.gy0), w.gy1);
  return w;
}

// The end of an entry point: were the launches accepted, the binning's flag read back (and, where the caller has one, one more int of
// its own: extra_dev -> *extra_host, written only on success), the stream synchronised.  -> 0, NUHTC_E_INVALID when a point lay outside
// the stated box, NUHTC_E_HIP.
inline int cellbin_finish(const CellBin& a, hipStream_t s, const int* extra_dev = nullptr, int* extra_host = nullptr) {
  int h_flag = 0, h_extra = 0;
  if (!launched() || hipMemcpyAsync(&h_flag, a.flag, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess) return NUHTC_E_HIP;
  if (extra_dev && hipMemcpyAsync(&h_extra, extra_dev, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess) return NUHTC_E_HIP;
  if (hipStreamSynchronize(s) != hipSuccess) return NUHTC_E_HIP;
  if (h_flag) return NUHTC_E_INVALID;
  if (extra_host) *extra_host = h_extra;
  return 0;
}

}  // namespace
