// Per-nucleus Fourier-descriptor integers (gfx950) for the Shape.FSD1..6 features: INTEGERS ONLY, a pure function of the ordered ring
// of a nucleus -- no mask, no frame, no tile.  nuhtc_amd/nucfsd.py defines the row and restates it in numpy (fsd_reference); the device
// must equal it bit for bit, and the host derives the six features.  The rings are the `verts` / `ring_off` of nuhtc_op_ring_fill
// (ringfeat.hip), read the same way.
//
// ring_fsd_kernel: one workgroup of 256 threads per ring, the ring walked twice in chunks of 256 edges (one edge a thread), so a ring
// of any length is measured; 2 KB of LDS for the cumulative pairs of ONE chunk.
//   1. every edge is classified (nucfsd_edge: on one of the eight chain directions, its unit steps, axial or diagonal) and the steps are
//      summed in int64 -> the totals A and B and the status.  A ring that is not measured leaves its status and zeros, and nothing else.
//   2. the ring again, chunk by chunk: an exclusive scan of the chunk's axial and diagonal steps (block_exscan of block_prims.h) on top
//      of the running carry gives (a_e, b_e), the start length of every edge of the chunk, in LDS.  The start lengths do not decrease
//      along the ring, so sample k lies in this chunk exactly when it has not been placed yet and the NEXT chunk starts beyond it (the
//      carry after this chunk, or the end of the ring); thread k < 128 then finds the last edge of the chunk that starts at or before the
//      sample by binary search with the exact comparison (nucfsd_search, nucfsd_sign: integers only) and writes its five numbers.
//      Every sample is placed in exactly one chunk, the last chunk taking whatever is left.
// Plain vector stores; no scratch, no atomics.
#include "block_prims.h"
#include "common.h"
#include "nucfsd_host.h"

namespace {

struct RingFsdParams {
  const int32_t* verts;      // [nv][2]
  const int64_t* ring_off;   // [n + 1]
  long long nv;
  int32_t* rows;             // [n][644]
  int32_t* status;           // [n]
};

// edge e of the ring of n vertices that starts at vertex `a` of verts: false when it is off the chain
__device__ __forceinline__ bool ring_edge(const int32_t* __restrict__ verts, long long a, int n, int e, int& x, int& y, int64_t& steps, bool& diagonal,
                                          int& code) {
  const long long v = a + e, nx = e + 1 < n ? v + 1 : a;
  x = verts[2 * v]; y = verts[2 * v + 1];
  return nucfsd_edge((int64_t)verts[2 * nx] - x, (int64_t)verts[2 * nx + 1] - y, steps, diagonal, code);
}

__global__ __launch_bounds__(NUCFSD_CHUNK) void ring_fsd_kernel(RingFsdParams p) {
  constexpr int NT = NUCFSD_CHUNK, NW = NT / 64;
  __shared__ int ca[NT], cb[NT], scan_lds[NW + 1];
  __shared__ long long part[2 * NW];
  const int i = blockIdx.x, tid = threadIdx.x;
  int32_t* __restrict__ row = p.rows + (size_t)i * NUCFSD_ROW;
  const long long a = p.ring_off[i], b = p.ring_off[i + 1];
  const bool listed = a >= 0 && b >= a && b <= p.nv;                  // the vertices are inside the array (nv <= 2^30: so is their count)
  const int n = listed ? (int)(b - a) : 0;
  // ---- 1. the edges: on the chain, and their steps in all
  long long sa = 0, sb = 0;
  int bad = 0;
  for (int e = tid; e < n; e += NT) {
    int x, y, code;
    int64_t steps;
    bool diagonal;
    if (!ring_edge(p.verts, a, n, e, x, y, steps, diagonal, code)) bad = 1;
    if (diagonal) sb += steps; else sa += steps;                       // steps < 2^32 and n <= 2^30: inside int64
  }
  sa = wave_sum(sa); sb = wave_sum(sb);
  if ((tid & 63) == 0) { part[tid >> 6] = sa; part[NW + (tid >> 6)] = sb; }
  const int off_chain = __syncthreads_or(bad);                         // (also: part[] is written)
  long long A = 0, B = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) { A += part[w]; B += part[NW + w]; }
  const int st = !listed || off_chain ? NUCFSD_NOT_TRACED : A + B == 0 ? NUCFSD_DEGENERATE : A + B > NUCFSD_MAX_STEPS ? NUCFSD_TOO_LONG : NUCFSD_OK;
  if (tid == 0) p.status[i] = st;
  if (st != NUCFSD_OK) {
    for (int w = tid; w < NUCFSD_ROW; w += NT) row[w] = w == 0 ? st : 0;
    return;
  }
  if (tid == 0) { row[0] = NUCFSD_OK; row[1] = (int)A; row[2] = (int)B; row[3] = n; }
  // ---- 2. the start length of every edge, a chunk at a time, and the samples that fall into the chunk
  int carry_a = 0, carry_b = 0;                                        // the steps before the chunk: at most 2^24 in all
  bool placed = tid >= NUCFSD_K;                                       // thread k < 128 places sample k
  for (int c0 = 0; c0 < n; c0 += NT) {
    const int e = c0 + tid, m = min(NT, n - c0);
    int x = 0, y = 0, code = 0, da = 0, db = 0;
    if (e < n) {
      int64_t steps;
      bool diagonal;
      ring_edge(p.verts, a, n, e, x, y, steps, diagonal, code);
      if (diagonal) db = (int)steps; else da = (int)steps;
    }
    int tot_a, tot_b;
    const int ea = carry_a + block_exscan<NT>(da, scan_lds, &tot_a), eb = carry_b + block_exscan<NT>(db, scan_lds, &tot_b);
    if (tid < m) { ca[tid] = ea; cb[tid] = eb; }
    carry_a += tot_a; carry_b += tot_b;
    __syncthreads();
    // the next chunk starts at (carry_a, carry_b): beyond sample k, or there is no next chunk
    if (!placed && (c0 + NT >= n || !nucfsd_at_or_before(carry_a, carry_b, tid, A, B))) {
      const int j = nucfsd_search(ca, cb, m, tid, A, B);
      int32_t* __restrict__ out = row + NUCFSD_HEAD + NUCFSD_PER * tid;
      int64_t steps;
      bool diagonal;
      ring_edge(p.verts, a, n, c0 + j, x, y, steps, diagonal, code);
      out[0] = x; out[1] = y; out[2] = code; out[3] = ca[j]; out[4] = cb[j];
      placed = true;
    }
    __syncthreads();                                                   // the chunk's pairs have been read
  }
}

}  // namespace

extern "C" {

int nuhtc_op_ring_fsd(int device, const int32_t* verts, int64_t nv, const int64_t* ring_off, int n, int32_t* rows, int32_t* status, void* stream) {
  if (!verts || !ring_off || !rows || !status || !nucfsd_args_ok(nv, n)) return NUHTC_E_INVALID;
  if (hipSetDevice(device) != hipSuccess) return NUHTC_E_HIP;
  hipStream_t s = (hipStream_t)stream;
  RingFsdParams p{verts, ring_off, (long long)nv, rows, status};
  ProfScope ps("ring_fsd", 0, (double)nv * 16 + (double)n * NUCFSD_ROW * 4, s);
  hipLaunchKernelGGL(ring_fsd_kernel, dim3((unsigned)n), dim3(NUCFSD_CHUNK), 0, s, p);
  return launched() ? 0 : NUHTC_E_HIP;
}

}  // extern "C"
