// Neighbourhood enrichment of a slide (gfx950): the class-pair contact counts of the nucleus centres, observed and under P label
// permutations -- the permutation test of histoCAT / squidpy's nhood_enrichment, with the positions kept and the labels shuffled.
//
// Definition (nuhtc_amd/enrichment.py holds it in full, with the brute-force restatement `enrichment_reference`): n points in HALF pixels
// (|p| < 2^27, n <= 2^24), one label each, C classes (1 .. 14), a radius r (1 .. 16384 half pixels, inclusive), P permutations
// (1 .. 1024) and a seed.  An ordered pair (i, j), i != j, is a contact when dx * dx + dy * dy <= r * r (coincident points are contacts).
// observed[a][b] counts the contacts with label_i = a and label_j = b, perm_counts[p - 1][a][b] the same under lab_p[i] = lab[pi_p(i)],
// class_n[c] the points of class c; a label outside 0 .. C - 1 is in no row and no column, but its row takes part in every shuffle.
// pi_p is a keyed six-round Feistel network on row numbers with cycle-walking (cellenrich_host.h), an exact function of (n, seed, p) on
// device and host alike.  Integer adds only: the result does not depend on the arrival order of any atomic and is bitwise the same on
// every call.
//
// Stages, all on the caller's stream:
//   geometry   on the HOST from the caller's bounding box (cell_grid_side of cellgrid_host.h): the cell side is the smallest multiple of
//              r whose grid has at most 2^22 cells.
//   binning    cellbin.h, ONE key per cell: the records come out sorted by cell.
//   zeroing    observed, perm_counts and class_n are zeroed by a kernel of this call AFTER the binning and only if the flag is clear, so
//              a point outside the stated box leaves every output untouched (NUHTC_E_INVALID).
//   batches    the permutations are worked off 16 at a time, two launches per batch:
//     shuffle  one thread per record POSITION: pi_p of the record's row for the (up to) 16 permutations of the batch, the round keys
//              computed on the host and passed as kernel arguments, and one uint64 per position holding the 16 shuffled classes as
//              nibbles, cs_class(labels[pi_p(rec.w)], C).  The words are in RECORD order, so the sweep reads word j beside recs[j].
//              The 16 cycle-walks of a thread are one loop over the applications of F (a walk that ends hands over to the next slot),
//              so a wave waits for the longest sum of 16 walks and not 16 times for the longest walk.
//     sweep    one thread per record in that order, 256 per workgroup, a grid-stride loop over the blocks of 256 records.  cell_sweep
//              of cellbin.h runs ONCE per query for the whole batch; for every contact the thread loads the neighbour's word and adds 1
//              per slot into the workgroup's LDS table [slot][a][b] (32-bit LDS atomics without return), a and b being the nibbles of
//              the query's and the neighbour's word.  The table has a row and a column for the class "none" (C), so the inner loop has
//              no branch; they are dropped when the table is flushed into the global int64 outputs (64-bit vector atomics, non-zero
//              entries only).  The first sweep carries the OBSERVED labels as a 17th slot (the record's own label words, which
//              cell_sweep has loaded anyway) and takes the class census; P = 16 is one sweep, P = 1000 is 63.
//
// Why the table and not private counters: a query has one class per slot but its neighbours have any, so private counting needs 16 x C
// counters per thread; nibble-parallel sums in registers need C masked compares of 64 bits per contact and a widening step every 15
// contacts.  The LDS table costs 16 adds per contact whatever C is.
//
// No counter can overflow for any accepted input (the budget is stated in cellenrich_host.h): a table entry is uint32 and a workgroup
// flushes at least every ce_flush_blocks(n) blocks, blocks x 256 x (n - 1) <= 2^32 - 1; the census of a workgroup counts its own queries
// (<= n <= 2^24); the outputs are int64 (<= n (n - 1) < 2^48).  70 000 coincident points put 4.9 x 10^9 contacts into four entries of
// every table and are counted exactly (tests/test_hip_enrichment.py).
//
// Measured on one MI355X (tools/bench_enrichment.py -> profiles/cell_enrichment.json; 500 000 centres on a 36 000-px square, r = 64 px,
// C = 5, medians of 10 calls).  P = 1000, 63 batches: 10.6 ms per call on the uniform set (5 contacts per nucleus; binning 0.07, shuffles
// 3.97, sweeps 6.46) and 32.2 ms on the clustered set (20 contacts per nucleus; shuffles 3.99, sweeps 27.9).  P = 16, one batch with the
// observed slot, the binning and the call's allocations and synchronisation: 0.75 and 1.15 ms, 1.4 x and 1.5 x nuhtc_cell_spatial with the
// single edge r on the same points (0.54 and 0.75 ms); every further batch adds 0.16 and 0.50 ms, 0.30 x and 0.67 x that call.  So the
// re-sweep per batch is not what costs: where contacts are many the time is the 16 LDS adds per contact (lanes of a wave meet on the few
// class pairs and serialise), where they are few the shuffle is 40 % of the call.  With the 16 walks of a thread as 16 separate loops the
// shuffles took 7.0 ms instead of 4.0.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, profiles/cell_enrichment_resources.txt): ce_sweep_kernel takes 31 VGPRs and 70
// SGPRs with the observed slot, 28 and 63 without, 15,376 / 15,300 B of static LDS and no scratch; ce_shuffle_kernel 16 VGPRs, 23 SGPRs,
// 384 B LDS, no scratch; ce_zero_kernel 6 and 16; registers allow 8 waves per SIMD in all of them.
//
// Everything that decides a value, an index or a limit -- the generator, the nibble packing, the table index, the flush interval
// (cellenrich_host.h), the grid geometry and the pair distance (cellgrid_host.h) -- is plain C++, and
// tools/dev/cellenrich_host_check.cpp runs exactly those functions on the host under -fsanitize=address,undefined.  The kernel code
// itself is not sanitized.
#include <algorithm>
#include <cstring>

#include "cellbin.h"
#include "cellenrich_host.h"

namespace {

struct CellEnrichArgs {
  CellBin b;                          // the points, the grid and the records in cell order
  int n, C, P, nblk;
  int r;                              // the radius
  int half_bits;                      // h of the generator
  int flush_blocks;                   // blocks of queries between two flushes of the LDS table
  uint32_t key[CE_BATCH][CE_ROUNDS];  // the round keys of the batch being launched
  unsigned long long* nib;            // [n] the shuffled classes of the batch, 16 nibbles per record position
  unsigned long long* observed;       // [C][C]
  unsigned long long* perm_counts;    // [P][C][C]
  unsigned long long* class_n;        // [C]
};

__global__ __launch_bounds__(256) void ce_zero_kernel(CellEnrichArgs a) {
  if (*a.b.flag) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.P * a.C * a.C) a.perm_counts[i] = 0;
  if (i < a.C * a.C) a.observed[i] = 0;
  if (i < a.C) a.class_n[i] = 0;
}

// the shuffled classes of `ns` permutations for every record position
__global__ __launch_bounds__(CE_NT) void ce_shuffle_kernel(CellEnrichArgs a, int ns) {
  __shared__ uint32_t key[CE_BATCH][CE_ROUNDS];          // in LDS: a lane reads the keys of ITS slot
  const CellBin& g = a.b;
  if (*g.flag) return;                                   // the records are incomplete: nothing is read from them (uniform)
  if (threadIdx.x < CE_BATCH * CE_ROUNDS) key[threadIdx.x / CE_ROUNDS][threadIdx.x % CE_ROUNDS] = a.key[threadIdx.x / CE_ROUNDS][threadIdx.x % CE_ROUNDS];
  __syncthreads();
  const int j = blockIdx.x * CE_NT + threadIdx.x;
  if (j >= a.n) return;
  const uint32_t row = (uint32_t)g.recs[j].w, n = (uint32_t)a.n;
  unsigned long long word = 0;
  if (n == 1) {
    for (int s = 0; s < ns; ++s) word = ce_pack(word, s, cs_class(g.labels[0], a.C));
  } else {
    // ce_permute for the slots one after the other, as ONE loop over the applications of F: a lane whose walk ends goes on to its next
    // slot at once, so the wave waits for the longest SUM of walks (about 2 ns + a few) and not ns times for the longest single walk
    int s = 0;
    uint32_t x = row;
    while (s < ns) {
      x = ce_feistel(x, a.half_bits, key[s]);
      if (x < n) {                                       // pi_p(row) for the slot's p
        word = ce_pack(word, s, cs_class(g.labels[x], a.C));
        ++s; x = row;
      }
    }
  }
  a.nib[j] = word;
}

// the workgroup's table into the outputs: the non-zero entries of the classes proper; the table is left cleared
template <bool OBS>
__device__ __forceinline__ void ce_flush(const CellEnrichArgs& a, unsigned* table, int first, int ns) {
  const int C = a.C, K = ce_slot_words(C);
  __syncthreads();
  for (int i = threadIdx.x; i < (OBS ? CE_BATCH + 1 : ns) * K; i += CE_NT) {
    const unsigned v = table[i];
    if (!v) continue;
    table[i] = 0;
    const int s = i / K, rem = i - s * K, ca = rem / (C + 1), cb = rem - ca * (C + 1);
    if (ca >= C || cb >= C) continue;
    if (OBS && s == CE_OBS_SLOT) atomicAdd(&a.observed[ca * C + cb], (unsigned long long)v);
    else atomicAdd(&a.perm_counts[((size_t)(first + s) * C + ca) * C + cb], (unsigned long long)v);        // s < ns: first + s < P
  }
  __syncthreads();
}

// the contacts of every query under the `ns` permutations from row `first` of perm_counts on; OBS: and under the observed labels
template <bool OBS>
__global__ __launch_bounds__(CE_NT) void ce_sweep_kernel(CellEnrichArgs a, int first, int ns) {
  __shared__ unsigned table[CE_TABLE_WORDS];
  __shared__ unsigned cn[16];
  const CellBin& g = a.b;
  if (*g.flag) return;                                   // the binning met a point outside the box: nothing is written (uniform)
  const int tid = threadIdx.x, C = a.C, K = ce_slot_words(C), r = a.r;
  for (int i = tid; i < CE_TABLE_WORDS; i += CE_NT) table[i] = 0;
  if (tid < 16) cn[tid] = 0;
  __syncthreads();
  int counted = 0;
  for (int blk = blockIdx.x; blk < a.nblk; blk += gridDim.x) {          // uniform over the workgroup: every thread meets every barrier
    const int q = blk * CE_NT + tid;
    if (q < a.n) {
      const int4 me = g.recs[q];
      const unsigned long long mine = a.nib[q];
      const int my_class = cs_class(me.z, C);
      if (OBS && my_class < C) atomicAdd(&cn[my_class], 1u);
      cell_sweep(g, me, r, [&](const int4& o) { return o.w != me.w; }, [&](int j, const int4& o, int) {
        unsigned long long m = mine, w = a.nib[j];
        int at = 0;
        for (int s = 0; s < ns; ++s) {
          atomicAdd(&table[at + (int)(m & 15u) * (C + 1) + (int)(w & 15u)], 1u);
          m >>= 4; w >>= 4; at += K;
        }
        if (OBS) atomicAdd(&table[ce_table_at(CE_OBS_SLOT, my_class, cs_class(o.z, C), C)], 1u);
      });
    }
    if (++counted == a.flush_blocks) {
      ce_flush<OBS>(a, table, first, ns);
      counted = 0;
    }
  }
  if (counted) ce_flush<OBS>(a, table, first, ns);
  if (OBS && tid < C && cn[tid]) atomicAdd(&a.class_n[tid], (unsigned long long)cn[tid]);
}

}  // namespace

extern "C" int nuhtc_enrichment_permutation(int64_t n, uint32_t seed, int p, int32_t* out) {
  return ce_fill_permutation(n, seed, p, out) ? 0 : NUHTC_E_INVALID;
}

extern "C" int nuhtc_cell_enrichment(int device, const int32_t* points, const int32_t* labels, int64_t n, int num_classes, int r, int num_perms,
                                     uint32_t seed, int x_min, int y_min, int x_max, int y_max, int64_t* observed, int64_t* perm_counts,
                                     int64_t* class_n, void* stream) {
  if (!ce_perms_ok(num_perms) || !cell_call_ok(n, CE_MAX_POINTS, num_classes, r, x_min, y_min, x_max, y_max)) return NUHTC_E_INVALID;
  if (!observed || !perm_counts || !class_n || (n > 0 && (!points || !labels))) return NUHTC_E_INVALID;
  if (hipSetDevice(device) != hipSuccess) return NUHTC_E_HIP;
  hipStream_t s = (hipStream_t)stream;
  const int C = num_classes, P = num_perms;
  if (n == 0) {
    if (hipMemsetAsync(observed, 0, (size_t)C * C * sizeof(int64_t), s) != hipSuccess ||
        hipMemsetAsync(perm_counts, 0, (size_t)P * C * C * sizeof(int64_t), s) != hipSuccess ||
        hipMemsetAsync(class_n, 0, C * sizeof(int64_t), s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      return NUHTC_E_HIP;
    return 0;
  }
  CellEnrichArgs a;
  memset(&a, 0, sizeof(a));
  a.n = (int)n; a.C = C; a.P = P; a.r = r; a.nblk = (int)((n + CE_NT - 1) / CE_NT);
  a.half_bits = n > 1 ? ce_half_bits((uint32_t)n) : 1;
  a.flush_blocks = ce_flush_blocks(n);
  a.observed = reinterpret_cast<unsigned long long*>(observed); a.perm_counts = reinterpret_cast<unsigned long long*>(perm_counts);
  a.class_n = reinterpret_cast<unsigned long long*>(class_n);
  DevScratch tmp;      // every temporary of the call, freed on the way out
  const int nchunk = cellbin_setup(a.b, points, labels, (int)n, x_min, y_min, x_max, y_max, r, CE_MAX_CELLS, 1, tmp, s);
  if (!nchunk) return NUHTC_E_HIP;
  a.nib = tmp.alloc<unsigned long long>((size_t)n * sizeof(unsigned long long));
  if (!tmp.ok()) return NUHTC_E_HIP;
  {
    ProfScope ps("cell_enrichment_bin", 0, 0, s);
    cellbin_launch(a.b, nchunk, s);
    hipLaunchKernelGGL(ce_zero_kernel, dim3((P * C * C + 255) / 256), dim3(256), 0, s, a);
  }
  const unsigned grid = (unsigned)std::min(a.nblk, 2048);
  for (int first = 0; first < P; first += CE_BATCH) {
    const int ns = std::min((int)CE_BATCH, P - first);
    for (int k = 0; k < ns; ++k) ce_keys(seed, (uint32_t)(first + k + 1), a.key[k]);
    {
      ProfScope ps("cell_enrichment_shuffle", 0, 0, s);
      hipLaunchKernelGGL(ce_shuffle_kernel, dim3((unsigned)a.nblk), dim3(CE_NT), 0, s, a, ns);
    }
    {
      ProfScope ps("cell_enrichment_sweep", 0, 0, s);
      if (first == 0) hipLaunchKernelGGL(ce_sweep_kernel<true>, dim3(grid), dim3(CE_NT), 0, s, a, first, ns);
      else hipLaunchKernelGGL(ce_sweep_kernel<false>, dim3(grid), dim3(CE_NT), 0, s, a, first, ns);
    }
  }
  return cellbin_finish(a.b, s);
}
