// The front of the per-nucleus measurements for nuclei that come from a WRITTEN GeoJSON (nuhtc_amd/ringfeat.py, tools/wsi_feat_extract.py)
// instead of a detection run (gfx950): rings -> bit masks and slide pixels -> frames, in the layout nuhtc_op_nucleus_morph and
// nuhtc_op_nucleus_texture read with K = 1.  A nucleus has a square frame of side S (32, 64, 128 or 256) at a slide position `origin`.
//
// ring_fill_kernel: one workgroup of 256 threads per ring, two bitmaps of the frame in LDS (S * S / 32 words each: 16 KB at S = 256).
//   1. every vertex is moved into the frame and tested (inside the frame; the edge to the next vertex along one of the eight chain
//      directions); a ring that fails leaves a zero mask and its status, and nothing else;
//   2. the border is drawn by integer steps along every edge, one thread per edge, one LDS atomicOr per pixel;
//   3. the outside is seeded with the pixels of the frame's rim that are not border -- they are 4-neighbours of the pixels beyond the
//      frame, which are all outside -- and grown to its closure under "a free 4-neighbour of an outside pixel is outside" by sweeps:
//        V  one thread per word column walks the rows down and then up: outside(row) <- fill(outside(row) | outside(row before)) & ~border,
//           fill = the horizontal flood inside the 32-bit word (two Kogge-Stone fills, five steps each);
//        H  (S > 32) one thread per row walks the words right and then left with the same fill, the end bit of a word carried into the next.
//      A thread of either phase reads and writes only its own column / row and a barrier separates the phases: no word is ever read
//      while another thread writes it.  The block-wide "changed" flag is __syncthreads_or.  A sweep that changes nothing has seen a
//      fixed point; every other sweep adds a pixel, so S * S sweeps bound the loop whatever the input.  The closure is unique: the
//      mask does not depend on the order in which pixels were reached.  A convex nucleus takes one productive sweep and the empty one.
//   4. the mask is everything that is not outside: the pixels inside or on the border, i.e. the set nuhtc_fill_rings (geojson.hip)
//      computes on the host with a byte grid and a stack -- that code is the definition.  Plain vector stores.
//
// frame_gather_kernel: frames[i] = the S x S x 3 bytes of a device-resident slide block at origin[i], zeros where the frame leaves the
// block.  A thread assembles four consecutive bytes of a frame (the source has any alignment: byte loads) and stores one aligned word.
#include "common.h"

namespace {

struct RingFillParams {
  const int32_t* verts;      // [nv][2] slide pixels
  const int64_t* ring_off;   // [n + 1]
  const int32_t* origin;     // [n][2] slide position of the frame's pixel (0, 0)
  long long nv;
  int S;
  uint32_t* masks;           // [n][S][S / 32]
  int32_t* status;           // [n]
};

// flood of the seed bits `o` through the free bits `f` inside one word, both directions (o is a subset of f)
__device__ __forceinline__ unsigned word_fill(unsigned o, unsigned f) {
  unsigned g = o, p = f;
  g |= p & (g << 1); p &= p << 1;
  g |= p & (g << 2); p &= p << 2;
  g |= p & (g << 4); p &= p << 4;
  g |= p & (g << 8); p &= p << 8;
  g |= p & (g << 16);
  p = f;
  g |= p & (g >> 1); p &= p >> 1;
  g |= p & (g >> 2); p &= p >> 2;
  g |= p & (g >> 4); p &= p >> 4;
  g |= p & (g >> 8); p &= p >> 8;
  g |= p & (g >> 16);
  return g;
}

constexpr int RING_MAX_WORDS = 256 * 256 / 32;

__global__ __launch_bounds__(256) void ring_fill_kernel(RingFillParams p) {
  __shared__ unsigned border[RING_MAX_WORDS], outside[RING_MAX_WORDS];
  const int i = blockIdx.x, tid = threadIdx.x, S = p.S, W = S >> 5, words = S * W;
  uint32_t* __restrict__ out = p.masks + (size_t)i * words;
  long long a = p.ring_off[i], b = p.ring_off[i + 1];
  const bool listed = a >= 0 && b > a && b <= p.nv;       // a ring has a vertex, and its vertices are inside the array
  if (!listed) { a = 0; b = 0; }
  const long long ox = p.origin[2 * i], oy = p.origin[2 * i + 1];
  for (int w = tid; w < words; w += 256) border[w] = 0;
  // ---- 1. the vertices and edges
  int bad = 0;
  for (long long v = a + tid; v < b; v += 256) {
    const long long nx = v + 1 < b ? v + 1 : a;
    const long long x = (long long)p.verts[2 * v] - ox, y = (long long)p.verts[2 * v + 1] - oy;
    const long long dx = (long long)p.verts[2 * nx] - ox - x, dy = (long long)p.verts[2 * nx + 1] - oy - y;
    if (x < 0 || x >= S || y < 0 || y >= S) bad |= 1;
    if (dx != 0 && dy != 0 && (dx < 0 ? -dx : dx) != (dy < 0 ? -dy : dy)) bad |= 2;
  }
  const int outside_frame = __syncthreads_or(bad & 1);    // (also: border[] is zero)
  const int off_chain = __syncthreads_or(bad & 2);
  const int st = outside_frame ? 1 : (off_chain || !listed) ? 2 : 0;
  if (st) {
    for (int w = tid; w < words; w += 256) out[w] = 0;
    if (tid == 0) p.status[i] = st;
    return;
  }
  // ---- 2. the border: every vertex is inside the frame and every edge runs along a chain direction, so every step stays inside
  for (long long v = a + tid; v < b; v += 256) {
    const long long nx = v + 1 < b ? v + 1 : a;
    int x = (int)(p.verts[2 * v] - ox), y = (int)(p.verts[2 * v + 1] - oy);
    const int ex = (int)(p.verts[2 * nx] - ox), ey = (int)(p.verts[2 * nx + 1] - oy);
    const int sx = (ex > x) - (ex < x), sy = (ey > y) - (ey < y);
    const int steps = max(abs(ex - x), abs(ey - y));      // < S
    for (int k = 0; k <= steps; ++k) {
      atomicOr(&border[y * W + (x >> 5)], 1u << (x & 31));
      x += sx; y += sy;
    }
  }
  __syncthreads();
  // ---- 3. the outside: the rim's free pixels, then the sweeps
  for (int w = tid; w < words; w += 256) {
    const int y = w / W, k = w - y * W;
    unsigned rim = (y == 0 || y == S - 1) ? ~0u : 0u;
    if (k == 0) rim |= 1u;
    if (k == W - 1) rim |= 1u << 31;
    outside[w] = rim & ~border[w];
  }
  __syncthreads();
  for (int sweep = 0; sweep < S * S; ++sweep) {
    int changed = 0;
    if (tid < W) {                                        // V: column tid, down and up
      unsigned prev = 0;
      for (int y = 0; y < S; ++y) {
        const int w = y * W + tid;
        const unsigned f = ~border[w], o = outside[w], g = word_fill((o | prev) & f, f);
        if (g != o) { outside[w] = g; changed = 1; }
        prev = g;
      }
      prev = 0;
      for (int y = S - 1; y >= 0; --y) {
        const int w = y * W + tid;
        const unsigned f = ~border[w], o = outside[w], g = word_fill((o | prev) & f, f);
        if (g != o) { outside[w] = g; changed = 1; }
        prev = g;
      }
    }
    if (W > 1) {
      __syncthreads();
      if (tid < S) {                                      // H: row tid, right and left
        unsigned carry = 0;
        for (int k = 0; k < W; ++k) {
          const int w = tid * W + k;
          const unsigned f = ~border[w], o = outside[w], g = word_fill((o | carry) & f, f);
          if (g != o) { outside[w] = g; changed = 1; }
          carry = g >> 31;
        }
        carry = 0;
        for (int k = W - 1; k >= 0; --k) {
          const int w = tid * W + k;
          const unsigned f = ~border[w], o = outside[w], g = word_fill((o | carry) & f, f);
          if (g != o) { outside[w] = g; changed = 1; }
          carry = (g & 1u) << 31;
        }
      }
    }
    if (!__syncthreads_or(changed)) break;
  }
  // ---- 4. inside or on the border = not outside
  for (int w = tid; w < words; w += 256) out[w] = ~outside[w];
  if (tid == 0) p.status[i] = 0;
}

struct FrameGatherParams {
  const uint8_t* block;      // [bh][bw][3]
  const int32_t* origin;     // [n][2]
  int bh, bw, bx, by, S;
  uint32_t* frames;          // [n][S][S][3] bytes, as words
};

__global__ __launch_bounds__(256) void frame_gather_kernel(FrameGatherParams p) {
  const int i = blockIdx.x, S = p.S, row_bytes = S * 3, words = S * row_bytes / 4;
  const long long x0 = (long long)p.origin[2 * i] - p.bx, y0 = (long long)p.origin[2 * i + 1] - p.by;   // the frame's corner in the block
  uint32_t* __restrict__ dst = p.frames + (size_t)i * words;
  for (int w = blockIdx.y * 256 + threadIdx.x; w < words; w += gridDim.y * 256) {
    const int byte = w * 4, r = byte / row_bytes, c = byte - r * row_bytes;      // row_bytes is a multiple of 4: a word stays in its row
    const long long y = y0 + r;
    unsigned v = 0;
    if (y >= 0 && y < p.bh) {
      const uint8_t* __restrict__ src = p.block + y * p.bw * 3;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const long long at = x0 * 3 + c + t;              // byte of the block's row: pixel at / 3
        if (at >= 0 && at < (long long)p.bw * 3) v |= (unsigned)src[at] << (8 * t);
      }
    }
    dst[w] = v;
  }
}

bool frame_side_ok(int S) { return S == 32 || S == 64 || S == 128 || S == 256; }

}  // namespace

extern "C" {

int nuhtc_op_ring_fill(int device, const int32_t* verts, int64_t nv, const int64_t* ring_off, const int32_t* origin, int n, int S,
                       uint32_t* masks, int32_t* status, void* stream) {
  if (!verts || !ring_off || !origin || !masks || !status || nv < 1 || n < 1 || n > 4096 || !frame_side_ok(S)) return NUHTC_E_INVALID;
  if (hipSetDevice(device) != hipSuccess) return NUHTC_E_HIP;
  hipStream_t s = (hipStream_t)stream;
  RingFillParams p{verts, ring_off, origin, (long long)nv, S, masks, status};
  ProfScope ps("ring_fill", 0, 0, s);
  hipLaunchKernelGGL(ring_fill_kernel, dim3((unsigned)n), dim3(256), 0, s, p);
  return launched() ? 0 : NUHTC_E_HIP;
}

int nuhtc_op_frame_gather(int device, const uint8_t* block, int bh, int bw, int bx, int by, const int32_t* origin, int n, int S,
                          uint8_t* frames, void* stream) {
  if (!block || !origin || !frames || bh < 1 || bw < 1 || bh > 32768 || bw > 32768 || n < 1 || n > 4096 || !frame_side_ok(S)) return NUHTC_E_INVALID;
  if (hipSetDevice(device) != hipSuccess) return NUHTC_E_HIP;
  hipStream_t s = (hipStream_t)stream;
  FrameGatherParams p{block, origin, bh, bw, bx, by, S, (uint32_t*)frames};
  const int words = S * S * 3 / 4;
  ProfScope ps("frame_gather", 0, (double)n * words * 8, s);
  hipLaunchKernelGGL(frame_gather_kernel, dim3((unsigned)n, (unsigned)cdiv(words, 1024)), dim3(256), 0, s, p);
  return launched() ? 0 : NUHTC_E_HIP;
}

}  // extern "C"
