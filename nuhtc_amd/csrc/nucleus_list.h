// What the three per-nucleus kernels share (nucfeat.hip, nucmorph.hip, nuctex.hip: one workgroup per entry of a list of kept detections,
// each under that detection's final mask): the parts of their parameter blocks, the limits of the entry points that read tile pixels,
// the resolution of a list entry on the device and the fillers of the two host routes.  The structs and nucleus_sizes_error are plain
// C++, so a host program can exercise them under a sanitizer (tools/dev/nucmorph_host_check.cpp, nuctex_host_check.cpp); the rest is
// for hipcc.
#pragma once
#include <cstdint>
#include <string>

#if defined(__HIPCC__)
#include "engine.h"
#include "haematoxylin.h"
#endif

enum { NUCLEUS_MAX_SIDE = 1024 };

struct NucleusList {
  const int64_t* idx;      // entry d = tile * K + slot (idx_dev of nuhtc_export_kept) ...
  const int32_t* pairs;    // ... or, when idx is null, (tile, slot) at pairs[2 d]
  const int32_t* n_dev;    // entries = min(*n_dev, n_max); null: n_max
  int n_max, B, K;
};
struct NucleusMasks {
  const uint32_t* masks;   // [B][K][H][wpr], bit x & 31 of word x >> 5
  int H, W, wpr;
};
struct NucleusTiles {
  const uint8_t* tiles;    // [B][H][pitch][3]
  const int32_t* lut;      // [256]
  int kb[3];               // the coefficient of byte 0, 1, 2 of a pixel (channel_mode resolved on the host)
  int pitch;               // pixels per tile row (>= W)
};

// what is wrong with the sizes of a call that reads tile pixels (`what`: nucleus_morph, nucleus_texture), or empty.  The frame side is
// bounded by the per-row extents the morphometry keeps (NUCLEUS_MAX_SIDE entries, 16 bits a coordinate; a full frame holds 1024 x 1023
// pairs an offset: every texture count fits an int32); pitch = pixels per tile row (>= W).
inline std::string nucleus_sizes_error(const char* what, int B, int K, int H, int W, int pitch, int n_max, int channel_mode) {
  const char* why = nullptr;
  if (B < 1 || B > 4096 || K < 1 || K > 65536) why = ": B 1..4096, K 1..65536";
  else if (H < 1 || H > NUCLEUS_MAX_SIDE || W < 1 || W > NUCLEUS_MAX_SIDE || pitch < W || pitch > NUCLEUS_MAX_SIDE) why = ": H and W 1..1024, row pitch W..1024";
  else if (n_max < 1 || n_max > (1 << 24)) why = ": n_max 1..2^24";
  else if (channel_mode != 0 && channel_mode != 1) why = ": channel_mode is NUHTC_CH_AS_IS or NUHTC_CH_SWAP";
  return why ? std::string(what) + why : std::string();
}

#if defined(__HIPCC__)
// ---- device: entry d of the list -> (tile b, slot r)
enum NucleusEntry {
  NUCLEUS_PAST,      // d is past the count: the row is not written
  NUCLEUS_OUTSIDE,   // (b, r) is outside the batch: the caller writes its zero row and reads nothing
  NUCLEUS_REAL
};
__device__ __forceinline__ NucleusEntry nucleus_entry(const NucleusList& l, int d, long long& b, long long& r) {
  const int n = l.n_dev ? min(*l.n_dev, l.n_max) : l.n_max;
  if (d >= n) return NUCLEUS_PAST;
  if (l.idx) { const long long i = l.idx[d]; b = i / l.K; r = i - b * l.K; }
  else { b = l.pairs[2 * d]; r = l.pairs[2 * d + 1]; }
  return b < 0 || b >= l.B || r < 0 || r >= l.K ? NUCLEUS_OUTSIDE : NUCLEUS_REAL;
}
__device__ __forceinline__ const uint32_t* nucleus_mask(const NucleusMasks& m, int K, long long b, long long r) {
  return m.masks + (b * K + r) * (long long)m.H * m.wpr;
}
// the bits of a row's last word that are pixels (the readers of tile pixels mask the padding bits off on every read)
__device__ __forceinline__ unsigned nucleus_last_word(const NucleusMasks& m) { return (m.W & 31) ? (1u << (m.W & 31)) - 1u : ~0u; }
__device__ __forceinline__ const uint8_t* nucleus_tile(const NucleusTiles& t, int H, long long b) { return t.tiles + b * (long long)H * t.pitch * 3; }

// ---- host, engine route: the list nuhtc_export_kept wrote, the masks of `dets`, the frame of e->cfg.  `name`: the entry point, `verb`:
// what it does under a detection; own_ok: the caller's own pointers and counts are good.
inline int nucleus_engine_route(nuhtc_engine* e, const char* name, const char* verb, const nuhtc_dets* dets, int B, const int64_t* idx_dev,
                                const int32_t* n_dev, int cap, bool own_ok, NucleusList& l, NucleusMasks& m) {
  if (!e) return NUHTC_E_INVALID;
  if (!e->finalized) FAIL(e, NUHTC_E_STATE, std::string(name) + " before nuhtc_finalize");
  if (e->cfg.features_only) FAIL(e, NUHTC_E_STATE, std::string("this engine was created with features_only = 1: it has no detections to ") + verb);
  if (!dets || !dets->masks || !idx_dev || !n_dev || !own_ok || B > e->cfg.max_batch) FAIL(e, NUHTC_E_INVALID, std::string("bad ") + name + " arguments");
  const nuhtc_config& c = e->cfg;
  l = NucleusList{idx_dev, nullptr, n_dev, cap, B, c.max_per_img};
  m = NucleusMasks{dets->masks, c.tile_h, c.tile_w, c.tile_w / 32};
  return 0;
}
// ---- host, op route: raw arrays (the caller has tested its pointers and, for the pool, its own wider limits)
inline void nucleus_op_route(int B, const uint32_t* masks, int K, int H, int W, const int32_t* pairs_dev, const int32_t* n_dev, int n_max,
                             NucleusList& l, NucleusMasks& m) {
  l = NucleusList{nullptr, pairs_dev, n_dev, n_max, B, K};
  m = NucleusMasks{masks, H, W, (W + 31) / 32};
}
// ---- both routes of the two kernels that read tile pixels (rows of W pixels): the limits of the filled list and masks, then the tiles
inline int nucleus_tiles_args(nuhtc_engine* e, const char* what, const NucleusList& l, const NucleusMasks& m, const uint8_t* tiles, int channel_mode,
                              const int32_t* lut_dev, const int32_t k[3], NucleusTiles& t) {
  const std::string why = nucleus_sizes_error(what, l.B, l.K, m.H, m.W, m.W, l.n_max, channel_mode);
  if (!why.empty()) FAIL(e, NUHTC_E_INVALID, why);
  t.tiles = tiles; t.lut = lut_dev; t.pitch = m.W;
  haematoxylin_byte_coefficients(t.kb, k, channel_mode);
  return 0;
}
#endif
