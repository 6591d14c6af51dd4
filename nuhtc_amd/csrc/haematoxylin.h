// The fixed-point haematoxylin value of a tile pixel, shared by the per-nucleus kernels that read the tile under a mask (nucmorph.hip: its
// 256-bin histogram; nuctex.hip: its 16 grey levels).  nuhtc_amd/nucmorph.py (`haematoxylin`, `stain_constants`) defines it and builds the
// table and the coefficients: h = clamp((kb0 L[byte 0] + kb1 L[byte 1] + kb2 L[byte 2] + 2^27) >> 28, 0, 255) in int64 with a floor shift.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/nuhtc_hip.h"

constexpr int HEM_FIX_SHIFT = 28;     // 2^16 of the table times 2^12 of the coefficients

// px: the three bytes of the pixel; lut: the table (256 ints, LDS or global); kb: the coefficient of byte 0, 1, 2
__device__ __forceinline__ int haematoxylin_value(const uint8_t* __restrict__ px, const int* lut, long long kb0, long long kb1, long long kb2) {
  const long long acc = kb0 * lut[px[0]] + kb1 * lut[px[1]] + kb2 * lut[px[2]] + (1ll << (HEM_FIX_SHIFT - 1));
  return (int)min(max(acc >> HEM_FIX_SHIFT, 0ll), 255ll);
}

// byte c of a pixel is red (k[0]), green or blue: the mapping of patch_embed_tiles_kernel (swin.hip), where NUHTC_CH_SWAP reads network
// channel c (0 = red) from byte 2 - c
inline void haematoxylin_byte_coefficients(int kb[3], const int32_t k[3], int channel_mode) {
  for (int c = 0; c < 3; ++c) kb[channel_mode == NUHTC_CH_SWAP ? 2 - c : c] = k[c];
}
