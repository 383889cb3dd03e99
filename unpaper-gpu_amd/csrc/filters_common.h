// filters_common.h — what the filter and decode kernel files share.
#pragma once

#include "filters.h"

namespace uph {

template <int FMT>
__device__ __forceinline__ void white_px(uint8_t* row, int32_t x) {
  store_px_row<FMT>(row, x, Px{255, 255, 255});
}

// Dark bits (byte < t) of 32 gray bytes (eight dwords) as one word, bit
// 4 d + q = byte q of dword d.  Per dword: 16-bit SWAR lanes hold
// (0x100 + t - 1) - byte, whose bit 8 is (byte < t) with nothing above it, so
// one byte permute gathers the four flags as bytes of 0 or 1; the eight
// dwords' flag bytes are stacked (bit 8 q + d), and four delta swaps
// transpose that 4 x 8 bit matrix into pixel order.
__device__ __forceinline__ uint32_t dark_bits32(const uint32_t (&w)[8], uint32_t white) {
  const uint32_t K = (0x100u + white - 1u) * 0x00010001u;
  uint32_t g = 0;
#pragma unroll
  for (int d = 0; d < 8; d++) {
    const uint32_t lo = K - (w[d] & 0x00FF00FFu);          // bits 8, 24: bytes 0, 2
    const uint32_t hi = K - ((w[d] >> 8) & 0x00FF00FFu);   // bits 8, 24: bytes 1, 3
    g |= __builtin_amdgcn_perm(hi, lo, 0x07030501u) << d;  // bytes: flags of bytes 0..3
  }
  auto dswap = [](uint32_t x, uint32_t m, int delta) {
    const uint32_t t = ((x >> delta) ^ x) & m;
    return x ^ t ^ (t << delta);
  };
  g = dswap(g, 0x0000F0F0u, 12);
  g = dswap(g, 0x00CC00CCu, 6);
  g = dswap(g, 0x0A0A0A0Au, 3);
  return dswap(g, 0x22222222u, 1);
}

}  // namespace uph
