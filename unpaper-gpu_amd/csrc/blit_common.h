// blit_common.h — what the blit, move and rotate kernel files share.
#pragma once

#include "common.h"

namespace uph {

constexpr int kThreads = 256;

// Raw byte copy of one pixel (keeps Y400A alpha, as memcpy paths do).
template <int FMT>
__device__ __forceinline__ void copy_px_raw(uint8_t* drow, int32_t dx, const uint8_t* srow,
                                            int32_t sx) {
  constexpr int B = FMT == F_GRAY8 ? 1 : FMT == F_Y400A ? 2 : 3;
#pragma unroll
  for (int k = 0; k < B; k++) drow[dx * B + k] = srow[sx * B + k];
}

}  // namespace uph
