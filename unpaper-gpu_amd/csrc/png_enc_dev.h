// png_enc_dev.h — device-side pieces the lossless encoders' kernels share
// (kernels_png.hip, kernels_tiff_enc.hip): the staged row, the PngPages
// addressing, the histogram visitor and the bit writer.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "png_enc.h"
#include "png_enc_core.h"

namespace uph {
namespace pngenc {

// A staged row: the aligned dwords that hold it, read as bytes.
struct LdsRow {
  const uint8_t* p;
  __device__ uint32_t byte(int64_t i) const { return p[i]; }
};

// The byte that holds pixel 0 of row `row` of page p and the pixel's bit in it.
__device__ inline const uint8_t* row_start(const PngPages& pg, const Shape& s, int p, int row, int* bit) {
  const int sheet = p / pg.per_sheet;
  const int j = p - sheet * pg.per_sheet;
  const int plane = pg.cur ? (pg.cur[(int64_t)sheet * pg.cur_step] & 1) : 0;
  const int64_t px = (int64_t)pg.offset + (int64_t)j * pg.sheet_width / pg.per_sheet;
  const uint8_t* r = pg.plane[plane] + sheet * pg.sheet_stride + (int64_t)row * pg.pitch;
  if (s.depth == 8) {
    *bit = 0;
    return r + px * s.channels;
  }
  *bit = (int)(px & 7);
  return r + (px >> 3);
}

struct LdsHist {
  uint32_t* h;
  __device__ void literal(uint32_t b) { atomicAdd(h + b, 1u); }
  __device__ void match(int len, int dist) {
    int sym, eb;
    uint32_t ev;
    length_symbol(len, &sym, &eb, &ev);
    atomicAdd(h + sym, 1u);
    distance_symbol(dist, &sym, &eb, &ev);
    atomicAdd(h + kLL + sym, 1u);
  }
};

// Writes bits LSB first from bit `at` of the zeroed stream `out` on.  Words
// that lie wholly inside the lane's bits are stored; the first word and the
// last, partial one are shared with the neighbours and merged with atomicOr.
struct EmitSink {
  uint32_t* out;
  int64_t w;     // word being filled
  uint64_t acc;  // its bits and the next word's
  int n;         // bits in acc (the first word's bits before `at` count as zeros)
  bool first = true;
  __device__ EmitSink(uint32_t* o, int64_t at) : out(o), w(at >> 5), acc(0), n((int)(at & 31)) {}
  __device__ void put(uint32_t bits, int len) {
    acc |= (uint64_t)bits << n;
    n += len;
    if (n >= 32) {
      if (first)
        atomicOr(out + w, (uint32_t)acc);
      else
        out[w] = (uint32_t)acc;
      first = false;
      w++;
      acc >>= 32;
      n -= 32;
    }
  }
  __device__ void finish() {
    if (n > 0) atomicOr(out + w, (uint32_t)acc);
  }
};

}  // namespace pngenc
}  // namespace uph
