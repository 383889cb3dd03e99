/* g4_row.h — one row of CCITT Group 4 (ITU-T T.6) coding, shared by the host
 * encoder (ccitt.cpp) and the device kernels (kernels_g4.hip) so that both
 * produce the same bits.
 *
 * A row is read through an accessor R with
 *     uint32_t word(int i)   32 pixels, the first in the MSB, 1 = black
 *     int      off           bit of word(0) that holds pixel 0 (>= 0)
 * and only bits [off, off + W) are taken as pixels.  The codes go to a sink S
 * with put(uint32_t code, int len) (len <= 13, the code right-aligned): a
 * counting sink sizes a row, an emitting sink writes it.
 *
 * T.6 2.2: with a0 the reference element (before the row at first, on an
 * imaginary white pixel), a1 / a2 the next changes of the coding row and
 * b1 / b2 those of the reference row (b1 the first change right of a0 to the
 * colour a1 changes to),
 *     b2 < a1        pass mode        0001, a0 = b2
 *     |a1 - b1| <= 3 vertical mode    1 / 011 / 000011 / 0000011 / 010 / ..
 *     else           horizontal mode  001 + M(a0a1) + M(a1a2), a0 = a2
 * where M is the T.4 run code of the run's colour: make-up codes (the 2560
 * one repeated for runs >= 2624) then always a terminating code.  Rows follow
 * one another with nothing between them; EOFB (two EOLs) ends the page.
 */
#ifndef UNPAPER_HIP_G4_ROW_H
#define UNPAPER_HIP_G4_ROW_H

#include <stdint.h>

#ifdef __HIPCC__
#define G4_FN __host__ __device__ static inline
#define G4_MEMBER __host__ __device__
#else
#define G4_FN static inline
#define G4_MEMBER
#endif

namespace uph {
namespace g4 {

constexpr int kRunCodes = 104;  // 0..63 terminating, 64 + k: make-up of 64 * (k + 1)
constexpr int kEofbBits = 24;   // 000000000001 twice
constexpr uint32_t kEol = 0x001;
constexpr int kEolBits = 12;

/* T.4 Tables 2 and 3 and the extended make-ups 1792..2560 (both colours):
 * code << 4 | length, [0] white, [1] black. */
constexpr uint32_t kRun[2][kRunCodes] = {
    {
        0x00358, 0x00076, 0x00074, 0x00084, 0x000B4, 0x000C4, 0x000E4, 0x000F4,
        0x00135, 0x00145, 0x00075, 0x00085, 0x00086, 0x00036, 0x00346, 0x00356,
        0x002A6, 0x002B6, 0x00277, 0x000C7, 0x00087, 0x00177, 0x00037, 0x00047,
        0x00287, 0x002B7, 0x00137, 0x00247, 0x00187, 0x00028, 0x00038, 0x001A8,
        0x001B8, 0x00128, 0x00138, 0x00148, 0x00158, 0x00168, 0x00178, 0x00288,
        0x00298, 0x002A8, 0x002B8, 0x002C8, 0x002D8, 0x00048, 0x00058, 0x000A8,
        0x000B8, 0x00528, 0x00538, 0x00548, 0x00558, 0x00248, 0x00258, 0x00588,
        0x00598, 0x005A8, 0x005B8, 0x004A8, 0x004B8, 0x00328, 0x00338, 0x00348,
        0x001B5, 0x00125, 0x00176, 0x00377, 0x00368, 0x00378, 0x00648, 0x00658,
        0x00688, 0x00678, 0x00CC9, 0x00CD9, 0x00D29, 0x00D39, 0x00D49, 0x00D59,
        0x00D69, 0x00D79, 0x00D89, 0x00D99, 0x00DA9, 0x00DB9, 0x00989, 0x00999,
        0x009A9, 0x00186, 0x009B9, 0x0008B, 0x000CB, 0x000DB, 0x0012C, 0x0013C,
        0x0014C, 0x0015C, 0x0016C, 0x0017C, 0x001CC, 0x001DC, 0x001EC, 0x001FC,
    },
    {
        0x0037A, 0x00023, 0x00032, 0x00022, 0x00033, 0x00034, 0x00024, 0x00035,
        0x00056, 0x00046, 0x00047, 0x00057, 0x00077, 0x00048, 0x00078, 0x00189,
        0x0017A, 0x0018A, 0x0008A, 0x0067B, 0x0068B, 0x006CB, 0x0037B, 0x0028B,
        0x0017B, 0x0018B, 0x00CAC, 0x00CBC, 0x00CCC, 0x00CDC, 0x0068C, 0x0069C,
        0x006AC, 0x006BC, 0x00D2C, 0x00D3C, 0x00D4C, 0x00D5C, 0x00D6C, 0x00D7C,
        0x006CC, 0x006DC, 0x00DAC, 0x00DBC, 0x0054C, 0x0055C, 0x0056C, 0x0057C,
        0x0064C, 0x0065C, 0x0052C, 0x0053C, 0x0024C, 0x0037C, 0x0038C, 0x0027C,
        0x0028C, 0x0058C, 0x0059C, 0x002BC, 0x002CC, 0x005AC, 0x0066C, 0x0067C,
        0x000FA, 0x00C8C, 0x00C9C, 0x005BC, 0x0033C, 0x0034C, 0x0035C, 0x006CD,
        0x006DD, 0x004AD, 0x004BD, 0x004CD, 0x004DD, 0x0072D, 0x0073D, 0x0074D,
        0x0075D, 0x0076D, 0x0077D, 0x0052D, 0x0053D, 0x0054D, 0x0055D, 0x005AD,
        0x005BD, 0x0064D, 0x0065D, 0x0008B, 0x000CB, 0x000DB, 0x0012C, 0x0013C,
        0x0014C, 0x0015C, 0x0016C, 0x0017C, 0x001CC, 0x001DC, 0x001EC, 0x001FC,
    },
};

/* The first x' in [x, W] whose pixel is not `colour` (W when the run of
 * `colour` that starts at x reaches the row's end).  x <= W. */
template <class R>
G4_FN int32_t run_end(const R& row, int32_t x, int32_t W, int colour) {
  const int32_t end = row.off + W;
  int32_t pos = row.off + x;
  if (pos >= end) return W;
  const uint32_t flip = colour ? 0xFFFFFFFFu : 0u;  // a 1 where the pixel differs from `colour`
  int32_t i = pos >> 5;
  uint32_t v = (row.word(i) ^ flip) & (0xFFFFFFFFu >> (pos & 31));
  for (;;) {
    if (v) {
      pos = (i << 5) + __builtin_clz(v);
      return (pos < end ? pos : end) - row.off;
    }
    i++;
    if ((i << 5) >= end) return W;
    v = row.word(i) ^ flip;
  }
}

/* The run code of `run` pixels of `colour`; `tab` is kRun or a copy of it. */
template <class S>
G4_FN void put_run(S& sink, const uint32_t (*tab)[kRunCodes], int colour, int32_t run) {
  const uint32_t* t = tab[colour];
  while (run >= 2624) {
    sink.put(t[63 + 40] >> 4, (int)(t[63 + 40] & 15));
    run -= 2560;
  }
  if (run >= 64) {
    const uint32_t m = t[63 + (run >> 6)];
    sink.put(m >> 4, (int)(m & 15));
    run &= 63;
  }
  sink.put(t[run] >> 4, (int)(t[run] & 15));
}

/* Codes row `cur` (W pixels) against the row above it, `ref`. */
template <class R, class S>
G4_FN void encode_row(const R& cur, const R& ref, int32_t W, const uint32_t (*tab)[kRunCodes], S& sink) {
  int colour = 0;  // of a0: the imaginary pixel before the row is white
  int32_t a0 = 0;  // stands for -1 until the first code: the first run counts from x = 0
  int32_t a1 = run_end(cur, 0, W, 0);
  int32_t b1 = run_end(ref, 0, W, 0);  // a black pixel at x = 0 is a change
  for (;;) {
    const int32_t b2 = b1 < W ? run_end(ref, b1, W, colour ^ 1) : W;
    if (b2 < a1) {
      sink.put(0x1, 4);  // pass
      a0 = b2;
    } else {
      const int32_t d = a1 - b1;
      if (d >= -3 && d <= 3) {
        /* V0 1; VR1 011, VR2 000011, VR3 0000011 (a1 right of b1); VL the
         * same with a last bit 0 */
        const int32_t ad = d < 0 ? -d : d;
        sink.put(d == 0 ? 0x1 : d > 0 ? 0x3 : 0x2, ad == 0 ? 1 : ad == 1 ? 3 : ad + 4);
        a0 = a1;
        colour ^= 1;
      } else {
        const int32_t a2 = a1 < W ? run_end(cur, a1, W, colour ^ 1) : W;
        sink.put(0x1, 3);  // horizontal
        put_run(sink, tab, colour, a1 - a0);
        put_run(sink, tab, colour ^ 1, a2 - a1);
        a0 = a2;
      }
    }
    if (a0 >= W) return;
    a1 = run_end(cur, a0, W, colour);
    /* past the reference pixels of the other colour at a0, then past the run
     * of a0's colour: the first change right of a0 to the other colour */
    b1 = run_end(ref, a0, W, colour ^ 1);
    b1 = run_end(ref, b1, W, colour);
  }
}

struct CountSink {
  int64_t bits = 0;
  G4_MEMBER void put(uint32_t, int len) { bits += len; }
};

}  // namespace g4
}  // namespace uph

#endif
