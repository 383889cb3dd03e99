/* tiff_strip.h — the decoder of one TIFF strip and the finishing of its rows,
 * shared by the host reader (tiff.cpp) and the device kernels
 * (kernels_tiff.hip) so that both give the same bytes and take the same
 * bounds checks: the host twin under ASan is the check of the device's.
 *
 * A strip is `in[0, n)`; it decodes to exactly `cap` bytes at `out` (the
 * strip's rows times the stored row bytes).  Every read of `in`, every table
 * index and every write of `out` is checked here; an error returns a status
 * (Status) and writes nothing more.
 *
 * PackBits (Compression 32773).  A header byte h (signed): 0..127 copies the
 * next h + 1 bytes, -127..-1 repeats the next byte 1 - h times, -128 does
 * nothing.  A literal or run that would pass the end of `in` or of `out` is an
 * error (kInput, kOutput), as is input that ends before `cap` bytes (kInput).
 *
 * LZW (Compression 5, the post-6.0 form).  Codes are read MSB first, 9 bits
 * wide at the start and after a Clear.  256 is Clear, 257 EOI, the first free
 * code 258.  The width grows one code early: to 10 bits when the next free
 * code is 511, to 11 at 1023, to 12 at 2047; with 4096 codes the table takes
 * no more.  A Clear may come at any point; the code after it must be a byte
 * (else kCode).  The strip ends when `cap` bytes are out (a string that would
 * pass `cap` is cut there) or at EOI; EOI, or the end of `in`, before `cap`
 * bytes is an error (kShort, kInput).  A code above the next free code is
 * kCode.  The old LSB-first form (first byte 0, second byte with bit 0 set,
 * libtiff's test) is refused as kOldLzw.
 *
 * LZW table.  Every dictionary string is a substring of the output already
 * written: the entry made after decoding a code is the previous code's string
 * plus one byte, and it lies where the previous string was written.  An entry
 * is (pos, len), positions relative to `out`, and decoding a code is a forward
 * byte copy from out[pos].  A code equal to the next free code is the same
 * copy from the previous string's position with its length + 1; that copy
 * overlaps its destination by one byte, which a forward copy gets right.
 * P is uint16_t for strips of at most 65,536 bytes (2 x 2 x 4096 bytes of
 * table), uint32_t beyond.  No entry that is used is longer than cap - 1.
 *
 * Row finishing, on the decoded bytes of one row:
 *   Predictor 2   running sum mod 256 along the row, stride = samples per
 *                 pixel; 8-bit samples only;
 *   FillOrder 2   1-bit data only.  libtiff (and so PIL) reverses the bits of a
 *                 strip's bytes before they are decoded, whatever the coder;
 *                 the callers do that to a compressed strip's input.  Only
 *                 for uncompressed rows is it a row operation: every byte
 *                 bit-reversed;
 *   MinIsWhite    8-bit gray v -> 255 - v (an extra sample is left as it is);
 *   palette       index -> the high bytes of its ColorMap entry, RGB24.
 */
#ifndef UNPAPER_HIP_TIFF_STRIP_H
#define UNPAPER_HIP_TIFF_STRIP_H

#include <stdint.h>

#ifdef __HIPCC__
#define TIFF_FN __host__ __device__ static inline
#else
#define TIFF_FN static inline
#endif

namespace uph {
namespace tiff {

enum Status : int32_t {
  kOk = 0,
  kInput = 1,    // the strip's bytes end too early
  kOutput = 2,   // a PackBits literal or run passes the strip's rows
  kCode = 4,     // an LZW code that cannot occur
  kShort = 8,    // EOI before the strip's rows are full
  kOldLzw = 16,  // the pre-6.0 LSB-first LZW
  kRange = 32,   // a job the decoder cannot take (size, compression)
};

enum : int32_t { kCompNone = 1, kCompLzw = 5, kCompPackBits = 32773 };

constexpr int kLzwCodes = 4096;
constexpr uint32_t kSmallStrip = 65536;  // decoded bytes a uint16_t table serves

TIFF_FN int32_t packbits(const uint8_t* in, uint32_t n, uint8_t* out, uint32_t cap) {
  uint32_t ip = 0, op = 0;
  while (op < cap) {
    if (ip >= n) return kInput;
    const int h = (int8_t)in[ip++];
    if (h == -128) continue;
    if (h >= 0) {
      const uint32_t c = (uint32_t)h + 1;
      if (c > n - ip) return kInput;
      if (c > cap - op) return kOutput;
      for (uint32_t i = 0; i < c; i++) out[op + i] = in[ip + i];
      ip += c;
      op += c;
    } else {
      const uint32_t c = (uint32_t)(1 - h);
      if (ip >= n) return kInput;
      if (c > cap - op) return kOutput;
      const uint8_t v = in[ip++];
      for (uint32_t i = 0; i < c; i++) out[op + i] = v;
      op += c;
    }
  }
  return kOk;
}

// pos / len: kLzwCodes entries each (indices below 258 are not used).
template <class P>
TIFF_FN int32_t lzw(const uint8_t* in, uint32_t n, uint8_t* out, uint32_t cap, P* pos, P* len) {
  if (sizeof(P) == 2 && cap > kSmallStrip) return kRange;
  if (n >= 2 && in[0] == 0 && (in[1] & 1)) return kOldLzw;
  uint32_t ip = 0, op = 0;
  uint32_t acc = 0;  // the low `have` bits are unread
  int have = 0, width = 9;
  int next = 258;
  bool fresh = true;             // no previous string (start, after a Clear)
  uint32_t ppos = 0, plen = 0;   // the previous code's string
  while (op < cap) {
    while (have < width) {
      if (ip >= n) return kInput;
      acc = (acc << 8) | in[ip++];
      have += 8;
    }
    const int code = (int)((acc >> (have - width)) & ((1u << width) - 1));
    have -= width;
    if (code == 257) return kShort;
    if (code == 256) {
      next = 258;
      width = 9;
      fresh = true;
      continue;
    }
    uint32_t spos, slen;
    if (code < 256) {
      out[op] = (uint8_t)code;
      spos = op;
      slen = 1;
      op++;
    } else {
      if (fresh || code > next) return kCode;
      uint32_t from;
      if (code == next) {
        from = ppos;
        slen = plen + 1;
      } else {
        from = pos[code];
        slen = len[code];
      }
      // from + slen <= op: an entry lies in what is written (the KwKwK copy
      // reads its own first byte back, one behind the write)
      if (from >= op || slen - 1 > op - from) return kCode;
      spos = op;
      uint32_t c = slen;
      if (c > cap - op) c = cap - op;
      for (uint32_t i = 0; i < c; i++) out[op + i] = out[from + i];
      op += c;
    }
    if (op >= cap) break;
    if (!fresh && next < kLzwCodes) {
      pos[next] = (P)ppos;
      len[next] = (P)(plen + 1);
      next++;
      if (next == 511 || next == 1023 || next == 2047) width++;
    }
    fresh = false;
    ppos = spos;
    plen = slen;
  }
  return kOk;
}

TIFF_FN uint8_t bitrev8(uint8_t v) {
  v = (uint8_t)((v >> 4) | (v << 4));
  v = (uint8_t)(((v & 0xCC) >> 2) | ((v & 0x33) << 2));
  return (uint8_t)(((v & 0xAA) >> 1) | ((v & 0x55) << 1));
}

// What a page's rows need after the strips are decoded.
struct RowOps {
  int32_t src_bytes;  // stored bytes a row
  int32_t spp;        // samples per pixel as stored (1, 2 or 3); 1 for 1-bit data
  int32_t predictor;  // 1 or 2
  int32_t bitrev;     // FillOrder 2 on uncompressed 1-bit rows
  int32_t invert;     // 8-bit MinIsWhite: sample 0 of every pixel -> 255 - v
  int32_t palette;    // indices -> RGB24 through `pal`
};

// One row: `src` (changed in place by the predictor) into `dst`, src_bytes
// bytes of it, or 3 * src_bytes with a palette (pal: 256 x RGB).
TIFF_FN void finish_row(uint8_t* src, uint8_t* dst, const RowOps& o, const uint8_t* pal) {
  const int32_t n = o.src_bytes;
  if (o.predictor == 2)
    for (int32_t i = o.spp; i < n; i++) src[i] = (uint8_t)(src[i] + src[i - o.spp]);
  if (o.palette) {
    for (int32_t i = 0; i < n; i++) {
      const uint8_t* e = pal + 3 * (int32_t)src[i];
      dst[3 * i] = e[0];
      dst[3 * i + 1] = e[1];
      dst[3 * i + 2] = e[2];
    }
  } else if (o.bitrev) {
    for (int32_t i = 0; i < n; i++) dst[i] = bitrev8(src[i]);
  } else if (o.invert) {
    for (int32_t i = 0; i < n; i++) dst[i] = (i % o.spp) == 0 ? (uint8_t)(255 - src[i]) : src[i];
  } else {
    for (int32_t i = 0; i < n; i++) dst[i] = src[i];
  }
}

}  // namespace tiff
}  // namespace uph

#endif /* UNPAPER_HIP_TIFF_STRIP_H */
