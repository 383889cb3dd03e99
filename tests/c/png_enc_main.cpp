// png_enc_main.cpp — the lossless PNG encoder's host twin (csrc/png_enc.cpp
// over csrc/png_enc_core.h) run stand-alone under ASan/UBSan (make
// sanitize_png): every image is encoded from a heap buffer of exactly the
// bytes it may read, the file's chunks are walked, the IDAT stream inflated
// with zlib, the filters undone and the samples compared.
#include <zlib.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "png_enc_core.h"
#include "runtime.h"
#include "unpaper_hip.h"

// the library's error reporting, which png_enc.cpp calls
namespace uph {
static char g_error[512];
bool fail(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof(g_error), fmt, ap);
  va_end(ap);
  return false;
}
}  // namespace uph

namespace {

int g_failures = 0;
uint32_t g_rng = 12345;
uint32_t rnd() { return g_rng = g_rng * 1664525u + 1013904223u, g_rng >> 8; }

void check(bool ok, const char* what, int fmt, int w, int h) {
  if (ok) return;
  g_failures++;
  fprintf(stderr, "png_enc_main: %s failed (format %d, %dx%d): %s\n", what, fmt, w, h, uph::g_error);
}

uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | p[1] << 16 | p[2] << 8 | p[3]; }

// kind: 0 text-like, 1 noise, 2 flat, 3 equal rows
void run_case(int fmt, int w, int h, int kind, int offset, int slack) {
  uph::pngenc::Shape s;
  if (!uph::pngenc::shape_of(fmt, w, h, &s)) return check(false, "shape_of", fmt, w, h);
  const int64_t stride = (s.depth == 8 ? s.row_bytes : ((int64_t)offset + w + 7) / 8) + slack;
  // the last row ends with its last pixel: a read past it is a heap overflow
  const size_t bytes = (size_t)(stride * (h - 1) + stride - slack);
  std::vector<uint8_t> px(bytes);
  for (size_t i = 0; i < bytes; i++) {
    const size_t x = i % (size_t)stride, y = i / (size_t)stride;
    uint8_t v = kind == 1 ? (uint8_t)rnd() : kind == 2 ? 0xFF : (rnd() % 5 ? 0xF0 : (uint8_t)rnd());
    if (kind == 3 && y > 0) v = px[x];
    px[i] = v;
  }
  const int64_t need = uphip_png_encode_host(px.data(), stride, offset, w, h, fmt, 300, nullptr, 0);
  if (need <= 0) return check(false, "sizing", fmt, w, h);
  std::vector<uint8_t> file((size_t)need);
  if (uphip_png_encode_host(px.data(), stride, offset, w, h, fmt, 300, file.data(), need) != need)
    return check(false, "encode", fmt, w, h);
  // chunks: IHDR pHYs IDAT IEND, each CRC
  size_t at = 8;
  const uint8_t* z = nullptr;
  size_t zn = 0;
  while (at + 12 <= file.size()) {
    const uint32_t n = be32(&file[at]);
    if (at + 12 + n > file.size()) return check(false, "chunk length", fmt, w, h);
    check(be32(&file[at + 8 + n]) == crc32(0L, &file[at + 4], n + 4), "chunk CRC", fmt, w, h);
    if (!memcmp(&file[at + 4], "IDAT", 4)) z = &file[at + 8], zn = n;
    at += 12 + n;
  }
  check(at == file.size() && z, "chunk walk", fmt, w, h);
  if (!z) return;
  check((int64_t)zn <= uph::pngenc::stored_size(s.total), "stored bound", fmt, w, h);
  std::vector<uint8_t> f((size_t)s.total);
  uLongf fl = (uLongf)f.size();
  if (uncompress(f.data(), &fl, z, (uLong)zn) != Z_OK || (int64_t)fl != s.total)
    return check(false, "inflate", fmt, w, h);
  // filters undone in place, then the samples against the source
  bool same = true;
  for (int y = 0; y < h; y++) {
    uint8_t* row = &f[(size_t)(y * s.line)] + 1;
    const uint8_t* up = y ? row - s.line : nullptr;
    const int t = row[-1];
    for (int64_t k = 0; k < s.row_bytes; k++) {
      if (t == 1 && k >= s.bpp) row[k] = (uint8_t)(row[k] + row[k - s.bpp]);
      if (t == 2 && up) row[k] = (uint8_t)(row[k] + up[k]);
      if (t > 2) same = false;
    }
    for (int x = 0; x < w * (s.depth == 8 ? s.channels : 1); x++) {
      if (s.depth == 8) {
        same = same && row[x] == px[(size_t)(y * stride + x)];
      } else {
        const int64_t b = (int64_t)offset + x;
        const int src = (px[(size_t)(y * stride + (b >> 3))] >> (7 - (b & 7))) & 1;
        same = same && ((row[x >> 3] >> (7 - (x & 7))) & 1) == (s.invert ? !src : src);
      }
    }
    if (s.depth == 1 && (w & 7)) same = same && !(row[s.row_bytes - 1] & (0xFF >> (w & 7)));
  }
  check(same, "samples", fmt, w, h);
}

}  // namespace

int main() {
  const int formats[5] = {UPHIP_FMT_GRAY8, UPHIP_FMT_RGB24, UPHIP_FMT_Y400A, UPHIP_FMT_MONOWHITE,
                          UPHIP_FMT_MONOBLACK};
  const int widths[] = {1, 2, 3, 7, 8, 9, 31, 32, 33, 257, 258, 259, 260, 261, 517, 2049};
  const int heights[] = {1, 2, 64, 65};
  int cases = 0;
  for (int fmt : formats) {
    const bool mono = fmt == UPHIP_FMT_MONOWHITE || fmt == UPHIP_FMT_MONOBLACK;
    for (int w : widths)
      for (int h : heights) {
        if (w > 33 && h > 2) continue;
        for (int kind = 0; kind < 4; kind++) {
          run_case(fmt, w, h, kind, 0, 0);
          run_case(fmt, w, h, kind, mono ? 5 : 0, 3);
          cases += 2;
        }
      }
    run_case(fmt, 203, 131, 0, mono ? 13 : 0, 1);
    run_case(fmt, 300, 200, 1, 0, 0);
    cases += 2;
  }
  run_case(UPHIP_FMT_GRAY8, 32769, 3, 3, 0, 0);  // the row above lies beyond the window
  run_case(UPHIP_FMT_GRAY8, 1240, 1754, 2, 0, 0);
  cases += 2;
  // argument errors leave through the error path
  uint8_t one = 0;
  if (uphip_png_encode_host(nullptr, 1, 0, 1, 1, UPHIP_FMT_GRAY8, 0, nullptr, 0) != -1 ||
      uphip_png_encode_host(&one, 1, 1, 1, 1, UPHIP_FMT_GRAY8, 0, nullptr, 0) != -1 ||
      uphip_png_encode_host(&one, 1, 0, 1, 1, 99, 0, nullptr, 0) != -1 ||
      uphip_png_encode_host(&one, 1, 0, 1, 1, UPHIP_FMT_GRAY8, 0, &one, 1) != -1)
    check(false, "argument errors", 0, 1, 1);
  if (g_failures) {
    fprintf(stderr, "png_enc_main: %d failures in %d cases\n", g_failures, cases);
    return 1;
  }
  printf("png_enc_main: ok (%d cases)\n", cases);
  return 0;
}
