// png_enc.cpp — the host side of the lossless PNG output: the encoder's host
// twin (png_enc_core.h run on the CPU; the kernels of kernels_png.hip produce
// the same bytes) and the PNG container around a zlib stream.  No reference
// peer: the reference's saveImage writes PNM only.
#include <zlib.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "png_enc.h"
#include "png_enc_core.h"
#include "runtime.h"
#include "unpaper_hip.h"

namespace uph {
namespace pngenc {

bool check_image(const char* who, const void* src, int64_t stride, int32_t offset, int32_t width, int32_t height,
                 int32_t format, int32_t dpi, Shape* s) {
  if (!src) return fail("%s: null source", who);
  if (width <= 0 || width > (1 << 20) || height <= 0 || height > (1 << 20))
    return fail("%s: invalid size %dx%d", who, width, height);
  if (!shape_of(format, width, height, s)) return fail("%s: unknown pixel format %d", who, format);
  if (dpi < 0) return fail("%s: dpi %d is negative", who, dpi);
  if (s->depth == 8 && offset != 0)
    return fail("%s: offset %d on a byte format (offset the pointer instead)", who, offset);
  const int64_t need = s->depth == 8 ? s->row_bytes : ((int64_t)offset + width + 7) / 8;
  if (offset < 0 || stride < need)
    return fail("%s: pixels %d..%lld do not fit rows of %lld bytes", who, offset, (long long)offset + width,
                (long long)stride);
  return true;
}

namespace {

struct HostRow {
  const uint8_t* p;
  uint32_t byte(int64_t i) const { return p[i]; }
};

struct HostSink {
  uint32_t* out;
  int64_t w = 0;
  uint64_t acc = 0;
  int n = 0;
  void put(uint32_t bits, int len) {
    acc |= (uint64_t)bits << n;
    n += len;
    if (n >= 32) {
      out[w++] |= (uint32_t)acc;
      acc >>= 32;
      n -= 32;
    }
  }
  void finish() {
    if (n > 0) out[w] |= (uint32_t)acc;
  }
};

struct HistVisitor {
  uint32_t* freq;
  void literal(uint32_t b) { freq[b]++; }
  void match(int len, int dist) {
    int sym, eb;
    uint32_t ev;
    length_symbol(len, &sym, &eb, &ev);
    freq[sym]++;
    distance_symbol(dist, &sym, &eb, &ev);
    freq[kLL + sym]++;
  }
};

int sorted_order(const uint32_t* freq, int n, uint16_t* order) {
  int used = 0;
  for (int s = 0; s < n; s++)
    if (freq[s]) order[sorted_place(freq, n, s)] = (uint16_t)s, used++;
  return used;
}

}  // namespace

void encode_stream_host(const uint8_t* px, int64_t stride, int32_t offset, const Shape& s, std::vector<uint8_t>* out) {
  // the filtered stream
  std::vector<uint8_t> rows((size_t)s.total);
  uint8_t* filt = rows.data();
  const int off = offset & 7;
  for (int32_t y = 0; y < s.height; y++) {
    const HostRow cur{px + (int64_t)y * stride + (offset >> 3)};
    const HostRow up{y ? cur.p - stride : cur.p};
    uint32_t sum[3] = {0, 0, 0};
    if (s.depth == 8) filter_sums(cur, off, up, off, y > 0, s, 0, 1, sum);
    const int f = choose_filter(s, sum);
    uint8_t* dst = filt + (int64_t)y * s.line;
    dst[0] = (uint8_t)f;
    filter_row(cur, off, up, off, y > 0, s, f, 0, 1, dst);
  }
  deflate_host(filt, s, out);
}

void deflate_host(const uint8_t* filt, const Shape& s, std::vector<uint8_t>* out) {
  // counts and the checksum
  PageTab t;
  memset(&t, 0, sizeof(t));
  const int64_t nseg = segments_of(s.total);
  uint32_t A = 1, B = 0;
  HistVisitor hv{t.freq};
  for (int64_t g = 0; g < nseg; g++) {
    const int64_t lo = g * kSegBytes, hi = std::min<int64_t>(lo + kSegBytes, s.total);
    parse_segment(filt, lo, hi, s, hv);
    uint32_t a, b;
    adler_segment(filt + lo, (int)(hi - lo), &a, &b);
    adler_append(&A, &B, (uint64_t)(hi - lo), a, b);
  }
  t.adler = B << 16 | A;
  t.freq[kEob]++;
  bool any = false;
  for (int i = 0; i < kDD; i++) any = any || t.freq[kLL + i];
  if (!any) t.freq[kLL] = 1;
  uint16_t lo_[kLL], do_[kDD];
  uint32_t work[2 * kLL];
  const int lu = sorted_order(t.freq, kLL, lo_), du = sorted_order(t.freq + kLL, kDD, do_);
  build_tables(&t, lo_, lu, do_, du, work);
  // sizes
  for (int64_t g = 0; g < nseg; g++) {
    CountSink cs;
    CodeTokens<CountSink> v(t.code, cs);
    parse_segment(filt, g * kSegBytes, std::min<int64_t>((g + 1) * kSegBytes, s.total), s, v);
    t.token_bits += cs.bits;
  }
  decide_size(&t, s.total);
  // the stream
  std::vector<uint32_t> words((size_t)(t.size + 3) / 4 + 1, 0u);
  uint8_t* z = (uint8_t*)words.data();
  if (t.stored) {
    z[0] = 0x78;
    z[1] = 0x01;
    for (int64_t i = 0; i < s.total; i += kStoredBlock) {
      stored_header(i, s.total, z + stored_place(i) - 5);
      memcpy(z + stored_place(i), filt + i, (size_t)std::min<int64_t>(kStoredBlock, s.total - i));
    }
    for (int k = 0; k < 4; k++) z[t.size - 4 + k] = (uint8_t)(t.adler >> (24 - 8 * k));
  } else {
    HostSink sink{words.data()};
    sink.put(0x78, 8);
    sink.put(0x01, 8);
    put_block_header(t, sink);
    CodeTokens<HostSink> v(t.code, sink);
    for (int64_t g = 0; g < nseg; g++)
      parse_segment(filt, g * kSegBytes, std::min<int64_t>((g + 1) * kSegBytes, s.total), s, v);
    sink.put(t.code[kEob] & 0xFFFFu, (int)(t.code[kEob] >> 16));
    sink.put(0, (8 - sink.n % 8) % 8);
    for (int k = 0; k < 4; k++) sink.put((t.adler >> (24 - 8 * k)) & 0xFFu, 8);
    sink.finish();
  }
  out->assign(z, z + t.size);
}

int64_t wrapped_size(int64_t stream, int32_t dpi) { return 8 + 25 + (dpi > 0 ? 21 : 0) + 12 + stream + 12; }

namespace {
uint8_t* chunk(uint8_t* p, const char type[4], const uint8_t* data, size_t n) {
  const uint32_t len = (uint32_t)n;
  for (int k = 0; k < 4; k++) p[k] = (uint8_t)(len >> (24 - 8 * k));
  memcpy(p + 4, type, 4);
  if (n) memcpy(p + 8, data, n);
  uLong c = crc32(0L, p + 4, 4);
  for (size_t at = 0; at < n;) {  // crc32 takes a uInt
    const size_t step = std::min<size_t>(n - at, (size_t)1 << 30);
    c = crc32(c, p + 8 + at, (uInt)step);
    at += step;
  }
  for (int k = 0; k < 4; k++) p[8 + n + k] = (uint8_t)(c >> (24 - 8 * k));
  return p + 12 + n;
}
}  // namespace

void wrap(const uint8_t* stream, int64_t len, const Shape& s, int32_t dpi, uint8_t* out) {
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
  memcpy(out, sig, 8);
  uint8_t* p = out + 8;
  uint8_t hdr[13];
  for (int k = 0; k < 4; k++) {
    hdr[k] = (uint8_t)((uint32_t)s.width >> (24 - 8 * k));
    hdr[4 + k] = (uint8_t)((uint32_t)s.height >> (24 - 8 * k));
  }
  hdr[8] = (uint8_t)s.depth;
  hdr[9] = (uint8_t)s.colour_type;
  hdr[10] = hdr[11] = hdr[12] = 0;  // deflate, adaptive filtering, not interlaced
  p = chunk(p, "IHDR", hdr, 13);
  if (dpi > 0) {
    const uint32_t ppm = (uint32_t)lround((double)dpi / 0.0254);
    uint8_t phys[9];
    for (int k = 0; k < 4; k++) phys[k] = phys[4 + k] = (uint8_t)(ppm >> (24 - 8 * k));
    phys[8] = 1;  // the unit is the metre
    p = chunk(p, "pHYs", phys, 9);
  }
  p = chunk(p, "IDAT", stream, (size_t)len);
  chunk(p, "IEND", nullptr, 0);
}

}  // namespace pngenc
}  // namespace uph

using namespace uph;

extern "C" int64_t uphip_png_wrap(const void* stream, int64_t len, int32_t width, int32_t height, int32_t format,
                                  int32_t dpi, void* out, int64_t capacity) {
  pngenc::Shape s;
  if (!stream || len <= 0) return fail("png_wrap: null or empty stream"), -1;
  if (len > 0x7FFFFFFFll) return fail("png_wrap: a %lld-byte stream does not fit one IDAT chunk", (long long)len), -1;
  if (width <= 0 || height <= 0) return fail("png_wrap: invalid size %dx%d", width, height), -1;
  if (!pngenc::shape_of(format, width, height, &s)) return fail("png_wrap: unknown pixel format %d", format), -1;
  if (dpi < 0) return fail("png_wrap: dpi %d is negative", dpi), -1;
  const int64_t size = pngenc::wrapped_size(len, dpi);
  if (!out) return size;
  if (capacity < size) return fail("png_wrap: the file needs %lld bytes, the buffer has %lld", (long long)size,
                                   (long long)capacity), -1;
  pngenc::wrap((const uint8_t*)stream, len, s, dpi, (uint8_t*)out);
  return size;
}

extern "C" int64_t uphip_png_encode_host(const void* pixels, int64_t stride, int32_t offset, int32_t width,
                                         int32_t height, int32_t format, int32_t dpi, void* out, int64_t capacity) {
  pngenc::Shape s;
  if (!pngenc::check_image("png_encode_host", pixels, stride, offset, width, height, format, dpi, &s)) return -1;
  std::vector<uint8_t> z;
  pngenc::encode_stream_host((const uint8_t*)pixels, stride, offset, s, &z);
  return uphip_png_wrap(z.data(), (int64_t)z.size(), width, height, format, dpi, out, capacity);
}
