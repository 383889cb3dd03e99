/* tiff_enc_core.h — the TIFF Deflate encoder's core, shared by the host twin
 * (tiff_write.cpp) and the device kernels (kernels_tiff_enc.hip) so that both
 * produce the same bytes.  What it codes is the data of one page of a TIFF
 * file with Compression 8 and Predictor 2: strips, each a zlib stream of its
 * own.  The LZ77 parse, the code tables and the stream's form are those of
 * png_enc_core.h; what differs is said here.
 *
 * Formats.  GRAY8 1 sample (Photometric 1), RGB24 3 samples (Photometric 2),
 * Y400A gray plus one extra sample (ExtraSamples 2), all 8 bits.  Bilevel
 * pages are not Deflate-coded: MONOWHITE goes through the Group 4 encoder,
 * MONOBLACK is refused.
 *
 * Strips.  RowsPerStrip = clamp(65536 / row_bytes, 1, height), integer
 * division (libtiff's default): every strip decodes to at most 65,536 bytes
 * unless a single row is longer.  The last strip may be shorter.
 *
 * Strip data.  Predictor 2: each sample byte minus the same sample of the
 * pixel to its left, mod 256; the first pixel of a row is unchanged.  There
 * is no filter byte, so a "line" is row_bytes and the page's predicted bytes
 * are height * row_bytes, strip after strip.
 *
 * Streams.  A stream is one strip.  Segments of kSegBytes restart at the
 * strip's first byte; positions count from it, so a candidate distance d
 * (1 .. bpp, then row_bytes when <= 32768) needs d <= i within the strip and
 * no match reaches into the previous strip.  Each strip has one
 * dynamic-Huffman block over its own histograms, or stored blocks when
 * coding would not shrink it, the `78 01` wrapper and its own Adler-32.  A
 * strip is at most stored_size(strip bytes) long.
 *
 * A page's packed form (the blob): its StripByteCounts as little-endian
 * uint32, one per strip, then the strips in order, each starting on a byte.
 * A container writer appends the blob as it is, points the StripByteCounts
 * tag at its head and derives StripOffsets by a prefix sum.
 */
#ifndef UNPAPER_HIP_TIFF_ENC_CORE_H
#define UNPAPER_HIP_TIFF_ENC_CORE_H

#include <stdint.h>

#include "png_enc_core.h"

namespace uph {
namespace tiffenc {

constexpr int64_t kStripAim = 65536;  // decoded bytes a strip holds at most (a longer row is a strip)

struct Layout {
  int32_t fmt, width, height, channels;
  int32_t rows_per_strip, nstrips;
  int64_t row_bytes;
  int64_t page_bytes;   // height * row_bytes: the predicted page
  int64_t strip_bytes;  // rows_per_strip * row_bytes: every strip but the last
  int64_t strip_segs;   // segments of a full strip
};

PNG_FN bool layout_of(int32_t fmt, int32_t width, int32_t height, Layout* l) {
  switch (fmt) {
    case UPHIP_FMT_GRAY8: l->channels = 1; break;
    case UPHIP_FMT_RGB24: l->channels = 3; break;
    case UPHIP_FMT_Y400A: l->channels = 2; break;
    default: return false;
  }
  l->fmt = fmt;
  l->width = width;
  l->height = height;
  l->row_bytes = (int64_t)width * l->channels;
  int64_t rps = kStripAim / l->row_bytes;
  if (rps < 1) rps = 1;
  if (rps > height) rps = height;
  l->rows_per_strip = (int32_t)rps;
  l->nstrips = (int32_t)((height + rps - 1) / rps);
  l->page_bytes = l->row_bytes * height;
  l->strip_bytes = l->row_bytes * rps;
  l->strip_segs = pngenc::segments_of(l->strip_bytes);
  return true;
}

/* Predicted bytes of strip k. */
PNG_FN int64_t strip_total(const Layout& l, int32_t k) {
  const int64_t left = l.page_bytes - (int64_t)k * l.strip_bytes;
  return left < l.strip_bytes ? left : l.strip_bytes;
}

/* The most a page's blob can take: the counts and every strip stored. */
PNG_FN int64_t blob_bound(const Layout& l) {
  return 4 * (int64_t)l.nstrips + (int64_t)(l.nstrips - 1) * pngenc::stored_size(l.strip_bytes) +
         pngenc::stored_size(strip_total(l, l.nstrips - 1));
}

/* What parse_segment reads of a shape, for a strip: the pixel's bytes and the
 * row distance.  `total` is the strip's. */
PNG_FN pngenc::Shape strip_shape(const Layout& l, int64_t total) {
  pngenc::Shape s;
  s.fmt = l.fmt;
  s.width = l.width;
  s.height = (int32_t)(total / l.row_bytes);
  s.depth = 8;
  s.colour_type = 0;
  s.channels = l.channels;
  s.bpp = l.channels;
  s.invert = 0;
  s.row_bytes = l.row_bytes;
  s.line = l.row_bytes;
  s.total = total;
  return s;
}

/* Writes predicted bytes k0, k0 + step, .. of a row read through R (uint32_t
 * byte(int64_t i)) to dst. */
template <class R>
PNG_FN void predict_row(const R& cur, const Layout& l, int64_t k0, int64_t step, uint8_t* dst) {
  for (int64_t k = k0; k < l.row_bytes; k += step) {
    const uint32_t x = cur.byte(k);
    const uint32_t a = k >= l.channels ? cur.byte(k - l.channels) : 0u;
    dst[k] = (uint8_t)((x - a) & 0xFFu);
  }
}

}  // namespace tiffenc
}  // namespace uph

#endif
