// png_enc.h — the device lossless PNG encoder (kernels_png.hip): the third
// output branch beside JPEG (jpeg_enc.h) and Group 4 (g4_enc.h).  What it
// produces per page is the zlib stream of png_enc_core.h, the same bytes as
// the host twin (png_enc.cpp); the host wraps it into a PNG file or a PDF
// /FlateDecode image.  All pages of a batch go through each launch
// (grid.y = page):
//
//   A  k_png_filter   a block stages up to 16 rows of a page and the row above
//                     into LDS (coalesced dword loads, odd dword stride); a
//                     wave per row sums the None / Sub / Up costs, takes the
//                     filter and writes the row's filtered bytes to `filt`
//   B  k_png_hist     a lane per segment of kSegBytes filtered bytes: the
//                     greedy parse into an LDS histogram, flushed with integer
//                     atomics to the page's counts; the segment's Adler sums
//   C  k_png_table    a wave per page: ranks the symbols, lane 0 builds the
//                     length-limited codes and sizes the block header
//   D  k_png_count    the same parse, each lane summing its tokens' bits
//      k_png_scan     per page: exclusive prefix sum of the bits (64-bit), the
//                     Adler-32 combined, the page's size, stored or coded
//      k_png_offsets  the pages' byte offsets in the packed output
//   E  k_png_emit     the same parse, each lane writing its codes at its
//                     segment's bit offset in the zeroed output: whole words
//                     with plain stores, a segment's first and last words with
//                     atomicOr; segment 0 writes the zlib and block headers,
//                     the last one end-of-block, padding and the Adler-32
//      k_png_stored   pages that would not shrink: the filtered bytes copied
//                     into stored blocks
//
// The parse is repeated in B, D and E, so no tokens are kept.  Device
// memory per page of `total` filtered bytes: total (filt) + the stored bound
// (out) + 16 bytes a segment + one PageTab.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "buffer.h"
#include "png_enc_core.h"

namespace uph {

// The pages of one encode, all of one size and format.  Page p lies in sheet
// s = p / per_sheet, whose rows start at
// plane[cur ? cur[s * cur_step] & 1 : 0] + s * sheet_stride, `pitch` apart,
// and begins at pixel offset + (p % per_sheet) * sheet_width / per_sheet of
// every row (a bit for bilevel formats: a page may start inside a byte).
struct PngPages {
  const uint8_t* plane[2];
  const int32_t* cur;  // device words that name each sheet's plane, or null
  int64_t cur_step;    // int32 words between two sheets' entries
  int64_t sheet_stride, pitch;
  int32_t per_sheet, sheet_width, offset;
  int32_t format, width, height, npages;
};

// Rows a block of k_png_filter takes and its LDS; fails, naming the kernel,
// when a row and the row above do not fit a block's LDS.
struct PngLaunch {
  int32_t rows, stride_words;
  uint32_t lds_bytes;
};
bool png_plan(const pngenc::Shape& s, PngLaunch* l);
// k_png_table over tabs[0..n): a wave per table, whatever its stream is (the
// TIFF encoder's strips take it too).
void png_table_launch(pngenc::PageTab* tabs, unsigned n, hipStream_t st);

// The device buffers of an encoder, allocated by the first encode and grown
// on demand (the stream is waited for only then).
struct PngContext {
  int device = -1;
  Buffer filt{Buffer::Device};        // npages * filt_stride filtered bytes
  Buffer segoff{Buffer::Device};      // int64 per segment: token bits, then their prefix sum
  Buffer segadler{Buffer::Device};    // uint2 per segment: Adler sums
  Buffer tabs{Buffer::Device};        // a pngenc::PageTab per page
  Buffer meta{Buffer::Device};        // int64: sizes[n] then offsets[n]
  Buffer out{Buffer::Device};         // the packed streams
  Buffer host_sizes{Buffer::Pinned};  // int64: sizes[n] of the last encode
  int n = 0;
  ~PngContext();  // selects the device; the buffers release after it
  size_t device_bytes() const {
    return filt.capacity() + segoff.capacity() + segadler.capacity() + tabs.capacity() + meta.capacity() +
           out.capacity();
  }
  // zeroes the output, queues the encode of pg and the copy of the sizes
  // into host_sizes
  bool encode_async(const PngPages& pg, hipStream_t st);
};

namespace pngenc {
// png_enc.cpp
bool check_image(const char* who, const void* src, int64_t stride, int32_t offset, int32_t width, int32_t height,
                 int32_t format, int32_t dpi, Shape* s);
// The zlib stream of the s.total filtered bytes at `filt` (the core's LZ77
// and entropy coding on the host; of `s` the parse reads bpp, line and total).
void deflate_host(const uint8_t* filt, const Shape& s, std::vector<uint8_t>* out);
}  // namespace pngenc

}  // namespace uph
