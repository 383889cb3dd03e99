// tiff_enc.h — TIFF output: the device Deflate encoder of a page's strips
// (kernels_tiff_enc.hip); its host twin and the container writer are
// tiff_write.h.  What the encoder produces per page is the blob of
// tiff_enc_core.h (StripByteCounts, then the strips), the same bytes on the
// device and on the host.  A stream is (page, strip); all streams of a batch
// go through each launch:
//
//   A  k_tiff_predict   a block stages up to 16 rows of a page into LDS
//                       (coalesced dword loads, odd dword stride); a wave per
//                       row writes the row's Predictor 2 differences to `filt`
//   B  k_tiff_hist      a lane per segment of a stream: the greedy parse into
//                       an LDS histogram, flushed to the stream's counts; the
//                       segment's Adler sums
//   C  k_png_table      PNG's kernel, a wave per stream: the counts to codes
//   D  k_tiff_count     the same parse, each lane summing its tokens' bits
//      k_tiff_scan      per stream: prefix sum of the bits, the Adler-32, the
//                       stream's size, stored or coded
//      k_tiff_pages     per page: the strips' places in the page's blob, the
//                       blob's size
//      k_tiff_offsets   the pages' byte offsets in the packed output
//      k_tiff_counts    per stream: its StripByteCounts entry at the blob's
//                       head, its place made one in the packed output
//   E  k_tiff_emit      the same parse, each lane writing its codes at its
//                       segment's bit offset in the zeroed output
//      k_tiff_stored    streams that would not shrink, as stored blocks
//
// The stream index lies on grid.y, folded: a block takes streams blockIdx.y,
// blockIdx.y + gridDim.y, .. so that more streams than a grid's 65,535 rows
// (a batch of double-page RGB sheets) need no second launch.  The PNG
// kernels (kernels_png.hip) are not shared: they keep one stream per page.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>


#include "buffer.h"
#include "png_enc.h"
#include "tiff_enc_core.h"

namespace uph {

constexpr int32_t kTiffFoldLimit = 65535;  // gridDim.y's limit

// The device buffers of an encoder, as PngContext.
struct TiffEncContext {
  int device = -1;
  Buffer filt{Buffer::Device};        // npages * filt_stride predicted bytes
  Buffer segoff{Buffer::Device};      // int64 per segment slot: token bits, then their prefix sum
  Buffer segadler{Buffer::Device};    // uint2 per segment slot: Adler sums
  Buffer tabs{Buffer::Device};        // a pngenc::PageTab per stream
  Buffer meta{Buffer::Device};        // int64: sizes[n], offsets[n] of the pages, place[streams] in the blob
  Buffer out{Buffer::Device};         // the packed blobs
  Buffer host_sizes{Buffer::Pinned};  // int64: sizes[n] of the last encode
  // An output the caller lends instead of `out` (4-byte aligned, at least the
  // pages' bound rounded up to a dword + 4 bytes: what the encode zeroes and
  // the only bytes it writes); `packed` is where the last encode's blobs lie.
  uint8_t* lent = nullptr;
  size_t lent_capacity = 0;
  uint8_t* packed = nullptr;
  int n = 0;
  ~TiffEncContext();  // selects the device; the buffers release after it
  size_t device_bytes() const {
    return filt.capacity() + segoff.capacity() + segadler.capacity() + tabs.capacity() + meta.capacity() +
           out.capacity();
  }
  // zeroes the output, queues the encode of pg (GRAY8, RGB24 or Y400A pages;
  // PngPages addressing) and the copy of the blobs' sizes into host_sizes.
  // `fold`: the most streams a launch puts on grid.y.
  bool encode_async(const PngPages& pg, hipStream_t st, int32_t fold = kTiffFoldLimit);
};

}  // namespace uph
