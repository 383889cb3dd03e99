// g4_enc.h — the device CCITT Group 4 encoder (kernels_g4.hip): the bilevel
// output branch beside the JPEG one (jpeg_enc.h).  Every row of every page is
// coded against the row above, which the source holds, so all rows are
// independent; a lane codes a row with the coder the host encoder uses
// (g4_row.h) and only the concatenation of the rows' bits needs a scan:
//
//   A  k_g4_rows<false>  a block of 64 lanes stages up to 64 consecutive rows
//                        of a page and the row above into LDS (coalesced
//                        dword loads, odd dword stride a row); lane r walks
//                        row r and writes its bit count
//   B  k_g4_scan         per page: exclusive prefix sum of the counts (64-bit),
//                        the page's byte size with EOFB and padding, -1 when
//                        larger than the page's share
//      k_g4_offsets      the pages' byte offsets in the packed output
//   C  k_g4_rows<true>   the same walk, each lane writing its codes at its
//                        row's bit offset in the zeroed output: whole words
//                        with plain stores, a row's first and last words
//                        (shared with its neighbours) with atomicOr; the
//                        lane of a page's last row appends EOFB
//
// Two passes keep the encoder free of per-row scratch and per-row caps.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "buffer.h"

namespace uph {

// The pages of one encode, all of one size: page p lies in sheet
// p / per_sheet at base + sheet * sheet_stride (rows `pitch` apart, packed
// bits, MSB first, 1 = black) and starts at bit
// bit_offset + (p % per_sheet) * width of every row.
struct G4Pages {
  const uint8_t* base;
  int64_t sheet_stride, pitch;
  int32_t per_sheet, bit_offset;
  int32_t width, height, npages;
};

// Rows a block takes and the LDS it needs for pages `width` wide; fails
// (naming the kernel) when not even one row and its reference fit.
struct G4Launch {
  int32_t rows, stride_words;
  uint32_t lds_bytes;
};
bool g4_plan(int32_t width, G4Launch* l);

// Queues A, B (sizes[p]: bytes, or -1 when above `share`; offs[p]) and C on
// st.  rowoff: npages * height entries; out: zeroed, 4-byte aligned, at
// least the sum of the sizes rounded up to 4 bytes.
bool g4_measure(const G4Pages& pg, const G4Launch& l, int64_t* rowoff, int64_t* sizes, int64_t* offs,
                int64_t share, hipStream_t st);
bool g4_emit(const G4Pages& pg, const G4Launch& l, const int64_t* rowoff, const int64_t* sizes,
             const int64_t* offs, uint8_t* out, hipStream_t st);

// The device buffers of a batch's encoder, allocated by the first encode and
// grown on demand (the stream is waited for only then).
struct G4Context {
  int device = -1;
  Buffer rowoff{Buffer::Device};
  Buffer meta{Buffer::Device};        // int64: sizes[n] then offsets[n]
  Buffer out{Buffer::Device};         // the packed streams
  Buffer host_sizes{Buffer::Pinned};  // int64: sizes[n] of the last encode
  int n = 0;
  ~G4Context();  // selects the device; the buffers release after it
  // zeroes the output, queues the encode of pg (pages above `share` bytes are
  // left out and sized -1) and the copy of the sizes into host_sizes
  bool encode_async(const G4Pages& pg, int64_t share, hipStream_t st);
};

}  // namespace uph
