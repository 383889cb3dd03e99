// tiff_dec.h — the device decode of PackBits and LZW TIFF pages
// (kernels_tiff.hip): what the host hands the two kernels.
//
// A page travels as a blob: its strips' bytes one after another, then, for a
// palette page, the 768 palette bytes.  The blobs of a launch lie in one
// device buffer `in`; the strips decode into one scratch buffer that holds
// every page as stored (rows `src_bytes` apart), and k_tiff_rows finishes
// each row into its destination at the destination's pitch.
//
//   k_tiff_strips  a lane per strip; a fixed number of lanes (at most
//                  kStripLanes) walks the jobs grid-stride, so the LZW tables
//                  (kTableBytes a lane) are bounded at 64 MiB a launch
//                  whatever the number of strips
//   k_tiff_rows    a wave per row: Predictor 2 as a wave prefix sum per sample,
//                  MinIsWhite inversion, palette lookup; only bytes
//                  [0, row bytes) of a destination row are written.  (The
//                  bits of a FillOrder 2 strip are reversed before it is
//                  decoded, tiff_strip.h: blob_fill does it on the way into
//                  pinned memory, so the rows have nothing to reverse.)
//
// A strip that fails ORs its tiff::Status into its page's status word and
// writes nothing more; the rows of a page whose status is set are not written.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "tiff.h"

namespace uph {
namespace tiff {

constexpr int kStripLanes = 4096;
constexpr size_t kTableBytes = 2 * sizeof(uint16_t) * kLzwCodes;  // pos and len of one lane

struct StripJob {
  uint64_t in_off;   // the strip's bytes in `in`
  uint64_t out_off;  // its first row in the scratch
  uint32_t in_len, out_len;
  int32_t comp;      // kCompPackBits or kCompLzw
  int32_t page;      // index of the page's status word
};

struct RowsPage {
  uint64_t src_off;  // the page in the scratch
  uint64_t pal_off;  // its palette in `in` (palette pages)
  uint8_t* dst;
  int64_t pitch;
  int32_t height;
  int32_t page;      // index of the page's status word
  RowOps ops;
};

// The blob of a page and its jobs (offsets from in_base / out_base).
size_t blob_bytes(const Page& p);
void blob_fill(const Document& doc, const Page& p, uint8_t* blob);
void page_jobs(const Page& p, uint64_t in_base, uint64_t out_base, int32_t status_index, StripJob* jobs);
RowsPage rows_page(const Page& p, uint64_t in_base, uint64_t out_base, int32_t status_index, uint8_t* dst,
                   int64_t pitch);
inline int strip_lanes(int64_t njobs) {
  const int64_t l = (njobs + 63) / 64 * 64;
  return (int)(l < kStripLanes ? l : kStripLanes);
}

// Queues both kernels on `st`.  All pointers are device memory; `pool` holds
// strip_lanes(njobs) * kTableBytes bytes (may be null when no job is LZW);
// `status` holds a zeroed word for every page.
bool launch(const StripJob* jobs, int njobs, bool any_lzw, const RowsPage* pages, int npages, int max_height,
            const uint8_t* in, uint64_t in_bytes, uint8_t* scratch, uint64_t scratch_bytes, uint16_t* pool,
            int32_t* status, hipStream_t st);

}  // namespace tiff
}  // namespace uph
