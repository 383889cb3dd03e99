// tiff.h — the TIFF reader: the container on the host (tiff.cpp), strips
// through the decoder of tiff_strip.h on the host or, for PackBits and LZW
// pages, on the device (tiff_dec.h, kernels_tiff.hip).
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "tiff_strip.h"
#include "unpaper_hip.h"

namespace uph {
namespace tiff {

// One IFD.  `error` is set when the page is refused; it names the tag.
struct Page {
  std::string error;
  int32_t width = 0, height = 0;
  int32_t format = UPHIP_FMT_NONE;
  int32_t bits = 1, spp = 1, extra = 0;
  int32_t photometric = 0, compression = 1, predictor = 1, fill_order = 1;
  uint32_t rows_per_strip = 0, t4_options = 0;
  float dpi[2] = {0, 0};
  int64_t src_row_bytes = 0;  // stored bytes a row
  std::vector<uint32_t> off, cnt;  // the strips, checked against the file
  std::vector<uint8_t> pal;        // 768 bytes (RGB of index i at 3 i) for palette pages
  RowOps ops{};
  uint32_t strip_rows(size_t s) const {
    const uint32_t left = (uint32_t)height - (uint32_t)s * rows_per_strip;
    return left < rows_per_strip ? left : rows_per_strip;
  }
};

struct Document {
  std::vector<uint8_t> bytes;
  std::string name;
  std::vector<Page> pages;
};

// Parses the header and every IFD; false (with the error) when the file is
// no classic TIFF or holds no IFD.  Pages the reader refuses are kept, with
// their `error`.
bool open(std::vector<uint8_t>&& bytes, const char* name, Document* doc);
// The page, or null with the error (out of range, or refused).
const Page* page(const Document& doc, int64_t index);
// PackBits or LZW, every strip at most 65,536 decoded bytes: what
// k_tiff_strips takes.  The device route of the runner also wants 8 strips.
bool device_decodable(const Page& p);
bool device_route(const Page& p);
// The page's pixels into dst (rows `linesize` apart), on the host.
bool decode_host(const Document& doc, const Page& p, uint8_t* dst, int64_t linesize);
// page + the `expect` and linesize checks of every read entry + decode_host
bool read_page(const Document& doc, int64_t index, void* dst, int64_t linesize, const UphipPnmInfo* expect);
bool read_file(const char* path, std::vector<uint8_t>* out);
bool open_file(const char* path, Document* doc);
const char* strip_error(int32_t status);  // a Status word in words

}  // namespace tiff
}  // namespace uph

struct UphipTiffDocument {
  uph::tiff::Document doc;
};
