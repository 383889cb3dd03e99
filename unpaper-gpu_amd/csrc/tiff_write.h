// tiff_write.h — the host side of TIFF output (tiff_write.cpp): the Deflate
// encoder's host twin over tiff_enc_core.h and the container writers.  No
// device code and no runtime header: the kernels' side is tiff_enc.h.
#pragma once

#include <stdint.h>

#include <mutex>
#include <string>
#include <vector>

#include "tiff_enc_core.h"

namespace uph {

namespace tiffenc {
// tiff_write.cpp: the host twin.  The page's blob from rows `stride` apart.
void encode_page_host(const uint8_t* px, int64_t stride, const Layout& l, std::vector<uint8_t>* blob);
// The arguments of the two encode entries; a bilevel format passes with
// *bilevel set, MONOBLACK is refused by name.
bool check_image(const char* who, const void* src, int64_t stride, int32_t offset, int32_t width, int32_t height,
                 int32_t format, int32_t dpi, Layout* l, bool* bilevel);
// A finished file into the caller's buffer: its size, out = NULL sizes, -1
// when `capacity` is too small.
int64_t give_file(const char* who, const std::vector<uint8_t>& file, void* out, int64_t capacity);
}  // namespace tiffenc

namespace tiff {

// A Group 4 stream of a w x h page as a file of its own: header, one IFD, the
// two resolution rationals, then the stream as the only strip.
bool g4_file(const uint8_t* p, size_t n, int32_t w, int32_t h, int32_t dpi, std::vector<uint8_t>* out);
// A Deflate page's blob as a file of its own: header, the blob, the IFD.
// The bytes a Writer given this one page produces.
bool deflate_file(const uint8_t* blob, size_t n, int32_t w, int32_t h, int32_t format, int32_t dpi,
                  std::vector<uint8_t>* out);

// A multi-page classic little-endian TIFF.  add_page* may be called from
// several threads in any order: a page's data is appended under the mutex
// and its place remembered (a page whose write fails is not remembered and
// the file stays valid with the others); finish() writes the IFDs after the
// data, chained in index order, and patches the header.  The file appears
// under its name only then; a writer destroyed unfinished leaves none.
class Writer {
 public:
  ~Writer();
  bool create(const char* path, int32_t dpi);
  bool add_page_deflate(int64_t index, const uint8_t* blob, size_t len, int32_t width, int32_t height,
                        int32_t format, int32_t dpi);
  bool add_page_g4(int64_t index, const uint8_t* data, size_t len, int32_t width, int32_t height, int32_t dpi);
  int64_t next_index();
  int page_count();
  bool finish();
  void abort();

  struct PageRec {
    int64_t index = 0;
    int32_t width = 0, height = 0, format = 0, dpi = 0;
    bool g4 = false;
    uint32_t data = 0, len = 0;  // where the page's data lies
    int32_t rows_per_strip = 0;
    std::vector<uint32_t> counts;  // StripByteCounts
  };

 private:
  std::mutex mu_;
  int fd_ = -1;
  std::string path_, part_;
  int32_t dpi_ = 300;
  int64_t pos_ = 0;        // bytes of the pages kept so far
  int64_t ifd_bytes_ = 0;  // what finish() will add for the pages taken
  int64_t next_index_ = 0;
  std::vector<PageRec> pages_;
  bool write_at(const void* p, size_t n, int64_t at);
  bool add(PageRec&& rec, const uint8_t* data, size_t len);
};

}  // namespace tiff
}  // namespace uph
