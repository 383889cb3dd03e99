// tiff_write.cpp — the host side of TIFF output: the Deflate encoder's host
// twin (tiff_enc_core.h run on the CPU; the kernels of kernels_tiff_enc.hip
// produce the same bytes) and the container writers: a page as a file of its
// own and tiff::Writer, one file of many pages.  No reference peer: the
// reference's saveImage writes PNM only.
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ccitt.h"
#include "runtime.h"
#include "png_enc.h"
#include "tiff_write.h"
#include "unpaper_hip.h"

namespace uph {
namespace tiffenc {

namespace {
struct HostRow {
  const uint8_t* p;
  uint32_t byte(int64_t i) const { return p[i]; }
};
}  // namespace

void encode_page_host(const uint8_t* px, int64_t stride, const Layout& l, std::vector<uint8_t>* blob) {
  std::vector<uint8_t> pred((size_t)l.page_bytes);
  for (int32_t y = 0; y < l.height; y++)
    predict_row(HostRow{px + (int64_t)y * stride}, l, 0, 1, pred.data() + (int64_t)y * l.row_bytes);
  blob->assign((size_t)(4 * (int64_t)l.nstrips), 0);
  std::vector<uint8_t> z;
  for (int32_t k = 0; k < l.nstrips; k++) {
    const int64_t total = strip_total(l, k);
    pngenc::deflate_host(pred.data() + (int64_t)k * l.strip_bytes, strip_shape(l, total), &z);
    const uint32_t n = (uint32_t)z.size();
    for (int b = 0; b < 4; b++) (*blob)[(size_t)(4 * k + b)] = (uint8_t)(n >> (8 * b));
    blob->insert(blob->end(), z.begin(), z.end());
  }
}

bool check_image(const char* who, const void* src, int64_t stride, int32_t offset, int32_t width, int32_t height,
                 int32_t format, int32_t dpi, Layout* l, bool* bilevel) {
  if (!src) return fail("%s: null source", who);
  if (width <= 0 || width > (1 << 20) || height <= 0 || height > (1 << 20))
    return fail("%s: invalid size %dx%d", who, width, height);
  if (format == UPHIP_FMT_MONOBLACK)
    return fail("%s: MONOBLACK pages are not written as TIFF (bilevel TIFF output is Group 4 of MONOWHITE pages)",
                who);
  *bilevel = format == UPHIP_FMT_MONOWHITE;
  if (!*bilevel && !layout_of(format, width, height, l)) return fail("%s: unknown pixel format %d", who, format);
  if (dpi < 0 || dpi > 1200) return fail("%s: dpi %d outside 0..1200", who, dpi);
  if (!*bilevel && offset != 0)
    return fail("%s: offset %d on a byte format (offset the pointer instead)", who, offset);
  const int64_t need = *bilevel ? ((int64_t)offset + width + 7) / 8 : l->row_bytes;
  if (offset < 0 || stride < need)
    return fail("%s: pixels %d..%lld do not fit rows of %lld bytes", who, offset, (long long)offset + width,
                (long long)stride);
  return true;
}

}  // namespace tiffenc

namespace tiff {

namespace {

constexpr int64_t kLimit = 0xFFFFFFFFll;  // classic TIFF: every offset below 2^32 - 1

struct Bytes {
  std::vector<uint8_t>& f;
  void u16(uint32_t v) {
    f.push_back((uint8_t)v);
    f.push_back((uint8_t)(v >> 8));
  }
  void u32(uint32_t v) {
    u16(v & 0xFFFF);
    u16(v >> 16);
  }
  // type 3 SHORT, 4 LONG, 5 RATIONAL; a SHORT sits in the low half, the rest zero
  void entry(uint32_t tag, uint32_t type, uint32_t count, uint32_t value) {
    u16(tag);
    u16(type);
    u32(count);
    u32(value);
  }
};

// The IFD of a page that lies at offset `at` (even), and after it the values
// that do not fit their entries, each on an even offset.  page_count 0: a
// file of one page, without NewSubfileType and PageNumber.  A Group 4 page
// has the tags of g4_file.
void build_ifd(const Writer::PageRec& r, uint32_t at, uint32_t page_no, uint32_t page_count, uint32_t next,
               std::vector<uint8_t>* out) {
  const bool multi = page_count > 0;
  const int spp = r.g4 ? 1 : r.format == UPHIP_FMT_RGB24 ? 3 : r.format == UPHIP_FMT_Y400A ? 2 : 1;
  const uint32_t nstrips = (uint32_t)r.counts.size();
  const int entries = 14 + (spp == 2) + (multi ? 2 : 0);
  // the values after the IFD: BitsPerSample of RGB, StripOffsets of several
  // strips, the resolutions
  uint32_t tail = at + 2 + (uint32_t)entries * 12 + 4;
  uint32_t bits_at = 0, offs_at = 0;
  if (spp == 3) bits_at = tail, tail += 6;
  if (nstrips > 1) offs_at = tail, tail += 4 * nstrips;
  const uint32_t res_at = tail;
  const uint32_t first = r.g4 ? r.data : r.data + 4 * nstrips;  // a blob starts with its counts
  Bytes b{*out};
  b.u16((uint32_t)entries);
  if (multi) b.entry(254, 4, 1, 2);                              // NewSubfileType: a page of many
  b.entry(256, 4, 1, (uint32_t)r.width);                         // ImageWidth
  b.entry(257, 4, 1, (uint32_t)r.height);                        // ImageLength
  if (spp == 3) b.entry(258, 3, 3, bits_at);                     // BitsPerSample
  else b.entry(258, 3, (uint32_t)spp, r.g4 ? 1u : spp == 2 ? 8u | 8u << 16 : 8u);
  b.entry(259, 3, 1, r.g4 ? 4 : 8);                              // Compression: CCITT T.6 or Deflate
  b.entry(262, 3, 1, r.g4 ? 0 : spp == 3 ? 2 : 1);               // PhotometricInterpretation
  if (r.g4) b.entry(266, 3, 1, 1);                               // FillOrder: MSB first
  b.entry(273, 4, nstrips, nstrips > 1 ? offs_at : first);       // StripOffsets
  b.entry(277, 3, 1, (uint32_t)spp);                             // SamplesPerPixel
  b.entry(278, 4, 1, (uint32_t)r.rows_per_strip);                // RowsPerStrip
  b.entry(279, 4, nstrips, nstrips > 1 ? r.data : r.counts[0]);  // StripByteCounts: the blob's head
  b.entry(282, 5, 1, res_at);                                    // XResolution
  b.entry(283, 5, 1, res_at + 8);                                // YResolution
  if (!r.g4) b.entry(284, 3, 1, 1);                              // PlanarConfiguration
  if (r.g4) b.entry(293, 4, 1, 0);                               // T6Options
  b.entry(296, 3, 1, 2);                                         // ResolutionUnit: inch
  if (multi) b.entry(297, 3, 2, (page_no & 0xFFFF) | (page_count > 0xFFFF ? 0 : page_count) << 16);  // PageNumber
  if (!r.g4) b.entry(317, 3, 1, 2);                              // Predictor: horizontal differencing
  if (spp == 2) b.entry(338, 3, 1, 2);                           // ExtraSamples: unassociated alpha
  b.u32(next);
  if (spp == 3)
    for (int i = 0; i < 3; i++) b.u16(8);
  if (nstrips > 1) {
    uint32_t o = first;
    for (uint32_t k = 0; k < nstrips; k++) {
      b.u32(o);
      o += r.counts[k];
    }
  }
  for (int i = 0; i < 2; i++) {
    b.u32((uint32_t)r.dpi);
    b.u32(1);
  }
}

// The record of a Deflate page from its blob: the counts read and checked.
bool deflate_record(const char* who, const uint8_t* blob, size_t len, int32_t width, int32_t height, int32_t format,
                    int32_t dpi, Writer::PageRec* r) {
  if (!blob || !len) return fail("%s: null or empty page", who);
  if (width <= 0 || width > (1 << 20) || height <= 0 || height > (1 << 20))
    return fail("%s: invalid size %dx%d", who, width, height);
  if (dpi < 0 || dpi > 1200) return fail("%s: dpi %d outside 0..1200", who, dpi);
  tiffenc::Layout l;
  if (!tiffenc::layout_of(format, width, height, &l))
    return fail("%s: format %d is no Deflate page (GRAY8, RGB24 or Y400A)", who, format);
  uint64_t sum = 4 * (uint64_t)l.nstrips;
  if (len < sum) return fail("%s: a %zu-byte page cannot hold the counts of %d strips", who, len, l.nstrips);
  r->counts.resize((size_t)l.nstrips);
  for (int32_t k = 0; k < l.nstrips; k++) {
    const uint8_t* p = blob + 4 * (size_t)k;
    const uint32_t n = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    if (!n) return fail("%s: strip %d is empty", who, k);
    r->counts[(size_t)k] = n;
    sum += n;
  }
  if (sum != len) return fail("%s: the strips' counts give %llu bytes, the page has %zu", who, (unsigned long long)sum, len);
  r->width = width;
  r->height = height;
  r->format = format;
  r->dpi = dpi ? dpi : 300;
  r->g4 = false;
  r->rows_per_strip = l.rows_per_strip;
  return true;
}

bool g4_record(const char* who, const uint8_t* data, size_t len, int32_t width, int32_t height, int32_t dpi,
               Writer::PageRec* r) {
  if (!data || !len) return fail("%s: null or empty page", who);
  if (width <= 0 || height <= 0) return fail("%s: invalid size %dx%d", who, width, height);
  if (dpi < 0 || dpi > 1200) return fail("%s: dpi %d outside 0..1200", who, dpi);
  if ((uint64_t)len >= (uint64_t)kLimit) return fail("%s: a %zu-byte strip is beyond the 4 GiB limit of classic TIFF", who, len);
  r->counts.assign(1, (uint32_t)len);
  r->width = width;
  r->height = height;
  r->format = UPHIP_FMT_MONOWHITE;
  r->dpi = dpi ? dpi : 300;
  r->g4 = true;
  r->rows_per_strip = height;
  return true;
}

void header(std::vector<uint8_t>* f, uint32_t first_ifd) {
  Bytes b{*f};
  b.u16(0x4949);
  b.u16(42);
  b.u32(first_ifd);
}

}  // namespace

bool g4_file(const uint8_t* p, size_t n, int32_t w, int32_t h, int32_t dpi, std::vector<uint8_t>* out) {
  Writer::PageRec r;
  if (!g4_record("tiff_g4", p, n, w, h, dpi, &r)) return false;
  out->clear();
  header(out, 8);
  std::vector<uint8_t> ifd;
  build_ifd(r, 8, 0, 0, 0, &ifd);  // sized first: the strip follows the IFD's values
  r.data = 8 + (uint32_t)ifd.size();
  if ((int64_t)r.data + (int64_t)n >= kLimit)
    return fail("tiff_g4: a %zu-byte strip is beyond the 4 GiB limit of classic TIFF", n);
  build_ifd(r, 8, 0, 0, 0, out);
  out->insert(out->end(), p, p + n);
  return true;
}

bool deflate_file(const uint8_t* blob, size_t n, int32_t w, int32_t h, int32_t format, int32_t dpi,
                  std::vector<uint8_t>* out) {
  Writer::PageRec r;
  if (!deflate_record("tiff_deflate", blob, n, w, h, format, dpi, &r)) return false;
  std::vector<uint8_t> ifd;
  r.data = 8;
  const int64_t at = (8 + (int64_t)n + 1) & ~(int64_t)1;
  build_ifd(r, (uint32_t)at, 0, 0, 0, &ifd);
  if (at + (int64_t)ifd.size() >= kLimit)
    return fail("tiff_deflate: a %zu-byte page is beyond the 4 GiB limit of classic TIFF", n);
  out->clear();
  out->reserve((size_t)at + ifd.size());
  header(out, (uint32_t)at);
  out->insert(out->end(), blob, blob + n);
  if (out->size() & 1) out->push_back(0);
  out->insert(out->end(), ifd.begin(), ifd.end());
  return true;
}

Writer::~Writer() { abort(); }

bool Writer::write_at(const void* p, size_t n, int64_t at) {
  const uint8_t* q = (const uint8_t*)p;
  size_t done = 0;
  while (done < n) {
    const ssize_t w = pwrite(fd_, q + done, n - done, (off_t)(at + (int64_t)done));
    if (w < 0) {
      if (errno == EINTR) continue;
      return fail("tiff_writer: cannot write %s: %s", part_.c_str(), strerror(errno));
    }
    done += (size_t)w;
  }
  return true;
}

bool Writer::create(const char* path, int32_t dpi) {
  std::lock_guard<std::mutex> lk(mu_);
  if (!path || !*path) return fail("tiff_writer: null path");
  if (fd_ >= 0) return fail("tiff_writer: already open");
  if (dpi < 0 || dpi > 1200) return fail("tiff_writer: dpi %d outside 0..1200", dpi);
  path_ = path;
  part_ = path_ + ".part";
  dpi_ = dpi ? dpi : 300;
  fd_ = ::open(part_.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
  if (fd_ < 0) return fail("tiff_writer: cannot create %s: %s", part_.c_str(), strerror(errno));
  std::vector<uint8_t> h;
  header(&h, 0);  // finish() patches the first IFD's offset
  pos_ = (int64_t)h.size();
  return write_at(h.data(), h.size(), 0);
}

// The page's data appended on an even offset (the pad byte before it stays a
// hole of the file, which reads as zero) and its record kept.  Every offset
// the page adds, its IFD's included (written by finish() after all data, so
// the IFDs of the pages taken so far count too), stays below the limit; a
// page that would not is refused, as is one whose write fails, and the file
// stays as it was: the next page takes the same place.
bool Writer::add(PageRec&& rec, const uint8_t* data, size_t len) {
  std::lock_guard<std::mutex> lk(mu_);
  if (fd_ < 0) return fail("tiff_writer: the writer is finished or was never opened");
  if (rec.index < 0) return fail("tiff_writer: page index %lld", (long long)rec.index);
  for (const PageRec& p : pages_)
    if (p.index == rec.index) return fail("tiff_writer: page %lld was added before", (long long)rec.index);
  std::vector<uint8_t> ifd;
  build_ifd(rec, 0, 1, 2, 0, &ifd);  // its size in a file of many pages
  const int64_t at = (pos_ + 1) & ~(int64_t)1;
  const int64_t ifd_room = ((int64_t)ifd.size() + 1) & ~(int64_t)1;
  if (at + (int64_t)len + 1 + ifd_bytes_ + ifd_room >= kLimit)
    return fail("tiff_writer: page %lld (%zu bytes) would put the file beyond the 4 GiB limit of classic TIFF",
                (long long)rec.index, len);
  if (!write_at(data, len, at)) return false;
  pos_ = at + (int64_t)len;
  rec.data = (uint32_t)at;
  rec.len = (uint32_t)len;
  ifd_bytes_ += ifd_room;
  if (rec.index >= next_index_) next_index_ = rec.index + 1;
  pages_.push_back(std::move(rec));
  return true;
}

bool Writer::add_page_deflate(int64_t index, const uint8_t* blob, size_t len, int32_t width, int32_t height,
                              int32_t format, int32_t dpi) {
  PageRec r;
  r.index = index;
  return deflate_record("tiff_writer", blob, len, width, height, format, dpi ? dpi : dpi_, &r) &&
         add(std::move(r), blob, len);
}

bool Writer::add_page_g4(int64_t index, const uint8_t* data, size_t len, int32_t width, int32_t height,
                         int32_t dpi) {
  PageRec r;
  r.index = index;
  return g4_record("tiff_writer", data, len, width, height, dpi ? dpi : dpi_, &r) && add(std::move(r), data, len);
}

int64_t Writer::next_index() {
  std::lock_guard<std::mutex> lk(mu_);
  return next_index_;
}

int Writer::page_count() {
  std::lock_guard<std::mutex> lk(mu_);
  return (int)pages_.size();
}

bool Writer::finish() {
  std::lock_guard<std::mutex> lk(mu_);
  if (fd_ < 0) return fail("tiff_writer: the writer is finished or was never opened");
  bool ok = true;
  if (pages_.empty()) ok = fail("tiff_writer: %s has no pages", path_.c_str());
  std::stable_sort(pages_.begin(), pages_.end(), [](const PageRec& a, const PageRec& b) { return a.index < b.index; });
  const uint32_t count = pages_.size() > 1 ? (uint32_t)pages_.size() : 0;
  const uint32_t first = (uint32_t)((pos_ + 1) & ~(int64_t)1);  // a pad byte stays a hole: it reads as zero
  std::vector<uint8_t> ifds;
  for (size_t k = 0; ok && k < pages_.size(); k++) {
    const uint32_t at = first + (uint32_t)ifds.size();
    std::vector<uint8_t> one;
    build_ifd(pages_[k], at, (uint32_t)k, count, 0, &one);
    if (one.size() & 1) one.push_back(0);
    if (k + 1 < pages_.size()) {  // the link, after the entries
      const uint32_t next = at + (uint32_t)one.size();
      const size_t link = 2 + 12 * (size_t)(one[0] | one[1] << 8);
      for (int b = 0; b < 4; b++) one[link + (size_t)b] = (uint8_t)(next >> (8 * b));
    }
    ifds.insert(ifds.end(), one.begin(), one.end());
  }
  ok = ok && write_at(ifds.data(), ifds.size(), first);
  if (ok) {
    uint8_t o[4];
    for (int b = 0; b < 4; b++) o[b] = (uint8_t)(first >> (8 * b));
    ok = write_at(o, 4, 4);
  }
  if (::close(fd_) != 0 && ok) ok = fail("tiff_writer: cannot close %s: %s", part_.c_str(), strerror(errno));
  fd_ = -1;
  if (ok && rename(part_.c_str(), path_.c_str()) != 0)
    ok = fail("tiff_writer: cannot rename %s: %s", part_.c_str(), strerror(errno));
  if (!ok) unlink(part_.c_str());
  return ok;
}

void Writer::abort() {
  std::lock_guard<std::mutex> lk(mu_);
  if (fd_ < 0) return;
  ::close(fd_);
  fd_ = -1;
  unlink(part_.c_str());
}

}  // namespace tiff
}  // namespace uph

using namespace uph;

struct UphipTiffWriter {
  tiff::Writer w;
};

namespace uph {
namespace tiffenc {
// The file of a coded page into the caller's buffer, sizes as uphip_png_encode.
int64_t give_file(const char* who, const std::vector<uint8_t>& file, void* out, int64_t capacity) {
  const int64_t size = (int64_t)file.size();
  if (!out) return size;
  if (capacity < size)
    return fail("%s: the file needs %lld bytes, the buffer has %lld", who, (long long)size, (long long)capacity), -1;
  memcpy(out, file.data(), file.size());
  return size;
}
}  // namespace tiffenc
}  // namespace uph

extern "C" {

int64_t uphip_tiff_encode_host(const void* pixels, int64_t stride, int32_t offset, int32_t width, int32_t height,
                               int32_t format, int32_t dpi, void* out, int64_t capacity) {
  tiffenc::Layout l;
  bool bilevel = false;
  if (!tiffenc::check_image("tiff_encode_host", pixels, stride, offset, width, height, format, dpi, &l, &bilevel))
    return -1;
  std::vector<uint8_t> data, file;
  if (bilevel) {
    if (!ccitt::encode((const uint8_t*)pixels, stride, offset, width, height, &data) ||
        !tiff::g4_file(data.data(), data.size(), width, height, dpi ? dpi : 300, &file))
      return -1;
  } else {
    tiffenc::encode_page_host((const uint8_t*)pixels, stride, l, &data);
    if (!tiff::deflate_file(data.data(), data.size(), width, height, format, dpi, &file)) return -1;
  }
  return tiffenc::give_file("tiff_encode_host", file, out, capacity);
}

UphipTiffWriter* uphip_tiff_writer_open(const char* path, int32_t dpi) {
  UphipTiffWriter* w = new UphipTiffWriter();
  if (!w->w.create(path, dpi)) {
    delete w;
    return nullptr;
  }
  return w;
}

int uphip_tiff_writer_add_page_deflate(UphipTiffWriter* w, int64_t index, const uint8_t* blob, size_t len,
                                       int32_t width, int32_t height, int32_t format, int32_t dpi) {
  if (!w) return fail("tiff_writer: null writer"), -1;
  return w->w.add_page_deflate(index < 0 ? w->w.next_index() : index, blob, len, width, height, format, dpi) ? 0 : -1;
}

int uphip_tiff_writer_add_page_g4(UphipTiffWriter* w, int64_t index, const uint8_t* data, size_t len, int32_t width,
                                  int32_t height, int32_t dpi) {
  if (!w) return fail("tiff_writer: null writer"), -1;
  return w->w.add_page_g4(index < 0 ? w->w.next_index() : index, data, len, width, height, dpi) ? 0 : -1;
}

int uphip_tiff_writer_finish(UphipTiffWriter* w) {
  if (!w) return fail("tiff_writer: null writer"), -1;
  return w->w.finish() ? 0 : -1;
}

void uphip_tiff_writer_close(UphipTiffWriter* w) { delete w; }

}  // extern "C"
