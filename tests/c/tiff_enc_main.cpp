// tiff_enc_main.cpp — the TIFF Deflate encoder's host twin and the container
// writer (csrc/tiff_write.cpp over csrc/tiff_enc_core.h) run stand-alone under
// ASan/UBSan (make sanitize_tiff_enc): every image is encoded from a heap
// buffer of exactly the bytes it may read and read back through the project's
// TIFF reader (csrc/tiff.cpp); then all pages go into one multi-page file,
// shuffled, and come back in order.
#include <unistd.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "runtime.h"
#include "tiff.h"
#include "tiff_enc_core.h"
#include "unpaper_hip.h"

// the library's error reporting, which the sources under test call
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
  fprintf(stderr, "tiff_enc_main: %s failed (format %d, %dx%d): %s\n", what, fmt, w, h, uph::g_error);
}

struct Case {
  int fmt, w, h;
  int64_t stride;
  std::vector<uint8_t> px;    // rows `stride` apart, the last one ending with its last pixel
  std::vector<uint8_t> page;  // the packed page inside the encoded file
};
std::vector<Case> g_cases;

// The file's pages through the reader against the cases' pixels.
void read_back(const std::vector<uint8_t>& file, const std::vector<const Case*>& want, const char* what) {
  uph::tiff::Document doc;
  std::vector<uint8_t> copy(file);
  if (!uph::tiff::open(std::move(copy), what, &doc) || doc.pages.size() != want.size())
    return check(false, what, 0, (int)doc.pages.size(), (int)want.size());
  for (size_t i = 0; i < want.size(); i++) {
    const Case& c = *want[i];
    const bool mono = c.fmt == UPHIP_FMT_MONOWHITE;
    const int64_t rb = mono ? (c.w + 7) / 8 : (int64_t)c.w * (c.fmt == UPHIP_FMT_RGB24 ? 3 : c.fmt == UPHIP_FMT_Y400A ? 2 : 1);
    std::vector<uint8_t> got((size_t)(rb * c.h));
    const UphipPnmInfo expect{c.w, c.h, c.fmt};
    if (!uph::tiff::read_page(doc, (int64_t)i, got.data(), rb, &expect)) {
      check(false, what, c.fmt, c.w, c.h);
      continue;
    }
    bool same = true;
    for (int y = 0; y < c.h && same; y++)
      if (mono) {
        for (int x = 0; x < c.w && same; x++)
          same = ((got[(size_t)(y * rb + (x >> 3))] ^ c.px[(size_t)(y * c.stride + (x >> 3))]) & (0x80 >> (x & 7))) == 0;
      } else {
        same = memcmp(&got[(size_t)(y * rb)], &c.px[(size_t)(y * c.stride)], (size_t)rb) == 0;
      }
    check(same, what, c.fmt, c.w, c.h);
  }
}

// kind: 0 text-like, 1 noise, 2 flat, 3 equal rows
void run_case(int fmt, int w, int h, int kind, int slack) {
  Case c;
  c.fmt = fmt, c.w = w, c.h = h;
  const bool mono = fmt == UPHIP_FMT_MONOWHITE;
  const int64_t rb = mono ? (w + 7) / 8 : (int64_t)w * (fmt == UPHIP_FMT_RGB24 ? 3 : fmt == UPHIP_FMT_Y400A ? 2 : 1);
  c.stride = rb + slack;
  c.px.resize((size_t)(c.stride * (h - 1) + rb));
  for (size_t i = 0; i < c.px.size(); i++) {
    const size_t x = i % (size_t)c.stride, y = i / (size_t)c.stride;
    uint8_t v = kind == 1 ? (uint8_t)rnd() : kind == 2 ? 0xFF : (rnd() % 5 ? 0xF0 : (uint8_t)rnd());
    if (kind == 3 && y > 0) v = c.px[x];
    c.px[i] = v;
  }
  const int64_t need = uphip_tiff_encode_host(c.px.data(), c.stride, 0, w, h, fmt, 300, nullptr, 0);
  if (need <= 0) return check(false, "sizing", fmt, w, h);
  std::vector<uint8_t> file((size_t)need);
  if (uphip_tiff_encode_host(c.px.data(), c.stride, 0, w, h, fmt, 300, file.data(), need) != need)
    return check(false, "encode", fmt, w, h);
  read_back(file, {&c}, "single page");
  if (!mono) {
    uph::tiffenc::Layout l;
    uph::tiffenc::layout_of(fmt, w, h, &l);
    // the strips lie between the header and the IFD, which the header names
    const uint32_t ifd = (uint32_t)file[4] | file[5] << 8 | file[6] << 16 | (uint32_t)file[7] << 24;
    size_t end = 8 + 4 * (size_t)l.nstrips;
    for (int k = 0; k < l.nstrips; k++) {
      const uint8_t* p = &file[8 + 4 * (size_t)k];
      const uint32_t n = (uint32_t)p[0] | p[1] << 8 | p[2] << 16 | (uint32_t)p[3] << 24;
      check((int64_t)n <= uph::pngenc::stored_size(uph::tiffenc::strip_total(l, k)), "stored bound", fmt, w, h);
      end += n;
    }
    check(((end + 1) & ~(size_t)1) == ifd && (int64_t)end - 8 <= uph::tiffenc::blob_bound(l), "page extent", fmt, w, h);
    c.page.assign(file.begin() + 8, file.begin() + (long)end);
  } else {
    const int64_t n = uphip_g4_encode_host(c.px.data(), c.stride, 0, w, h, nullptr, 0);
    c.page.resize(n > 0 ? (size_t)n : 0);
    check(n > 0 && uphip_g4_encode_host(c.px.data(), c.stride, 0, w, h, c.page.data(), n) == n, "group 4", fmt, w, h);
  }
  g_cases.push_back(std::move(c));
}

}  // namespace

int main() {
  const int formats[3] = {UPHIP_FMT_GRAY8, UPHIP_FMT_RGB24, UPHIP_FMT_Y400A};
  for (int fmt : formats) {
    for (int w : {1, 2, 3, 85, 86, 87, 255, 256, 257})
      for (int h : {1, 2, 65})
        for (int kind = 0; kind < 4; kind++) run_case(fmt, w, h, kind, kind == 1 ? 3 : 0);
    run_case(fmt, 203, 131, 0, 1);
  }
  // the strip rule's edges: one strip, an exact multiple, a shorter last strip
  for (int rb : {255, 256, 257}) {
    const int rps = 65536 / rb;
    run_case(UPHIP_FMT_GRAY8, rb, 2 * rps, 0, 0);
    run_case(UPHIP_FMT_GRAY8, rb, 2 * rps + 3, 3, 2);
  }
  run_case(UPHIP_FMT_GRAY8, 100, 65536 / 100 + 1, 0, 0);  // a last strip shorter than a segment
  run_case(UPHIP_FMT_GRAY8, 70000, 3, 3, 0);              // a row a strip, no row-distance candidate
  run_case(UPHIP_FMT_GRAY8, 32769, 4, 3, 0);
  run_case(UPHIP_FMT_RGB24, 85, 65536 / 255 + 40, 3, 0);  // equal rows across a strip boundary
  run_case(UPHIP_FMT_GRAY8, 256, 768, 1, 0);              // stored strips
  run_case(UPHIP_FMT_MONOWHITE, 203, 57, 0, 1);
  const int cases = (int)g_cases.size();

  // one file of all the pages, added in a shuffled order, one index left out
  char dir[] = "/tmp/tiff_enc_main_XXXXXX";
  if (!mkdtemp(dir)) return fprintf(stderr, "tiff_enc_main: no temporary directory\n"), 1;
  const std::string path = std::string(dir) + "/all.tif";
  UphipTiffWriter* w = uphip_tiff_writer_open(path.c_str(), 0);
  check(w != nullptr, "writer open", 0, 0, 0);
  std::vector<size_t> order(g_cases.size());
  for (size_t i = 0; i < order.size(); i++) order[i] = i;
  for (size_t i = order.size(); i > 1; i--) std::swap(order[i - 1], order[rnd() % i]);
  const size_t skipped = g_cases.size() / 2;
  std::vector<const Case*> want;
  for (size_t i = 0; i < g_cases.size(); i++)
    if (i != skipped) want.push_back(&g_cases[i]);
  for (size_t i : order) {
    const Case& c = g_cases[i];
    if (!w || i == skipped) continue;
    const int rc = c.fmt == UPHIP_FMT_MONOWHITE
                       ? uphip_tiff_writer_add_page_g4(w, (int64_t)i, c.page.data(), c.page.size(), c.w, c.h, 0)
                       : uphip_tiff_writer_add_page_deflate(w, (int64_t)i, c.page.data(), c.page.size(), c.w, c.h,
                                                            c.fmt, 0);
    check(rc == 0, "add page", c.fmt, c.w, c.h);
  }
  if (w) {
    check(uphip_tiff_writer_finish(w) == 0, "finish", 0, 0, 0);
    uphip_tiff_writer_close(w);
    std::vector<uint8_t> file;
    check(uph::tiff::read_file(path.c_str(), &file), "read the file back", 0, 0, 0);
    read_back(file, want, "multi-page");
  }
  // an unfinished writer leaves no file
  const std::string gone = std::string(dir) + "/gone.tif";
  w = uphip_tiff_writer_open(gone.c_str(), 0);
  if (w) {
    const Case& c = g_cases[0];
    check(uphip_tiff_writer_add_page_deflate(w, -1, c.page.data(), c.page.size(), c.w, c.h, c.fmt, 0) == 0,
          "add page", c.fmt, c.w, c.h);
    uphip_tiff_writer_close(w);
  }
  check(access(gone.c_str(), F_OK) != 0 && access((gone + ".part").c_str(), F_OK) != 0, "unfinished writer", 0, 0, 0);
  unlink(path.c_str());
  rmdir(dir);

  // argument errors leave through the error path
  uint8_t one[4] = {0, 0, 0, 0};
  if (uphip_tiff_encode_host(nullptr, 1, 0, 1, 1, UPHIP_FMT_GRAY8, 0, nullptr, 0) != -1 ||
      uphip_tiff_encode_host(one, 1, 1, 1, 1, UPHIP_FMT_GRAY8, 0, nullptr, 0) != -1 ||
      uphip_tiff_encode_host(one, 1, 0, 1, 1, 99, 0, nullptr, 0) != -1 ||
      uphip_tiff_encode_host(one, 1, 0, 1, 1, UPHIP_FMT_MONOBLACK, 0, nullptr, 0) != -1 ||
      uphip_tiff_encode_host(one, 1, 0, 1, 1, UPHIP_FMT_GRAY8, 0, one, 1) != -1 ||
      uphip_tiff_writer_add_page_deflate(nullptr, 0, one, 4, 1, 1, UPHIP_FMT_GRAY8, 0) != -1)
    check(false, "argument errors", 0, 1, 1);
  if (g_failures) {
    fprintf(stderr, "tiff_enc_main: %d failures in %d cases\n", g_failures, cases);
    return 1;
  }
  printf("tiff_enc_main: ok (%d cases)\n", cases);
  return 0;
}
