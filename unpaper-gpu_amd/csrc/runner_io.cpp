// runner_io.cpp — the runner's sources and sinks (the C ABI's constructors)
// and the store side of a host-fed run: a finished chunk's sheets into the
// sink, raw or through the sink's codec.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "runner_internal.h"

using namespace uph;

namespace {

// The reference names output files with sprintf(buf, pattern, outputNr++)
// (image_pipeline.c:742): an int conversion such as "out%04d.pbm".  The
// pattern becomes a format string here, so it may hold at most one integer
// conversion (flags, width and precision kept, any length modifier replaced
// by ll to match the int64_t page number) and "%%"; anything else (%s, %n,
// a second conversion) is refused.
bool output_pattern(const char* p, std::string* out) {
  int nconv = 0;
  out->clear();
  for (const char* c = p; *c; c++) {
    if (*c != '%') {
      out->push_back(*c);
      continue;
    }
    if (c[1] == '%') {
      out->append("%%");
      c++;
      continue;
    }
    std::string spec = "%";
    const char* q = c + 1;
    while (*q && strchr("-+ #0", *q)) spec.push_back(*q++);
    while (*q >= '0' && *q <= '9') spec.push_back(*q++);
    if (*q == '.') {
      spec.push_back(*q++);
      while (*q >= '0' && *q <= '9') spec.push_back(*q++);
    }
    while (*q && strchr("hljzt", *q)) q++;  // length modifiers: replaced below
    if (!*q || !strchr("diuoxX", *q))
      return fail("sink_pnm: pattern \"%s\": only one integer conversion (%%d, %%05d, ...) "
                  "is allowed", p);
    if (++nconv > 1) return fail("sink_pnm: pattern \"%s\" has more than one conversion", p);
    spec.append("ll");
    spec.push_back(*q);
    out->append(spec);
    c = q;
  }
  return true;
}

// A Group 4 stream of a w x h page as a TIFF file of its own (tiff::g4_file).
bool write_tiff_g4(const std::string& path, const uint8_t* p, size_t n, int32_t w, int32_t h, int32_t dpi) {
  std::vector<uint8_t> f;
  if (!tiff::g4_file(p, n, w, h, dpi, &f)) return false;
  FILE* o = fopen(path.c_str(), "wb");
  if (!o) return fail("tiff_g4: cannot create %s", path.c_str());
  const bool ok = fwrite(f.data(), 1, f.size(), o) == f.size();
  return (fclose(o) == 0 && ok) || fail("tiff_g4: cannot write %s", path.c_str());
}

// A sink of numbered files: `what` names the constructor in its errors.
UphipSink* file_sink(const char* what, const char* pattern, int64_t wrap, UphipSink::Codec codec) {
  if (!pattern) return fail("%s: null pattern", what), nullptr;
  std::string fmt;
  if (!output_pattern(pattern, &fmt)) return nullptr;
  UphipSink* k = new UphipSink();
  k->pattern = fmt;
  k->wrap = wrap;
  k->codec = codec;
  return k;
}

bool dpi_ok(const char* what, int32_t dpi) {
  return (dpi >= 0 && dpi <= 1200) || fail("%s: dpi %d outside 0..1200", what, dpi);
}

// The sink's PDF, opened: the caller's metadata copied, 300 dpi by default
// (PDF_RENDER_DPI, pdf_pipeline_cpu_batch.c:41).
std::unique_ptr<pdf::Writer> make_pdf_writer(const char* path, const UphipPdfMetadata* meta, int32_t dpi) {
  pdf::Meta m;
  if (meta) {
    const char* f[8] = {meta->title,   meta->author,   meta->subject,       meta->keywords,
                        meta->creator, meta->producer, meta->creation_date, meta->modification_date};
    std::string* o[8] = {&m.title,   &m.author,   &m.subject,       &m.keywords,
                         &m.creator, &m.producer, &m.creation_date, &m.modification_date};
    for (int i = 0; i < 8; i++)
      if (f[i]) {
        *o[i] = f[i];
        m.has[i] = true;
      }
  }
  std::unique_ptr<pdf::Writer> w(new pdf::Writer());
  if (!w->create(path, meta ? &m : nullptr, dpi ? dpi : 300)) return nullptr;
  return w;
}

UphipSink* pdf_sink(const char* path, const UphipPdfMetadata* meta, int32_t dpi, UphipSink::Codec codec) {
  std::unique_ptr<pdf::Writer> w = make_pdf_writer(path, meta, dpi);
  if (!w) return nullptr;
  UphipSink* k = new UphipSink();
  k->pdfw = std::move(w);
  k->pdf_dpi = dpi ? dpi : 300;
  k->codec = codec;
  return k;
}

}  // namespace

extern "C" {

UphipSource* uphip_source_callback(UphipLoadFn load, void* user) {
  if (!load) return fail("source_callback: null function"), nullptr;
  UphipSource* s = new UphipSource();
  s->load = load;
  s->user = user;
  return s;
}

UphipSource* uphip_source_memory(const void* base, int64_t linesize, int64_t page_stride,
                                 int64_t npages) {
  if (!base || npages <= 0) return fail("source_memory: bad arguments"), nullptr;
  UphipSource* s = new UphipSource();
  s->base = (const uint8_t*)base;
  s->linesize = linesize;
  s->page_stride = page_stride;
  s->npages = npages;
  return s;
}

UphipSource* uphip_source_pnm(const char* const* paths, int64_t npaths) {
  if (!paths || npaths <= 0) return fail("source_pnm: no files"), nullptr;
  UphipSource* s = new UphipSource();
  for (int64_t i = 0; i < npaths; i++) s->paths.emplace_back(paths[i] ? paths[i] : "");
  return s;
}

UphipSource* uphip_source_pdf(const char* path, int32_t dpi) {
  if (!path) return fail("source_pdf: null path"), nullptr;
  if (dpi < 0) return fail("source_pdf: dpi %d", dpi), nullptr;
  std::vector<uint8_t> bytes;
  if (!jpeg_read_file(path, &bytes)) return nullptr;
  auto doc = std::make_shared<pdf::Document>();
  if (!doc->open(std::move(bytes), path)) return nullptr;
  if (doc->encrypted()) return fail("source_pdf: %s is encrypted (decryption is not supported)", path), nullptr;
  if (doc->page_count() <= 0) return fail("source_pdf: %s has no pages", path), nullptr;
  UphipSource* s = new UphipSource();
  s->pdf = std::move(doc);
  s->pdf_dpi = dpi;
  return s;
}

UphipSource* uphip_source_tiff(const char* path, int32_t flags) {
  if (!path) return fail("source_tiff: null path"), nullptr;
  if ((flags & ~(UPHIP_TIFF_HOST_DECODE | UPHIP_TIFF_DEVICE_DECODE)) ||
      flags == (UPHIP_TIFF_HOST_DECODE | UPHIP_TIFF_DEVICE_DECODE))
    return fail("source_tiff: flags %d", flags), nullptr;
  auto doc = std::make_shared<tiff::Document>();
  if (!tiff::open_file(path, doc.get())) return nullptr;
  UphipSource* s = new UphipSource();
  s->tiff = std::move(doc);
  s->tiff_flags = flags;
  return s;
}

int64_t uphip_source_page_count(UphipSource* s) {
  if (!s) return fail("source_page_count: null source"), -1;
  if (s->pdf) return s->pdf->page_count();
  if (s->tiff) return (int64_t)s->tiff->pages.size();
  if (s->base) return s->npages;
  if (!s->paths.empty()) return (int64_t)s->paths.size();
  return fail("source_page_count: a callback source has no page count"), -1;
}

int uphip_source_max_geometry(UphipSource* s, UphipPnmInfo* info) {
  if (!s || !info) return fail("source_max_geometry: null argument"), -1;
  if (s->load || s->base)
    return fail("source_max_geometry: callback and memory sources carry no page sizes"), -1;
  const int64_t n = uphip_source_page_count(s);
  if (n <= 0) return -1;
  UphipPnmInfo m{0, 0, 0};
  for (int64_t i = 0; i < n; i++) {
    UphipPnmInfo g{0, 0, 0};
    std::string name;
    if (!source_page_info(s, i, &g, &name)) return -1;
    if (i == 0) m.format = g.format;
    if (g.format != m.format)
      return fail("source_max_geometry: %s is of format %d, the pages before it of format %d (one run takes "
                  "one page format)", name.c_str(), g.format, m.format), -1;
    m.width = std::max(m.width, g.width);
    m.height = std::max(m.height, g.height);
  }
  *info = m;
  return 0;
}

void uphip_source_destroy(UphipSource* s) { delete s; }

UphipSink* uphip_sink_callback(UphipStoreFn store, void* user) {
  if (!store) return fail("sink_callback: null function"), nullptr;
  UphipSink* k = new UphipSink();
  k->store = store;
  k->user = user;
  return k;
}

UphipSink* uphip_sink_memory(void* base, int64_t linesize, int64_t sheet_stride, int64_t nsheets) {
  if (!base || nsheets <= 0) return fail("sink_memory: bad arguments"), nullptr;
  UphipSink* k = new UphipSink();
  k->base = (uint8_t*)base;
  k->linesize = linesize;
  k->sheet_stride = sheet_stride;
  k->nsheets = nsheets;
  return k;
}

UphipSink* uphip_sink_pnm(const char* pattern, int64_t wrap) {
  return file_sink("sink_pnm", pattern, wrap, UphipSink::Codec::Raw);
}

UphipSink* uphip_sink_jpeg(const char* pattern, int64_t wrap, int32_t quality, int32_t sampling) {
  if (!pattern) return fail("sink_jpeg: null pattern"), nullptr;
  if (quality == 0) quality = UPHIP_JPEG_DEFAULT_QUALITY;
  if (quality < 1 || quality > 100) return fail("sink_jpeg: quality %d outside 1..100", quality), nullptr;
  if (sampling < UPHIP_JPEG_444 || sampling > UPHIP_JPEG_420)
    return fail("sink_jpeg: unknown sampling %d", sampling), nullptr;
  UphipSink* k = file_sink("sink_jpeg", pattern, wrap, UphipSink::Codec::Jpeg);
  if (!k) return nullptr;
  k->quality = quality;
  k->sampling = sampling;
  return k;
}

UphipSink* uphip_sink_jp2(const char* pattern, int64_t wrap) {
  return file_sink("sink_jp2", pattern, wrap, UphipSink::Codec::Jp2);
}

UphipSink* uphip_sink_discard(void) { return new UphipSink(); }

UphipSink* uphip_sink_pdf(const char* path, const UphipPdfMetadata* meta, int32_t dpi, int32_t quality,
                          int32_t mode) {
  if (!path) return fail("sink_pdf: null path"), nullptr;
  if (mode != UPHIP_PDF_FAST && mode != UPHIP_PDF_HIGH) return fail("sink_pdf: unknown mode %d", mode), nullptr;
  if (quality == 0) quality = UPHIP_JPEG_DEFAULT_QUALITY;
  if (quality < 1 || quality > 100) return fail("sink_pdf: quality %d outside 1..100", quality), nullptr;
  if (!dpi_ok("sink_pdf", dpi)) return nullptr;
  UphipSink* k = pdf_sink(path, meta, dpi, mode == UPHIP_PDF_HIGH ? UphipSink::Codec::Jp2 : UphipSink::Codec::Jpeg);
  if (!k) return nullptr;
  k->quality = quality;
  k->sampling = UPHIP_JPEG_444;
  return k;
}

UphipSink* uphip_sink_tiff_g4(const char* pattern, int64_t wrap, int32_t dpi) {
  if (!pattern) return fail("sink_tiff_g4: null pattern"), nullptr;
  if (!dpi_ok("sink_tiff_g4", dpi)) return nullptr;
  UphipSink* k = file_sink("sink_tiff_g4", pattern, wrap, UphipSink::Codec::G4);
  if (k) k->pdf_dpi = dpi ? dpi : 300;
  return k;
}

UphipSink* uphip_sink_pdf_bilevel(const char* path, const UphipPdfMetadata* meta, int32_t dpi) {
  if (!path) return fail("sink_pdf_bilevel: null path"), nullptr;
  if (!dpi_ok("sink_pdf_bilevel", dpi)) return nullptr;
  return pdf_sink(path, meta, dpi, UphipSink::Codec::G4);
}

UphipSink* uphip_sink_png(const char* pattern, int64_t wrap, int32_t dpi) {
  if (!pattern) return fail("sink_png: null pattern"), nullptr;
  if (!dpi_ok("sink_png", dpi)) return nullptr;
  UphipSink* k = file_sink("sink_png", pattern, wrap, UphipSink::Codec::Png);
  if (k) k->png_dpi = dpi;
  return k;
}

UphipSink* uphip_sink_tiff(const char* pattern, int64_t wrap, int32_t dpi) {
  if (!pattern) return fail("sink_tiff: null pattern"), nullptr;
  if (!dpi_ok("sink_tiff", dpi)) return nullptr;
  UphipSink* k = file_sink("sink_tiff", pattern, wrap, UphipSink::Codec::Tiff);
  if (k) k->pdf_dpi = dpi ? dpi : 300;
  return k;
}

UphipSink* uphip_sink_tiff_multipage(const char* path, int32_t dpi) {
  if (!path) return fail("sink_tiff_multipage: null path"), nullptr;
  if (!dpi_ok("sink_tiff_multipage", dpi)) return nullptr;
  std::unique_ptr<tiff::Writer> w(new tiff::Writer());
  if (!w->create(path, dpi)) return nullptr;
  UphipSink* k = new UphipSink();
  k->tiffw = std::move(w);
  k->pdf_dpi = dpi ? dpi : 300;
  k->codec = UphipSink::Codec::Tiff;
  return k;
}

UphipSink* uphip_sink_pdf_lossless(const char* path, const UphipPdfMetadata* meta, int32_t dpi) {
  if (!path) return fail("sink_pdf_lossless: null path"), nullptr;
  if (!dpi_ok("sink_pdf_lossless", dpi)) return nullptr;
  return pdf_sink(path, meta, dpi, UphipSink::Codec::Png);  // the bilevel sink's writer; the pages differ
}

int uphip_tiff_g4_write(const char* path, const uint8_t* data, size_t len, int32_t width, int32_t height,
                        int32_t dpi) {
  if (!path || !data || !len) return fail("tiff_g4_write: null argument"), -1;
  if (width <= 0 || height <= 0) return fail("tiff_g4_write: invalid size %dx%d", width, height), -1;
  if (!dpi_ok("tiff_g4_write", dpi)) return -1;
  return write_tiff_g4(path, data, len, width, height, dpi ? dpi : 300) ? 0 : -1;
}

int uphip_sink_finish(UphipSink* k) {
  if (!k) return fail("sink_finish: null sink"), -1;
  if (k->tiffw) {
    const bool ok = k->tiffw->finish();
    k->tiffw.reset();
    return ok ? 0 : -1;
  }
  if (!k->pdfw) return 0;
  const bool ok = k->pdfw->close();
  k->pdfw.reset();
  return ok ? 0 : -1;
}

void uphip_sink_destroy(UphipSink* k) { delete k; }

}  // extern "C"

// ---------------------------------------------------------------------------
// the store side
// ---------------------------------------------------------------------------
namespace {

// The file of output page `idx` (job * output_count + page) of a pattern sink.
std::string sink_path(const UphipSink* k, int64_t idx) {
  if (k->wrap > 0) idx %= k->wrap;
  char path[4096];
  // the pattern holds at most one ll integer conversion (output_pattern)
#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Wformat-nonliteral"
  snprintf(path, sizeof(path), k->pattern.c_str(), (long long)idx);
#pragma GCC diagnostic pop
  return path;
}

// A sheet as it left the pipeline: to the callback, the caller's memory or
// one PNM file per output page.
void store_sheet(UphipRunner* r, const UphipSink* k, int64_t job, const uint8_t* sheet, bool* ok) {
  const int oc = r->oc;
  if (k->store) {
    if (k->store(k->user, job, sheet, r->out_linesize, r->out_w, r->out_h, r->out_fmt) != 0) *ok = false;
    return;
  }
  const int64_t rb = row_bytes(r->out_w, r->out_fmt);
  if (k->base) {
    if (job < 0 || job >= k->nsheets) {
      *ok = fail("sink_memory: sheet %lld out of range", (long long)job);
      return;
    }
    uint8_t* d = k->base + job * k->sheet_stride;
    for (int32_t y = 0; y < r->out_h; y++)
      memcpy(d + (int64_t)y * k->linesize, sheet + (int64_t)y * r->out_linesize, (size_t)rb);
    return;
  }
  if (k->pattern.empty()) return;  // discard
  // output pages side by side in the sheet (sheet_stages.c:606-624)
  const int32_t pw = r->out_w / oc;
  const int64_t prb = row_bytes(pw, r->out_fmt);
  std::vector<uint8_t> tmp;
  for (int j = 0; j < oc; j++) {
    const uint8_t* src = sheet;
    int64_t ls = r->out_linesize;
    const bool mono = r->out_fmt == UPHIP_FMT_MONOWHITE || r->out_fmt == UPHIP_FMT_MONOBLACK;
    if (j > 0 || (oc > 1 && mono && (pw & 7))) {  // a page of its own (fresh padding bits)
      const int64_t x0 = (int64_t)j * pw;
      tmp.assign((size_t)(prb * r->out_h), 0);
      for (int32_t y = 0; y < r->out_h; y++) {
        const uint8_t* row = sheet + (int64_t)y * r->out_linesize;
        uint8_t* t = tmp.data() + (int64_t)y * prb;
        if (mono) {
          for (int32_t x = 0; x < pw; x++) {
            const int64_t sx = x0 + x;
            if (row[sx >> 3] & (0x80 >> (sx & 7))) t[x >> 3] |= (uint8_t)(0x80 >> (x & 7));
          }
        } else {
          const int64_t bpp = row_bytes(1, r->out_fmt);
          memcpy(t, row + x0 * bpp, (size_t)prb);
        }
      }
      src = tmp.data();
      ls = prb;
    }
    if (uphip_pnm_write(sink_path(k, job * oc + j).c_str(), src, ls, pw, r->out_h, r->out_fmt) != 0) *ok = false;
  }
}

bool write_file(const std::string& path, const uint8_t* p, size_t n) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) return fail("sink_jpeg: cannot create %s", path.c_str());
  const bool ok = fwrite(p, 1, n, f) == n;
  return (fclose(f) == 0 && ok) || fail("sink_jpeg: cannot write %s", path.c_str());
}

// A packed page of the slot's chunk: its bytes in the download, its size
// (-1: larger than its share of the batch's encode buffer) and where it goes.
struct PackedPage {
  int i;         // page of the chunk
  int64_t idx;   // output page of the run
  const uint8_t* data;
  int64_t size;
  PackedPage(const UphipRunner* r, const Slot* sl, int s, int j)
      : i(s * r->oc + j), idx((sl->first + s) * r->oc + j), data(sl->hjpg.as() + sl->joff[(size_t)i]),
        size(sl->jsize[(size_t)i]) {}
};

// A JPEG page the batch's encode buffers could not hold is encoded again on
// its own, on the device, from the batch's sheet.
bool store_jpeg_page(UphipRunner* r, const UphipSink* k, int device, const Slot* sl, int s, int j) {
  const PackedPage p(r, sl, s, j);
  if (p.size > 0) return sink_write(k, p.idx, p.data, (size_t)p.size);
  const void* src = nullptr;
  int64_t pitch = 0;
  int32_t w = 0, h = 0, fmt = 0;
  if (uphip_set_device(device) != 0 || uphip_batch_jpeg_page(sl->b, p.i, &src, &pitch, &w, &h, &fmt) != 0)
    return false;
  const int64_t n = uphip_jpeg_encode(src, pitch, w, h, fmt, k->quality, k->sampling, nullptr, 0);
  std::vector<uint8_t> file(n > 0 ? (size_t)n : 0);
  return n > 0 && uphip_jpeg_encode(src, pitch, w, h, fmt, k->quality, k->sampling, file.data(), n) == n &&
         sink_write(k, p.idx, file.data(), file.size());
}

// As store_jpeg_page: a Group 4 page larger than its share is coded again on
// its own from the batch's sheet.
bool store_g4_page(UphipRunner* r, const UphipSink* k, int device, const Slot* sl, int s, int j) {
  const PackedPage p(r, sl, s, j);
  const int32_t pw = r->out_w / r->oc;
  if (p.size > 0) return sink_write(k, p.idx, p.data, (size_t)p.size, pw, r->out_h);
  int64_t pitch = 0;
  const void* src = uphip_set_device(device) == 0 ? uphip_batch_output_ptr(sl->b, s, &pitch) : nullptr;
  if (!src) return false;
  const int64_t n = uphip_g4_encode(src, pitch, j * pw, pw, r->out_h, nullptr, 0);
  std::vector<uint8_t> file(n > 0 ? (size_t)n : 0);
  return n > 0 && uphip_g4_encode(src, pitch, j * pw, pw, r->out_h, file.data(), n) == n &&
         sink_write(k, p.idx, file.data(), file.size(), pw, r->out_h);
}

// A lossless page: its zlib stream into its PNG file or its page of the
// sink's PDF.  Every page has a size (uphip_batch_png_sizes refuses otherwise).
bool store_png_page(UphipRunner* r, const UphipSink* k, int, const Slot* sl, int s, int j) {
  const PackedPage p(r, sl, s, j);
  const int32_t pw = r->out_w / r->oc;
  if (p.size <= 0) return false;
  if (k->pdfw) {
    int comps = 0, bits = 0;
    return pdf::flate_layout(r->out_fmt, &comps, &bits) &&
           k->pdfw->add_page(p.idx, pdf::kPng, p.data, (size_t)p.size, pw, r->out_h, bits, comps, k->pdf_dpi);
  }
  const int64_t n = uphip_png_wrap(p.data, p.size, pw, r->out_h, r->out_fmt, k->png_dpi, nullptr, 0);
  std::vector<uint8_t> file(n > 0 ? (size_t)n : 0);
  return n > 0 && uphip_png_wrap(p.data, p.size, pw, r->out_h, r->out_fmt, k->png_dpi, file.data(), n) == n &&
         write_file(sink_path(k, p.idx), file.data(), file.size());
}

// A Deflate TIFF page: its packed page into the sink's file of many pages or
// a file of its own.
bool store_tiff_page(UphipRunner* r, const UphipSink* k, int, const Slot* sl, int s, int j) {
  const PackedPage p(r, sl, s, j);
  const int32_t pw = r->out_w / r->oc;
  if (p.size <= 0) return false;
  if (k->tiffw) return k->tiffw->add_page_deflate(p.idx, p.data, (size_t)p.size, pw, r->out_h, r->out_fmt, k->pdf_dpi);
  std::vector<uint8_t> file;
  return tiff::deflate_file(p.data, (size_t)p.size, pw, r->out_h, r->out_fmt, k->pdf_dpi, &file) &&
         write_file(sink_path(k, p.idx), file.data(), file.size());
}

constexpr PackedCodec kJpegCodec = {
    [](UphipBatch* b, const UphipSink* k) { return uphip_batch_encode_jpeg_async(b, k->quality, k->sampling); },
    uphip_batch_jpeg_sizes, uphip_batch_jpeg_download_async, store_jpeg_page};
constexpr PackedCodec kG4Codec = {[](UphipBatch* b, const UphipSink*) { return uphip_batch_encode_g4_async(b); },
                                  uphip_batch_g4_sizes, uphip_batch_g4_download_async, store_g4_page};
constexpr PackedCodec kPngCodec = {[](UphipBatch* b, const UphipSink*) { return uphip_batch_encode_png_async(b); },
                                   uphip_batch_png_sizes, uphip_batch_png_download_async, store_png_page};
constexpr PackedCodec kTiffCodec = {[](UphipBatch* b, const UphipSink*) { return uphip_batch_encode_tiff_async(b); },
                                    uphip_batch_tiff_sizes, uphip_batch_tiff_download_async, store_tiff_page};

// The pages of sheet s of a slot's chunk as JPEG 2000 files: each page's
// packed codewords from the device, its packets and boxes here.
void store_jp2_chunk_sheet(UphipRunner* r, const UphipSink* k, int device, const Slot* sl, int s, bool* ok) {
  thread_local std::vector<uint8_t> data, file;
  thread_local std::vector<uint32_t> off;
  const int oc = r->oc;
  if (*sl->hj2err) {
    *ok = fail("sink_jp2: code-blocks larger than the packing buffer");
    return;
  }
  const int J = sl->j2jobs;
  for (int j = 0; j < oc; j++)
    for (int q = 0; q < J; q++)
      if (sl->hj2nb[(size_t)(s * oc + j) * J + q] > 16) {
        *ok = fail("sink_jp2: a code-block's codeword outgrew its region");
        return;
      }
  for (int j = 0; j < oc; j++) {
    const int i = s * oc + j;
    const uint32_t* po = sl->hj2off + (size_t)i * J;
    const uint32_t base = po[0], end = po[J];
    data.resize((size_t)(end - base) + 1);
    off.resize((size_t)J);
    for (int q = 0; q < J; q++) off[(size_t)q] = po[q] - base;
    if (uphip_set_device(device) != 0 ||
        (end > base && !UPH_HIP(hipMemcpy(data.data(), sl->dj2pk + base, end - base, hipMemcpyDeviceToHost))) ||
        !j2k::encode_host_coded(sl->j2img, off.data(), sl->hj2len + (size_t)i * J, sl->hj2nb + (size_t)i * J,
                                data.data(), &file) ||
        !sink_write(k, (sl->first + s) * oc + j, file.data(), file.size()))
      *ok = false;
  }
}

}  // namespace

namespace uph {

const PackedCodec* packed_codec(const UphipSink* k, int32_t out_fmt) {
  switch (k->codec) {
    case UphipSink::Codec::Tiff: return out_fmt == UPHIP_FMT_MONOWHITE ? &kG4Codec : &kTiffCodec;
    case UphipSink::Codec::Jpeg: return &kJpegCodec;
    case UphipSink::Codec::G4: return &kG4Codec;
    case UphipSink::Codec::Png: return &kPngCodec;
    default: return nullptr;
  }
}

// An encoded output page `idx` (job * output_count + page): its file, or its
// page of the sink's PDF (the page accumulator's writes,
// pdf_page_accumulator.c:44-62; here straight from the store task, the
// writer orders the page tree).
bool sink_write(const UphipSink* k, int64_t idx, const uint8_t* p, size_t n, int32_t w, int32_t h) {
  if (k->tiffw) return k->tiffw->add_page_g4(idx, p, n, w, h, k->pdf_dpi);  // a Tiff sink's bilevel pages
  if (k->codec == UphipSink::Codec::G4 || k->codec == UphipSink::Codec::Tiff)
    // a Group 4 stream has no header: the caller gives the page's size
    return k->pdfw ? k->pdfw->add_page(idx, pdf::kCcitt, p, n, w, h, 0, 0, k->pdf_dpi)
                   : write_tiff_g4(sink_path(k, idx), p, n, w, h, k->pdf_dpi);
  if (!k->pdfw) return write_file(sink_path(k, idx), p, n);
  const bool jpeg = k->codec == UphipSink::Codec::Jpeg;
  UphipPnmInfo g{0, 0, 0};
  if (jpeg ? !jpeg_probe_mem(p, n, "output page", &g) : !j2k::probe(p, n, "output page", &g)) return false;
  return k->pdfw->add_page(idx, jpeg ? pdf::kJpeg : pdf::kJp2, p, n, g.width, g.height, 0, 0, k->pdf_dpi);
}

// Sheet s of a slot's finished chunk into the sink, through the sink's codec.
void store_chunk_sheet(UphipRunner* r, const UphipSink* k, int device, const Slot* sl, int s, bool* ok) {
  if (const PackedCodec* c = packed_codec(k, r->out_fmt)) {
    for (int j = 0; j < r->oc; j++)
      if (!c->store_page(r, k, device, sl, s, j)) *ok = false;
  } else if (k->codec == UphipSink::Codec::Jp2) {
    store_jp2_chunk_sheet(r, k, device, sl, s, ok);
  } else {
    store_sheet(r, k, sl->first + s, sl->hout.as() + (int64_t)s * r->out_sheet_stride, ok);
  }
}

}  // namespace uph
