// tiff.cpp — host TIFF reader: the TIFF third of the reference's loadImage
// (file.c:29-131), which opens any file through FFmpeg (README and
// doc/file-formats.md name PNG, JPEG and TIFF).  No libtiff: the container is
// parsed here, the strips go through tiff_strip.h (PackBits, LZW), zlib
// (Deflate) and ccitt.cpp (Group 3 / 4).
//
// Accepted: classic TIFF (magic 42) of either byte order, strips,
// PlanarConfiguration 1, BitsPerSample 1, 8, 8/8 (one extra sample), 8/8/8
// and 8 with a ColorMap; Photometric 0-3; SHORT or LONG offsets and counts.
//
//   1-bit, Photometric 0       -> MONOWHITE, bits as stored
//   1-bit, Photometric 1       -> MONOBLACK, bits as stored
//   8-bit gray                 -> GRAY8 (MinIsWhite: 255 - v)
//   gray + one extra sample    -> Y400A
//   8/8/8                      -> RGB24
//   palette                    -> RGB24 (loadImage's PAL8 case, file.c:110-120:
//                                 the high byte of every ColorMap entry)
//
// Which of the two equivalent 1-bit formats FFmpeg's TIFF decoder reports is
// unpinned (no FFmpeg where this was written); the bits are never changed, so
// MONOWHITE files written by uphip_tiff_g4_write read back as they were.
// Orientation is ignored: pixels come back as stored.
//
// Refused, each with the tag and its value in the error: BigTIFF, tiles,
// PlanarConfiguration 2, 2/4/16-bit samples, RGBA or more than one extra
// sample, YCbCr / CMYK / CIELab, any other compression.
#include "tiff.h"

#include <zlib.h>

#include <algorithm>
#include <cerrno>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>

#include "ccitt.h"
#include "runtime.h"

namespace uph {
namespace tiff {
namespace {

constexpr int64_t kMaxSide = 1 << 20;      // as the PNM and PNG readers
constexpr int64_t kMaxRaster = 1ll << 34;  // 3 * w * h, the PNG reader's cap
constexpr int kMaxIfds = 65535;
// no coder here expands by more (LZW with a full table: 2560; Deflate: 1032)
constexpr uint64_t kMaxExpansion = 4096;

struct File {
  const uint8_t* p;
  size_t n;
  bool be;
  uint32_t u16(size_t o) const { return be ? (uint32_t)p[o] << 8 | p[o + 1] : (uint32_t)p[o + 1] << 8 | p[o]; }
  uint32_t u32(size_t o) const { return be ? u16(o) << 16 | u16(o + 2) : u16(o + 2) << 16 | u16(o); }
  bool holds(uint64_t off, uint64_t len) const { return off <= n && len <= n - off; }
};

struct Entry {
  uint32_t tag, type, count;
  size_t at;  // of the value field
};

const char* tag_name(uint32_t tag) {
  switch (tag) {
    case 256: return "ImageWidth";
    case 257: return "ImageLength";
    case 258: return "BitsPerSample";
    case 259: return "Compression";
    case 262: return "PhotometricInterpretation";
    case 266: return "FillOrder";
    case 273: return "StripOffsets";
    case 277: return "SamplesPerPixel";
    case 278: return "RowsPerStrip";
    case 279: return "StripByteCounts";
    case 284: return "PlanarConfiguration";
    case 292: return "T4Options";
    case 296: return "ResolutionUnit";
    case 317: return "Predictor";
    case 320: return "ColorMap";
    case 338: return "ExtraSamples";
    default: return "tag";
  }
}

// The entry's values (BYTE, SHORT or LONG), at most `max` of them.
bool values(const File& f, const Entry& e, size_t max, std::vector<uint32_t>* out, std::string* err) {
  const uint32_t size = e.type == 1 ? 1 : e.type == 3 ? 2 : e.type == 4 ? 4 : 0;
  char msg[160];
  if (!size || e.count == 0 || e.count > max) {
    snprintf(msg, sizeof(msg), "%s (%u): type %u, count %u", tag_name(e.tag), e.tag, e.type, e.count);
    return *err = msg, false;
  }
  const uint64_t total = (uint64_t)e.count * size;
  size_t at = e.at;
  if (total > 4) {
    at = f.u32(e.at);
    if (!f.holds(at, total)) {
      snprintf(msg, sizeof(msg), "%s (%u): its %u values at offset %zu pass the end of the file", tag_name(e.tag),
               e.tag, e.count, at);
      return *err = msg, false;
    }
  }
  out->resize(e.count);
  for (uint32_t i = 0; i < e.count; i++)
    (*out)[i] = size == 1 ? f.p[at + i] : size == 2 ? f.u16(at + 2 * (size_t)i) : f.u32(at + 4 * (size_t)i);
  return true;
}

bool refuse(Page* pg, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
bool refuse(Page* pg, const char* fmt, ...) {
  char msg[200];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(msg, sizeof(msg), fmt, ap);
  va_end(ap);
  pg->error = msg;
  return false;
}

// One IFD at `ifd` (its entries lie inside the file) into `pg`.
bool parse_page(const File& f, size_t ifd, Page* pg) {
  const uint32_t n = f.u16(ifd);
  std::vector<uint32_t> v, bits{1}, offs, cnts, cmap, extra;
  bool have_w = false, have_h = false, have_rps = false, have_phot = false;
  uint32_t planar = 1, unit = 2;
  double res[2] = {0, 0};
  for (uint32_t i = 0; i < n; i++) {
    const size_t e = ifd + 2 + 12 * (size_t)i;
    const Entry en{f.u16(e), f.u16(e + 2), f.u32(e + 4), e + 8};
    const size_t whole = f.n;  // no array holds more values than the file has bytes
    switch (en.tag) {
      case 256: case 257: case 259: case 262: case 266: case 277: case 278: case 284: case 292: case 296: case 317:
        if (!values(f, en, 1, &v, &pg->error)) return false;
        break;
      default:
        break;
    }
    switch (en.tag) {
      case 256: pg->width = (int32_t)std::min<uint32_t>(v[0], 0x7FFFFFFF), have_w = true; break;
      case 257: pg->height = (int32_t)std::min<uint32_t>(v[0], 0x7FFFFFFF), have_h = true; break;
      case 258: if (!values(f, en, 8, &bits, &pg->error)) return false; break;
      case 259: pg->compression = (int32_t)v[0]; break;
      case 262: pg->photometric = (int32_t)v[0], have_phot = true; break;
      case 266: pg->fill_order = (int32_t)v[0]; break;
      case 273: if (!values(f, en, whole, &offs, &pg->error)) return false; break;
      case 277: pg->spp = (int32_t)v[0]; break;
      case 278: pg->rows_per_strip = v[0], have_rps = true; break;
      case 279: if (!values(f, en, whole, &cnts, &pg->error)) return false; break;
      case 282: case 283:
        if (en.type == 5 && en.count == 1 && f.holds(f.u32(en.at), 8)) {
          const size_t at = f.u32(en.at);
          const uint32_t num = f.u32(at), den = f.u32(at + 4);
          res[en.tag - 282] = den ? (double)num / den : 0;
        }
        break;
      case 284: planar = v[0]; break;
      case 292: pg->t4_options = v[0]; break;
      case 296: unit = v[0]; break;
      case 317: pg->predictor = (int32_t)v[0]; break;
      case 320: if (!values(f, en, 768, &cmap, &pg->error)) return false; break;
      case 322: case 323: case 324: case 325:
        return refuse(pg, "tiles are not supported (%s, tag %u)",
                      en.tag == 322 ? "TileWidth" : en.tag == 323 ? "TileLength" : en.tag == 324 ? "TileOffsets"
                                                                                               : "TileByteCounts",
                      en.tag);
      case 338: if (!values(f, en, 8, &extra, &pg->error)) return false; break;
      default: break;
    }
  }
  if (!have_w || !have_h) return refuse(pg, "no %s", have_w ? "ImageLength" : "ImageWidth");
  const int64_t w = pg->width, h = pg->height;
  if (w <= 0 || h <= 0 || w > kMaxSide || h > kMaxSide || 3 * w * h > kMaxRaster)
    return refuse(pg, "ImageWidth x ImageLength %lldx%lld is out of range", (long long)w, (long long)h);
  if (planar != 1 && pg->spp > 1) return refuse(pg, "PlanarConfiguration %u is not supported", planar);
  for (uint32_t b : bits)
    if (b != bits[0]) return refuse(pg, "BitsPerSample %u/%u is not supported", bits[0], b);
  if (bits[0] != 1 && bits[0] != 8) return refuse(pg, "BitsPerSample %u is not supported", bits[0]);
  if ((int)bits.size() != pg->spp && !(bits.size() == 1 && pg->spp == 1))
    return refuse(pg, "BitsPerSample has %zu values for SamplesPerPixel %d", bits.size(), pg->spp);
  pg->bits = (int32_t)bits[0];
  pg->extra = (int32_t)extra.size();
  const int phot = have_phot ? pg->photometric : (pg->bits == 1 ? 0 : 1);
  pg->photometric = phot;
  if (phot < 0 || phot > 3) return refuse(pg, "PhotometricInterpretation %d is not supported", phot);
  if (pg->extra > 1) return refuse(pg, "ExtraSamples: %d extra samples are not supported", pg->extra);
  if (pg->bits == 1) {
    if (pg->spp != 1) return refuse(pg, "SamplesPerPixel %d with BitsPerSample 1", pg->spp);
    if (phot > 1) return refuse(pg, "PhotometricInterpretation %d with BitsPerSample 1", phot);
    pg->format = phot == 0 ? UPHIP_FMT_MONOWHITE : UPHIP_FMT_MONOBLACK;
  } else if (phot <= 1) {
    if (pg->spp == 1 && pg->extra == 0) pg->format = UPHIP_FMT_GRAY8;
    else if (pg->spp == 2 && pg->extra == 1) pg->format = UPHIP_FMT_Y400A;
    else return refuse(pg, "SamplesPerPixel %d (ExtraSamples %d) for a gray image", pg->spp, pg->extra);
  } else if (phot == 2) {
    if (pg->spp == 4) return refuse(pg, "SamplesPerPixel 4 (RGBA, ExtraSamples %d) is not supported", pg->extra);
    if (pg->spp != 3 || pg->extra) return refuse(pg, "SamplesPerPixel %d for an RGB image", pg->spp);
    pg->format = UPHIP_FMT_RGB24;
  } else {
    if (pg->spp != 1) return refuse(pg, "SamplesPerPixel %d for a palette image", pg->spp);
    if (cmap.size() != 768) return refuse(pg, "ColorMap has %zu entries, 768 expected", cmap.size());
    pg->format = UPHIP_FMT_RGB24;
    pg->pal.resize(768);
    for (int i = 0; i < 256; i++)
      for (int c = 0; c < 3; c++) pg->pal[(size_t)(3 * i + c)] = (uint8_t)(cmap[(size_t)(256 * c + i)] >> 8);
  }
  const int comp = pg->compression;
  const bool fax = comp == 3 || comp == 4;
  if (comp != 1 && comp != kCompPackBits && comp != kCompLzw && comp != 8 && comp != 32946 && !fax)
    return refuse(pg, "Compression %d is not supported", comp);
  if (fax && pg->bits != 1) return refuse(pg, "Compression %d with BitsPerSample %d", comp, pg->bits);
  const bool predicts = comp == kCompLzw || comp == 8 || comp == 32946;
  if (!predicts) pg->predictor = 1;
  if (pg->predictor != 1 && pg->predictor != 2) return refuse(pg, "Predictor %d is not supported", pg->predictor);
  if (pg->predictor == 2 && pg->bits == 1) return refuse(pg, "Predictor 2 with BitsPerSample 1");
  if (pg->fill_order != 1 && pg->fill_order != 2) return refuse(pg, "FillOrder %d", pg->fill_order);
  if (pg->fill_order == 2 && pg->bits != 1) return refuse(pg, "FillOrder 2 with BitsPerSample %d", pg->bits);
  pg->src_row_bytes = pg->bits == 1 ? (w + 7) / 8 : w * pg->spp;
  if (unit == 2 || unit == 3)
    for (int i = 0; i < 2; i++) pg->dpi[i] = (float)(unit == 3 ? res[i] * 2.54 : res[i]);
  // strips
  if (offs.empty()) return refuse(pg, "no StripOffsets");
  if (!have_rps || pg->rows_per_strip == 0 || pg->rows_per_strip > (uint32_t)h) pg->rows_per_strip = (uint32_t)h;
  const uint64_t nstrips = ((uint64_t)h + pg->rows_per_strip - 1) / pg->rows_per_strip;
  if (offs.size() != nstrips)
    return refuse(pg, "StripOffsets has %zu entries for %llu strips (RowsPerStrip %u)", offs.size(),
                  (unsigned long long)nstrips, pg->rows_per_strip);
  if (cnts.empty()) {
    if (nstrips != 1 || comp != 1) return refuse(pg, "no StripByteCounts");
    const uint64_t need = (uint64_t)pg->src_row_bytes * (uint64_t)h;
    if (!f.holds(offs[0], need)) return refuse(pg, "StripOffsets %u: the strip passes the end of the file", offs[0]);
    cnts.assign(1, (uint32_t)need);
  }
  if (cnts.size() != nstrips)
    return refuse(pg, "StripByteCounts has %zu entries for %llu strips", cnts.size(), (unsigned long long)nstrips);
  pg->off = std::move(offs);
  pg->cnt = std::move(cnts);
  for (size_t s = 0; s < pg->off.size(); s++) {
    if (!f.holds(pg->off[s], pg->cnt[s]))
      return refuse(pg, "StripOffsets %u + StripByteCounts %u pass the end of the file", pg->off[s], pg->cnt[s]);
    const uint64_t need = (uint64_t)pg->src_row_bytes * pg->strip_rows(s);
    if (need > 0x7FFFFFFFull) return refuse(pg, "RowsPerStrip %u: a strip of %llu bytes", pg->rows_per_strip,
                                            (unsigned long long)need);
    if (comp == 1 ? pg->cnt[s] < need : (!fax && need > kMaxExpansion * ((uint64_t)pg->cnt[s] + 1)))
      return refuse(pg, "StripByteCounts %u is too small for a strip of %llu bytes", pg->cnt[s],
                    (unsigned long long)need);
  }
  pg->ops.src_bytes = (int32_t)pg->src_row_bytes;
  pg->ops.spp = pg->spp;
  pg->ops.predictor = pg->predictor;
  // FillOrder 2 as libtiff reads it: the strip's bytes are reversed before they
  // are decoded, whatever the coder; for uncompressed rows that is the rows
  pg->ops.bitrev = pg->fill_order == 2 && comp == 1;
  pg->ops.invert = pg->bits == 8 && phot == 0;
  pg->ops.palette = phot == 3;
  return true;
}

const char* status_text(int32_t st) {
  return (st & kOldLzw)   ? "old-style (LSB-first) LZW is not supported"
         : (st & kRange)  ? "a strip too large for its decoder"
         : (st & kCode)   ? "a code that cannot occur"
         : (st & kOutput) ? "a run passes the strip's rows"
         : (st & kShort)  ? "the data ends before the strip's rows are full"
                          : "the strip's bytes end too early";
}

bool inflate_strip(const uint8_t* in, uint32_t n, uint8_t* out, uint32_t need) {
  z_stream z{};
  if (inflateInit(&z) != Z_OK) return false;
  z.next_in = const_cast<uint8_t*>(in);
  z.avail_in = n;
  z.next_out = out;
  z.avail_out = need;
  const int r = inflate(&z, Z_FINISH);
  inflateEnd(&z);
  // the strip's rows in full; a stream that holds more is cut there (Z_BUF_ERROR)
  return z.avail_out == 0 && (r == Z_STREAM_END || r == Z_BUF_ERROR || r == Z_OK);
}

}  // namespace

const char* strip_error(int32_t st) { return status_text(st); }

bool open(std::vector<uint8_t>&& bytes, const char* name, Document* doc) {
  doc->bytes = std::move(bytes);
  doc->name = name ? name : "";
  doc->pages.clear();
  const char* nm = doc->name.c_str();
  const File probe{doc->bytes.data(), doc->bytes.size(), false};
  if (probe.n < 8) return fail("tiff: %s: not a TIFF file", nm);
  const bool le = probe.p[0] == 'I' && probe.p[1] == 'I', be = probe.p[0] == 'M' && probe.p[1] == 'M';
  if (!le && !be) return fail("tiff: %s: not a TIFF file", nm);
  const File f{probe.p, probe.n, be};
  const uint32_t magic = f.u16(2);
  if (magic == 43) return fail("tiff: %s: BigTIFF (magic 43) is not supported", nm);
  if (magic != 42) return fail("tiff: %s: not a TIFF file (magic %u)", nm, magic);
  std::vector<uint32_t> seen;
  uint32_t ifd = f.u32(4);
  while (ifd != 0 && (int)doc->pages.size() < kMaxIfds) {
    if (std::find(seen.begin(), seen.end(), ifd) != seen.end()) break;  // a chain that loops ends here
    if (!f.holds(ifd, 2) || !f.holds(ifd, 2 + 12 * (uint64_t)f.u16(ifd) + 4)) {
      if (doc->pages.empty()) return fail("tiff: %s: the IFD at offset %u passes the end of the file", nm, ifd);
      break;
    }
    seen.push_back(ifd);
    doc->pages.emplace_back();
    parse_page(f, ifd, &doc->pages.back());
    ifd = f.u32(ifd + 2 + 12 * (size_t)f.u16(ifd));
  }
  if (doc->pages.empty()) return fail("tiff: %s: no image (IFD offset 0)", nm);
  return true;
}

const Page* page(const Document& doc, int64_t index) {
  if (index < 0 || index >= (int64_t)doc.pages.size())
    return fail("tiff: %s: page %lld out of range (%zu pages)", doc.name.c_str(), (long long)index,
                doc.pages.size()),
           nullptr;
  const Page& p = doc.pages[(size_t)index];
  if (!p.error.empty())
    return fail("tiff: %s: page %lld: %s", doc.name.c_str(), (long long)index, p.error.c_str()), nullptr;
  return &p;
}

bool device_decodable(const Page& p) {
  if (p.compression != kCompPackBits && p.compression != kCompLzw) return false;
  return (uint64_t)p.src_row_bytes * p.rows_per_strip <= kSmallStrip;
}

bool device_route(const Page& p) { return device_decodable(p) && p.off.size() >= 8; }

bool decode_host(const Document& doc, const Page& p, uint8_t* dst, int64_t linesize) {
  const char* nm = doc.name.c_str();
  const int comp = p.compression;
  const size_t rb = (size_t)p.src_row_bytes;
  const uint64_t strip_max = (uint64_t)rb * p.rows_per_strip;
  // the decoded strip: left untouched beyond what a strip's data fills, so a
  // crafted header commits no memory
  std::unique_ptr<uint8_t[]> scratch;
  if (comp != 1 && comp != 3 && comp != 4) {
    scratch.reset(new (std::nothrow) uint8_t[strip_max]);
    if (!scratch) return fail("tiff: %s: out of memory (a strip of %llu bytes)", nm, (unsigned long long)strip_max);
  }
  std::vector<uint8_t> row(rb), rev;
  ccitt::Image fax;
  for (size_t s = 0; s < p.off.size(); s++) {
    const uint8_t* in = doc.bytes.data() + p.off[s];
    const uint32_t n = p.cnt[s], rows = p.strip_rows(s);
    const uint32_t need = (uint32_t)(rb * rows);
    const uint8_t* dec = scratch.get();
    if (p.fill_order == 2 && comp != 1) {
      rev.resize(n);
      for (uint32_t i = 0; i < n; i++) rev[i] = bitrev8(in[i]);
      in = rev.data();
    }
    if (comp == 1) {
      dec = in;
    } else if (comp == kCompPackBits || comp == kCompLzw) {
      int32_t st;
      if (comp == kCompPackBits) {
        st = packbits(in, n, scratch.get(), need);
      } else if (need <= kSmallStrip) {
        uint16_t pos[kLzwCodes], len[kLzwCodes];
        st = lzw<uint16_t>(in, n, scratch.get(), need, pos, len);
      } else {
        uint32_t pos[kLzwCodes], len[kLzwCodes];
        st = lzw<uint32_t>(in, n, scratch.get(), need, pos, len);
      }
      if (st != kOk) return fail("tiff: %s: strip %zu: %s", nm, s, status_text(st));
    } else if (comp == 8 || comp == 32946) {
      if (!inflate_strip(in, n, scratch.get(), need)) return fail("tiff: %s: strip %zu: corrupt Deflate data", nm, s);
    } else {
      ccitt::Params prm;
      prm.k = comp == 4 ? -1 : (p.t4_options & 1) ? 1 : 0;
      prm.columns = p.width;
      prm.eol = comp == 3;
      if (!ccitt::decode(in, n, prm, (int32_t)rows, &fax, nm)) return false;
      dec = fax.bits.data();  // stride (width + 7) / 8 = the stored row bytes
    }
    for (uint32_t y = 0; y < rows; y++) {
      memcpy(row.data(), dec + (size_t)y * rb, rb);
      finish_row(row.data(), dst + ((int64_t)s * p.rows_per_strip + y) * linesize, p.ops, p.pal.data());
    }
  }
  return true;
}

bool read_file(const char* path, std::vector<uint8_t>* out) {
  FILE* f = fopen(path, "rb");
  if (!f) return fail("tiff: cannot open %s: %s", path, strerror(errno));
  bool ok = fseek(f, 0, SEEK_END) == 0;
  const long n = ok ? ftell(f) : -1;
  ok = ok && n >= 0 && fseek(f, 0, SEEK_SET) == 0;
  if (ok) {
    out->resize((size_t)n);
    ok = n == 0 || fread(out->data(), 1, (size_t)n, f) == (size_t)n;
  }
  fclose(f);
  return ok || fail("tiff: cannot read %s", path);
}

bool open_file(const char* path, Document* doc) {
  std::vector<uint8_t> bytes;
  return read_file(path, &bytes) && open(std::move(bytes), path, doc);
}

// The checks of every read entry: geometry against `expect`, the row pitch.
bool read_page(const Document& doc, int64_t index, void* dst, int64_t linesize, const UphipPnmInfo* expect) {
  const Page* p = page(doc, index);
  if (!p) return false;
  if (expect && (expect->width != p->width || expect->height != p->height || expect->format != p->format))
    return fail("tiff: %s is %dx%d format %d, expected %dx%d format %d", doc.name.c_str(), p->width, p->height,
                p->format, expect->width, expect->height, expect->format);
  if (linesize < row_bytes(p->width, p->format)) return fail("tiff_read: linesize too small");
  return decode_host(doc, *p, (uint8_t*)dst, linesize);
}

}  // namespace tiff
}  // namespace uph

using namespace uph;

extern "C" {

UphipTiffDocument* uphip_tiff_open(const char* path) {
  if (!path) return fail("tiff_open: null path"), nullptr;
  try {
    std::unique_ptr<UphipTiffDocument> d(new UphipTiffDocument());
    if (!tiff::open_file(path, &d->doc)) return nullptr;
    return d.release();
  } catch (const std::bad_alloc&) {
    return fail("tiff: %s: out of memory", path), nullptr;
  }
}

void uphip_tiff_close(UphipTiffDocument* doc) { delete doc; }

int uphip_tiff_page_count(UphipTiffDocument* doc) {
  if (!doc) return fail("tiff_page_count: null document"), -1;
  return (int)doc->doc.pages.size();
}

int uphip_tiff_page_probe(UphipTiffDocument* doc, int page, UphipPnmInfo* info, float* dpi_out) {
  if (!doc || !info) return fail("tiff_page_probe: null argument"), -1;
  const tiff::Page* p = tiff::page(doc->doc, page);
  if (!p) return -1;
  info->width = p->width;
  info->height = p->height;
  info->format = p->format;
  if (dpi_out) dpi_out[0] = p->dpi[0], dpi_out[1] = p->dpi[1];
  return 0;
}

int uphip_tiff_read_page(UphipTiffDocument* doc, int page, void* dst, int64_t linesize,
                         const UphipPnmInfo* expect) {
  if (!doc || !dst) return fail("tiff_read_page: null argument"), -1;
  try {
    return tiff::read_page(doc->doc, page, dst, linesize, expect) ? 0 : -1;
  } catch (const std::bad_alloc&) {
    return fail("tiff: %s: out of memory", doc->doc.name.c_str()), -1;
  }
}

int uphip_tiff_page_on_device(UphipTiffDocument* doc, int page) {
  if (!doc) return fail("tiff_page_on_device: null document"), -1;
  const tiff::Page* p = tiff::page(doc->doc, page);
  return p ? (tiff::device_route(*p) ? 1 : 0) : -1;
}

int uphip_tiff_probe(const char* path, UphipPnmInfo* info) {
  if (!path || !info) return fail("tiff_probe: null argument"), -1;
  UphipTiffDocument* d = uphip_tiff_open(path);
  if (!d) return -1;
  const int r = uphip_tiff_page_probe(d, 0, info, nullptr);
  uphip_tiff_close(d);
  return r;
}

int uphip_tiff_read(const char* path, void* dst, int64_t linesize, const UphipPnmInfo* expect) {
  if (!path || !dst) return fail("tiff_read: null argument"), -1;
  UphipTiffDocument* d = uphip_tiff_open(path);
  if (!d) return -1;
  const int r = uphip_tiff_read_page(d, 0, dst, linesize, expect);
  uphip_tiff_close(d);
  return r;
}

}  // extern "C"
