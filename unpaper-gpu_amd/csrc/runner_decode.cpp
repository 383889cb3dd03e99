// runner_decode.cpp — the load side of a host-fed run: a source's page into
// the slot's staging (the decode queue's work, lib/decode_queue.c), the host
// half of JPEG / JPEG 2000 / PDF pages, and what the device thread queues for
// a loaded chunk: the staging upload, the pages' device decode and, for a
// JPEG 2000 sink, the chunk's device encode.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "runner_internal.h"

namespace uph {
namespace {

int mem_load(const UphipSource* s, int64_t idx, void* dst, int64_t linesize,
             const UphipPnmInfo& geo) {
  if (idx < 0 || idx >= s->npages) return fail("source_memory: page %lld out of range", (long long)idx), -1;
  const int64_t rb = row_bytes(geo.width, geo.format);
  const uint8_t* src = s->base + idx * s->page_stride;
  uint8_t* d = (uint8_t*)dst;
  if (linesize == s->linesize && linesize == rb) {
    memcpy(d, src, (size_t)(rb * geo.height));
  } else {
    for (int32_t y = 0; y < geo.height; y++)
      memcpy(d + (int64_t)y * linesize, src + (int64_t)y * s->linesize, (size_t)rb);
  }
  return 0;
}

// A page the runner takes, or the error that names it: of the runner's
// geometry, or, with a fixed sheet (sheet_size fully set, no pre_rotate), of
// its format and at most its size.  *size: the page's.
bool same_geometry(const UphipRunner* r, const UphipPnmInfo& g, const char* kind, const char* name,
                   PageSize* size) {
  const bool fmt = g.format == r->geo.page_format;
  *size = PageSize{g.width, g.height};
  if (fmt && g.width == r->geo.page_width && g.height == r->geo.page_height) return true;
  if (r->fixed_sheet) {
    if (fmt && g.width > 0 && g.height > 0 && g.width <= r->geo.page_width && g.height <= r->geo.page_height)
      return true;
    return fail("%s: %s is %dx%d format %d, the runner takes format %d up to the maximum %dx%d", kind, name,
                g.width, g.height, g.format, r->geo.page_format, r->geo.page_width, r->geo.page_height);
  }
  return fail("%s: %s is %dx%d format %d, expected %dx%d format %d (a fully set sheet_size, without "
              "pre_rotate, admits pages of other sizes up to the geometry's)",
              kind, name, g.width, g.height, g.format, r->geo.page_width, r->geo.page_height,
              r->geo.page_format);
}

int pnm_load(const UphipRunner* r, const UphipSource* s, int64_t idx, void* dst, int64_t linesize,
             PageSize* size) {
  if (idx < 0 || idx >= (int64_t)s->paths.size())
    return fail("source_pnm: page %lld out of range", (long long)idx), -1;
  const char* path = s->paths[(size_t)idx].c_str();
  UphipPnmInfo g{0, 0, 0};
  if (uphip_image_probe(path, &g) != 0 || !same_geometry(r, g, "source_pnm", path, size)) return -1;
  return uphip_image_read(path, dst, linesize, &g);
}

bool is_jpeg_file(const std::string& path) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  uint8_t sig[3];
  const bool yes = fread(sig, 1, 3, f) == 3 && sig[0] == 0xFF && sig[1] == 0xD8 && sig[2] == 0xFF;
  fclose(f);
  return yes;
}

// The host half of a JPEG page into the slot's pinned buffer `jp`.
bool jpeg_load_mem(UphipRunner* r, int device, const uint8_t* data, size_t size, const char* name,
                   JpegPage* jp, PageSize* ps) {
  thread_local JdecStreamHost S;
  // the frame header first: a file of the wrong geometry (or a crafted one
  // claiming a huge frame) is refused before anything is sized from it
  UphipPnmInfo info{0, 0, 0};
  if (!jpeg_probe_mem(data, size, name, &info) || !same_geometry(r, info, "jpeg", name, ps)) return false;
  // a one-scan sequential file goes to the device as its unstuffed entropy
  // data (Huffman decoding there too); progressive / multi-scan files are
  // entropy-decoded here
  const int dev = jpeg_stream_prepare(data, size, name, &S);
  if (dev < 0) return false;
  JpegDecoded d;
  if (!dev && !jpeg_entropy_decode(data, size, name, &d)) return false;
  // pinned memory for this device (the pool thread may have another current)
  if (uphip_set_device(device) != 0) return false;
  const size_t need = (size_t)(dev ? S.hd.total_bytes : d.h.total_bytes);
  if (!jp->host.reserve(need, need / 4)) return false;
  if (dev)
    jpeg_stream_pack(S, jp->host.as());
  else
    jpeg_pack(d, jp->host.as());
  jp->h = dev ? S.hd.h : d.h;
  jp->dev = dev == 1;
  jp->j2k = false;
  jp->bytes = need;
  jp->on = true;
  return true;
}

bool is_j2k_file(const std::string& path) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  uint8_t sig[12];
  const size_t n = fread(sig, 1, 12, f);
  fclose(f);
  return j2k::is_j2k(sig, n);
}

// The host half of a JPEG 2000 page (headers, packet headers) into the
// slot's pinned buffer `jp`: its code-block jobs, then their codewords.
bool j2k_load_mem(UphipRunner* r, int device, const uint8_t* data, size_t size, const char* name,
                  JpegPage* jp, PageSize* ps) {
  thread_local j2k::T1Batch tb;
  UphipPnmInfo info{0, 0, 0};
  if (!j2k::probe(data, size, name, &info) || !same_geometry(r, info, "jp2", name, ps)) return false;
  if (!j2k::decode_host(data, size, name, &jp->img, nullptr, &tb)) return false;
  if (uphip_set_device(device) != 0) return false;
  jp->njobs = (int32_t)tb.jobs.size();
  jp->jobs_bytes = (sizeof(j2k::T1Job) * tb.jobs.size() + 255) & ~(size_t)255;
  jp->maxw = tb.maxw;
  jp->maxh = tb.maxh;
  const size_t need = jp->jobs_bytes + tb.data.size();
  if (!jp->host.reserve(need, need / 4)) return false;
  memcpy(jp->host.as(), tb.jobs.data(), sizeof(j2k::T1Job) * tb.jobs.size());
  memcpy(jp->host.as() + jp->jobs_bytes, tb.data.data(), tb.data.size());
  jp->h = JpegHeader{};
  jp->h.scratch_bytes = (int64_t)j2k::decode_tmp_bytes(jp->img);  // the line buffer
  jp->j2k = true;
  jp->dev = false;
  jp->bytes = need;
  jp->on = true;
  return true;
}

// A JPEG or JPEG 2000 file through its loader above.
bool file_load(decltype(jpeg_load_mem)* load, UphipRunner* r, int device, const std::string& path, JpegPage* jp,
               PageSize* ps) {
  // per pool thread, kept across pages: fresh multi-MB buffers per page would
  // page-fault (and contend on the address space) on every load
  thread_local std::vector<uint8_t> file;
  return jpeg_read_file(path.c_str(), &file) && load(r, device, file.data(), file.size(), path.c_str(), jp, ps);
}

// Page `idx` of a PDF source (the decode queue of the PDF pipeline,
// pdf_pipeline_cpu_batch.c:381-496): its image's JPEG / JPEG 2000 bytes to
// the device decode like a file's, Flate / raw pixels decoded here.
bool pdf_load(UphipRunner* r, int device, const UphipSource* s, int64_t idx, uint8_t* dst, JpegPage* jp,
              PageSize* ps) {
  if (idx < 0 || idx >= s->pdf->page_count())
    return fail("source_pdf: page %lld out of range (%d pages)", (long long)idx, s->pdf->page_count());
  thread_local pdf::PageImage im;
  UphipPnmInfo g{0, 0, 0};
  if (!pdf::page_geometry(*s->pdf, (int)idx, s->pdf_dpi, &im, &g)) return false;
  char name[64];
  snprintf(name, sizeof(name), "pdf page %lld", (long long)idx);
  if (im.format == pdf::kJpeg) return jpeg_load_mem(r, device, im.data.data(), im.data.size(), name, jp, ps);
  if (im.format == pdf::kJp2) return j2k_load_mem(r, device, im.data.data(), im.data.size(), name, jp, ps);
  return same_geometry(r, g, "pdf", name, ps) && pdf::decode_pixels(im, dst, r->in_pitch, name);
}

size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

bool is_tiff_file(const std::string& path) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  uint8_t sig[4];
  const bool yes = fread(sig, 1, 4, f) == 4 && ((sig[0] == 'I' && sig[1] == 'I' && sig[2] == 42 && sig[3] == 0) ||
                                                (sig[0] == 'M' && sig[1] == 'M' && sig[2] == 0 && sig[3] == 42));
  fclose(f);
  return yes;
}

// Page `idx` of a TIFF document: its pixels into the staging, or, when the
// source asks for the device route and the page qualifies, its strips into
// the slot's pinned blob `tp` (tiff_dec.h).
bool tiff_load(UphipRunner* r, int device, const tiff::Document& doc, int64_t idx, bool host_only, uint8_t* dst,
               TiffPage* tp, PageSize* ps) {
  const tiff::Page* p = tiff::page(doc, idx);
  if (!p) return false;
  // the geometry first: nothing is sized from a page of another shape
  char name[24];
  snprintf(name, sizeof(name), " page %lld", (long long)idx);
  if (!same_geometry(r, UphipPnmInfo{p->width, p->height, p->format}, "tiff", (doc.name + name).c_str(), ps))
    return false;
  if (host_only || !tiff::device_route(*p)) return tiff::decode_host(doc, *p, dst, r->in_pitch);
  if (uphip_set_device(device) != 0) return false;
  const size_t need = tiff::blob_bytes(*p);
  if (!tp->host.reserve(need, need / 4)) return false;
  tiff::blob_fill(doc, *p, tp->host.as());
  tp->jobs.resize(p->off.size());
  tiff::page_jobs(*p, 0, 0, 0, tp->jobs.data());
  tp->rows = tiff::rows_page(*p, 0, 0, 0, nullptr, 0);
  tp->raster = (uint64_t)p->src_row_bytes * (uint64_t)p->height;
  tp->lzw = p->compression == tiff::kCompLzw;
  tp->bytes = need;
  tp->on = true;
  return true;
}

constexpr int kJ2kSubBatch = 16;  // pages coded per k_j2k_t1enc launch (bounds the arena)

}  // namespace

bool load_page(UphipRunner* r, int device, const UphipSource* s, int64_t job, int32_t j,
               uint8_t* dst, JpegPage* jp, TiffPage* tp, PageSize* ps) {
  const UphipPnmInfo geo{r->geo.page_width, r->geo.page_height, r->geo.page_format};
  const int64_t idx = job * r->opts.input_count + j;
  *ps = PageSize{geo.width, geo.height};  // callback and memory sources carry no size of their own
  if (s->load) return s->load(s->user, job, j, dst, r->in_pitch) == 0;
  if (s->base) return mem_load(s, idx, dst, r->in_pitch, geo) == 0;
  if (s->pdf) return pdf_load(r, device, s, idx, dst, jp, ps);
  if (s->tiff) return tiff_load(r, device, *s->tiff, idx, !(s->tiff_flags & UPHIP_TIFF_DEVICE_DECODE), dst, tp, ps);
  if (idx >= 0 && idx < (int64_t)s->paths.size()) {
    const std::string& path = s->paths[(size_t)idx];
    if (is_jpeg_file(path)) return file_load(jpeg_load_mem, r, device, path, jp, ps);
    if (is_j2k_file(path)) return file_load(j2k_load_mem, r, device, path, jp, ps);
    if (is_tiff_file(path)) {
      tiff::Document doc;
      return tiff::open_file(path.c_str(), &doc) && tiff_load(r, device, doc, 0, true, dst, tp, ps);
    }
  }
  return pnm_load(r, s, idx, dst, r->in_pitch, ps) == 0;
}

bool source_page_info(const UphipSource* s, int64_t idx, UphipPnmInfo* g, std::string* name) {
  char buf[32];
  snprintf(buf, sizeof(buf), " page %lld", (long long)idx);
  if (s->pdf) {
    thread_local pdf::PageImage im;
    *name = "pdf" + std::string(buf);
    return pdf::page_geometry(*s->pdf, (int)idx, s->pdf_dpi, &im, g);
  }
  if (s->tiff) {
    const tiff::Page* p = tiff::page(*s->tiff, idx);
    *name = s->tiff->name + buf;
    if (p) *g = UphipPnmInfo{p->width, p->height, p->format};
    return p != nullptr;
  }
  if (idx < 0 || idx >= (int64_t)s->paths.size()) return fail("source: page %lld out of range", (long long)idx);
  *name = s->paths[(size_t)idx];
  return uphip_image_probe(name->c_str(), g) == 0;
}

// Queue the H2D copy of the slot's staged pages, skipping the JPEG pages (their
// decode writes the batch's input slots itself, after this copy): runs of
// other pages go as one copy each (the staging is laid out like the slots).
bool upload_staging(UphipRunner* r, Slot* sl, int npages) {
  bool any = false;
  auto on = [sl](int p) { return sl->jpg[(size_t)p].on || sl->tif[(size_t)p].on; };
  for (int p = 0; p < npages; p++) any |= on(p);
  if (!any)
    return uphip_batch_upload_async(sl->b, sl->count, sl->hin.as(), r->in_pitch, r->in_page_stride) == 0;
  hipStream_t st = (hipStream_t)uphip_batch_stream(sl->b);
  for (int p = 0; p < npages;) {
    if (on(p)) {
      p++;
      continue;
    }
    int e = p;
    while (e < npages && !on(e)) e++;
    int64_t pitch = 0;
    uint8_t* dst = (uint8_t*)uphip_batch_input_ptr(sl->b, p, &pitch);
    if (!dst || pitch != r->in_pitch ||
        !UPH_HIP(hipMemcpyAsync(dst, sl->hin.as() + (int64_t)p * r->in_page_stride,
                                (size_t)((int64_t)(e - p) * r->in_page_stride),
                                hipMemcpyHostToDevice, st)))
      return false;
    p = e;
  }
  return true;
}

// Queue the chunk's JPEG and JPEG 2000 pages on the slot's stream: upload each
// packed page (JPEG 2000: its coefficient planes), then decode it into its
// input slot (after the staging upload, before the run).
bool jpeg_submit(Slot* sl, int npages) {
  size_t total = 0, scr = 0, pk = 0, hs = 0;
  int ndev = 0;
  int64_t max_nsub = 0, max_nmac = 0;
  sl->jdev = false;
  for (int p = 0; p < npages; p++) {
    const JpegPage& jp = sl->jpg[(size_t)p];
    if (!jp.on) continue;
    total += up256(jp.bytes);  // page starts aligned (JPEG 2000 planes are int32)
    scr = std::max(scr, (size_t)jp.h.scratch_bytes);
    if (jp.dev) {
      const JdecHeader& hd = *jp.host.as<const JdecHeader>();
      ndev++;
      pk += up256((size_t)jp.h.total_bytes);
      hs += up256(jdec_scratch_bytes(hd));
      max_nsub = std::max<int64_t>(max_nsub, hd.nsub);
      max_nmac = std::max<int64_t>(max_nmac, hd.nmac);
    }
  }
  if (!total) return true;
  // the slot's stream is idle here (the slot was free): old buffers can go
  auto grow = [](Buffer& b, size_t need) { return b.reserve(need, need / 4); };
  if (!grow(sl->djpg, total) || (scr && !grow(sl->dscr, scr))) return false;
  uint8_t* const djpg = sl->djpg.as();
  uint8_t* const dscr = sl->dscr.as();
  hipStream_t st = (hipStream_t)uphip_batch_stream(sl->b);
  if (ndev) {
    sl->jdev = true;
    if (!grow(sl->djpk, pk) || !grow(sl->djsc, hs) || !grow(sl->djst, 4 * (size_t)npages) ||
        !sl->djob.reserve(sizeof(JdecJob) * (size_t)npages) || !sl->hjob.reserve(sizeof(JdecJob) * (size_t)npages) ||
        !UPH_HIP(hipMemsetAsync(sl->djst.as(), 0, 4 * (size_t)npages, st)))
      return false;
  }
  JdecJob* const hjob = sl->hjob.as<JdecJob>();
  // upload every page; the device-decoded ones as one batch of jobs
  size_t off = 0, poff = 0, soff = 0;
  int nj = 0;
  for (int p = 0; p < npages; p++) {
    JpegPage& jp = sl->jpg[(size_t)p];
    if (!jp.on) continue;
    if (!UPH_HIP(hipMemcpyAsync(djpg + off, jp.host.as(), jp.bytes, hipMemcpyHostToDevice, st)))
      return false;
    if (jp.dev) {
      const JdecHeader& hd = *jp.host.as<const JdecHeader>();
      hjob[nj++] = JdecJob{djpg + off, sl->djpk.as() + poff, sl->djsc.as() + soff, sl->djst.as<int32_t>() + p};
      poff += up256((size_t)jp.h.total_bytes);
      soff += up256(jdec_scratch_bytes(hd));
    }
    off += up256(jp.bytes);
  }
  if (nj) {
    if (!UPH_HIP(hipMemcpyAsync(sl->djob.as(), hjob, sizeof(JdecJob) * (size_t)nj, hipMemcpyHostToDevice, st)) ||
        !jdec_launch_batch(sl->djob.as<JdecJob>(), nj, max_nsub, max_nmac, st))
      return false;
  }
  // JPEG 2000 pages: every code-block of the chunk in one launch (offsets
  // made chunk-wide), into one coefficient buffer
  {
    int64_t nj = 0, coefs = 0;
    int maxw = 0, maxh = 0;
    for (int p = 0; p < npages; p++) {
      const JpegPage& jp = sl->jpg[(size_t)p];
      if (!jp.on || !jp.j2k) continue;
      nj += jp.njobs;
      coefs += jp.img.coef_elems;
      maxw = std::max(maxw, jp.maxw);
      maxh = std::max(maxh, jp.maxh);
    }
    if (coefs > 0) {
      const int nslots = (int)std::min<int64_t>((nj + 63) / 64, 1024);
      if (!grow(sl->dj2c, (size_t)coefs * 4) ||
          !grow(sl->dj2t, (size_t)std::max(nslots, 1) * j2k::t1_slot_bytes(maxw, maxh)) ||
          !grow(sl->dj2j, sizeof(j2k::T1Job) * (size_t)std::max<int64_t>(nj, 1)) ||
          !sl->hj2j.reserve(sizeof(j2k::T1Job) * (size_t)nj + 256))
        return false;
      j2k::T1Job* const hj2j = sl->hj2j.as<j2k::T1Job>();
      size_t o = 0;
      int64_t q = 0, cb = 0;
      for (int p = 0; p < npages; p++) {
        const JpegPage& jp = sl->jpg[(size_t)p];
        if (!jp.on) continue;
        if (jp.j2k) {
          const j2k::T1Job* pj = jp.host.as<const j2k::T1Job>();
          for (int i = 0; i < jp.njobs; i++) {
            j2k::T1Job t = pj[i];
            t.data += (uint32_t)(o + jp.jobs_bytes);
            t.out += cb;
            hj2j[q++] = t;
          }
          cb += jp.img.coef_elems;
        }
        o += up256(jp.bytes);
      }
      if (o > 0xFFFFFFF0u) return fail("jp2: chunk too large for 32-bit codeword offsets");
      if (!UPH_HIP(hipMemcpyAsync(sl->dj2j.as(), hj2j, sizeof(j2k::T1Job) * (size_t)nj,
                                  hipMemcpyHostToDevice, st)) ||
          !UPH_HIP(hipMemsetAsync(sl->dj2c.as(), 0, (size_t)coefs * 4, st)) ||
          !j2k::t1_launch(sl->dj2j.as<j2k::T1Job>(), (int)nj, djpg, sl->dj2c.as<uint32_t>(), sl->dj2t.as(), nslots,
                          maxw, maxh, st))
        return false;
    }
  }
  // pixels: each page from its packed coefficients into its input slot
  off = 0;
  int k = 0;
  int64_t cb = 0;
  for (int p = 0; p < npages; p++) {
    JpegPage& jp = sl->jpg[(size_t)p];
    if (!jp.on) continue;
    int64_t pitch = 0;
    uint8_t* dst = (uint8_t*)uphip_batch_input_ptr(sl->b, p, &pitch);
    if (jp.j2k) {
      if (!dst || !j2k::decode_launch(jp.img, sl->dj2c.as<uint32_t>() + cb, dst, pitch, dscr, st)) return false;
      cb += jp.img.coef_elems;
      off += up256(jp.bytes);
      continue;
    }
    const uint8_t* packed = jp.dev ? hjob[k++].packed : djpg + off;
    if (!dst || !jpeg_launch(jp.h, packed, dscr, dst, pitch, st)) return false;
    off += up256(jp.bytes);
  }
  return true;
}

// Queue the chunk's device-route TIFF pages on the slot's stream: one upload
// per blob, the jobs and page records of all of them (offsets made
// chunk-wide), then one launch of the strips and one of the rows into the
// pages' input slots (after the staging upload, before the run).
bool tiff_submit(Slot* sl, int npages) {
  size_t in_bytes = 0, njobs = 0, npg = 0;
  uint64_t raster = 0;
  bool lzw = false;
  int maxh = 0;
  sl->tdev = false;
  for (int p = 0; p < npages; p++) {
    const TiffPage& tp = sl->tif[(size_t)p];
    if (!tp.on) continue;
    in_bytes += up256(tp.bytes);
    njobs += tp.jobs.size();
    raster += (tp.raster + 255) & ~(uint64_t)255;
    lzw |= tp.lzw;
    maxh = std::max(maxh, tp.rows.height);
    npg++;
  }
  if (!npg) return true;
  const size_t jb = up256(sizeof(tiff::StripJob) * njobs), rb = up256(sizeof(tiff::RowsPage) * npg);
  auto grow = [](Buffer& b, size_t need) { return b.reserve(need, need / 4); };
  if (!grow(sl->dtif, in_bytes + jb + rb) || !grow(sl->htif, jb + rb) || !grow(sl->dtsc, (size_t)raster) ||
      !grow(sl->dtst, 4 * (size_t)npages) ||
      (lzw && !sl->dtpl.reserve((size_t)tiff::strip_lanes((int64_t)njobs) * tiff::kTableBytes)))
    return false;
  hipStream_t st = (hipStream_t)uphip_batch_stream(sl->b);
  sl->tdev = true;
  tiff::StripJob* hj = sl->htif.as<tiff::StripJob>();
  tiff::RowsPage* hr = (tiff::RowsPage*)(sl->htif.as() + jb);
  uint8_t* const din = sl->dtif.as();
  size_t io = 0, q = 0, k = 0;
  uint64_t so = 0;
  for (int p = 0; p < npages; p++) {
    const TiffPage& tp = sl->tif[(size_t)p];
    if (!tp.on) continue;
    if (!UPH_HIP(hipMemcpyAsync(din + io, tp.host.as(), tp.bytes, hipMemcpyHostToDevice, st))) return false;
    for (tiff::StripJob j : tp.jobs) {
      j.in_off += io;
      j.out_off += so;
      j.page = p;
      hj[q++] = j;
    }
    tiff::RowsPage rp = tp.rows;
    rp.src_off += so;
    rp.pal_off += io;
    rp.page = p;
    rp.dst = (uint8_t*)uphip_batch_input_ptr(sl->b, p, &rp.pitch);
    if (!rp.dst) return false;
    hr[k++] = rp;
    io += up256(tp.bytes);
    so += (tp.raster + 255) & ~(uint64_t)255;
  }
  return UPH_HIP(hipMemcpyAsync(din + in_bytes, sl->htif.as(), jb + rb, hipMemcpyHostToDevice, st)) &&
         UPH_HIP(hipMemsetAsync(sl->dtst.as(), 0, 4 * (size_t)npages, st)) &&
         tiff::launch((const tiff::StripJob*)(din + in_bytes), (int)njobs, lzw,
                      (const tiff::RowsPage*)(din + in_bytes + jb), (int)npg, maxh, din, in_bytes, sl->dtsc.as(),
                      raster, sl->dtpl.as<uint16_t>(), sl->dtst.as<int32_t>(), st);
}

// The chunk's output pages as lossless JPEG 2000 code-blocks, queued on the
// batch's stream once its run has finished: per sub-batch of pages the
// forward transforms of each page, one code-block launch, the packing into
// one buffer (offsets chained across sub-batches); then the offsets, lengths
// and plane counts to pinned memory.  The store tasks copy each page's
// packed bytes and write its packets and file.
bool jp2_chunk_submit(UphipRunner* r, Slot* sl, int npg) {
  if (npg <= 0) return true;
  std::vector<const uint8_t*> src((size_t)npg);
  int64_t pitch = 0;
  int32_t w = 0, h = 0, fmt = 0;
  for (int i = 0; i < npg; i++) {
    const void* p = nullptr;
    if (uphip_batch_jpeg_page(sl->b, i, &p, &pitch, &w, &h, &fmt) != 0) return false;
    src[(size_t)i] = (const uint8_t*)p;
  }
  if (fmt != UPHIP_FMT_GRAY8 && fmt != UPHIP_FMT_RGB24) return fail("sink_jp2: GRAY8 or RGB24 sheets only");
  j2k::Image& img = sl->j2img;
  std::vector<j2k::T1EncJob> page;
  size_t obytes = 0;
  if (!j2k::encode_geometry(w, h, fmt == UPHIP_FMT_GRAY8 ? 1 : 3, &img) ||
      !j2k::encode_jobs(img, &page, &obytes))
    return false;
  const int J = (int)page.size();
  sl->j2jobs = J;
  int maxw = 1, maxh = 1;
  for (const j2k::T1EncJob& j : page) {
    maxw = std::max(maxw, (int)j.w);
    maxh = std::max(maxh, (int)j.h);
  }
  const int P = std::min(npg, kJ2kSubBatch);
  const int nslots = std::min((P * J + 63) / 64, 1024);
  const size_t cb = up256((size_t)P * img.coef_elems * 4), tb = up256((size_t)img.coef_elems * 4);
  const size_t ob = up256((size_t)P * obytes), sb = up256((size_t)nslots * j2k::t1enc_slot_bytes(maxw, maxh));
  const size_t jb = up256(sizeof(j2k::T1EncJob) * (size_t)P * J);
  const size_t nj = (size_t)npg * J;
  const size_t lb = up256(4 * nj), fb = up256(4 * (nj + 1)), nb = up256(nj), eb = 256;
  // packed codewords: the pages' raw bytes and a half more (lossless files
  // of 8-bit pages stay below their samples); a chunk past it fails loudly
  const uint64_t pk = (uint64_t)npg * ((uint64_t)img.coef_elems * 3 / 2 + 65536);
  const size_t need = cb + tb + ob + sb + jb + lb + fb + nb + eb + up256(pk);
  const size_t hjobs = jb;
  const size_t hneed = hjobs + 4 * (nj + 1) + 4 * nj + nj + 64;
  if (!sl->dj2e.reserve(need) || !sl->hj2e.reserve(hneed)) return false;
  uint8_t* a = sl->dj2e.as();
  uint32_t* dcoef = (uint32_t*)a;
  void* dtmp = a + cb;
  uint8_t* dout = a + cb + tb;
  void* dscr = a + cb + tb + ob;
  j2k::T1EncJob* djobs = (j2k::T1EncJob*)(a + cb + tb + ob + sb);
  uint32_t* dlen = (uint32_t*)(a + cb + tb + ob + sb + jb);
  uint32_t* doff = (uint32_t*)(a + cb + tb + ob + sb + jb + lb);
  uint8_t* dnb = a + cb + tb + ob + sb + jb + lb + fb;
  int32_t* derr = (int32_t*)(a + cb + tb + ob + sb + jb + lb + fb + nb);
  uint8_t* dpk = a + cb + tb + ob + sb + jb + lb + fb + nb + eb;
  sl->dj2pk = dpk;
  hipStream_t st = (hipStream_t)uphip_batch_stream(sl->b);
  // the jobs of a sub-batch: page p's blocks with its coefficient and output
  // offsets (the same for every sub-batch: staged once)
  j2k::T1EncJob* sub = sl->hj2e.as<j2k::T1EncJob>();  // pinned: the copy is asynchronous
  for (int p = 0; p < P; p++)
    for (int i = 0; i < J; i++) {
      j2k::T1EncJob t = page[(size_t)i];
      t.in += (int64_t)p * img.coef_elems;
      t.out += (uint32_t)((size_t)p * obytes);
      sub[(size_t)p * J + i] = t;
    }
  if (!UPH_HIP(hipMemcpyAsync(djobs, sub, sizeof(j2k::T1EncJob) * (size_t)P * J, hipMemcpyHostToDevice, st)) ||
      !UPH_HIP(hipMemsetAsync(doff, 0, 4, st)) || !UPH_HIP(hipMemsetAsync(derr, 0, 4, st)))
    return false;
  for (int p0 = 0; p0 < npg; p0 += P) {
    const int n = std::min(P, npg - p0);
    for (int p = 0; p < n; p++)
      if (!j2k::encode_launch(img, src[(size_t)(p0 + p)], pitch, dcoef + (size_t)p * img.coef_elems, dtmp, st))
        return false;
    const size_t j0 = (size_t)p0 * J;
    if (!j2k::t1enc_launch(djobs, n * J, dcoef, dout, dlen + j0, dnb + j0, dscr, nslots, maxw, maxh, st) ||
        !j2k::t1enc_pack(djobs, n * J, dout, dlen + j0, doff + j0, dpk, pk, derr, true, st))
      return false;
  }
  sl->hj2off = (uint32_t*)(sl->hj2e.as() + hjobs);
  sl->hj2len = sl->hj2off + nj + 1;
  sl->hj2nb = (uint8_t*)(sl->hj2len + nj);
  sl->hj2err = (int32_t*)(((uintptr_t)(sl->hj2nb + nj) + 3) & ~(uintptr_t)3);
  return UPH_HIP(hipMemcpyAsync(sl->hj2off, doff, 4 * (nj + 1), hipMemcpyDeviceToHost, st)) &&
         UPH_HIP(hipMemcpyAsync(sl->hj2len, dlen, 4 * nj, hipMemcpyDeviceToHost, st)) &&
         UPH_HIP(hipMemcpyAsync(sl->hj2nb, dnb, nj, hipMemcpyDeviceToHost, st)) &&
         UPH_HIP(hipMemcpyAsync(sl->hj2err, derr, 4, hipMemcpyDeviceToHost, st));
}

}  // namespace uph
