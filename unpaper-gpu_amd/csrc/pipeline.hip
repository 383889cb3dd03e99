// pipeline.hip — the batch sheet pipeline: src/core/sheet_stages.c:44-696 for
// a whole batch of sheets at once (the MI355X-native peer of lib/batch_worker.c
// running process_sheet, sheet_process.c:134, per job).  This file holds the
// uphip_batch_* exports and the three encode branches.
//
// Everything that decides SIZES depends only on the options and the input
// geometry, so it is planned on the host once per batch shape, down to every
// argument block that is the same for all sheets (pipeline_plan.hip).
// Everything that depends on PIXELS (masks, rotations, borders, fills) stays
// in HBM: small per-sheet control kernels turn detection results into the
// arguments of the next data kernel, so a batch runs start to finish without a
// host round trip (pipeline_run.hip).  One launch per stage covers every sheet.
#include <cstring>

#include "pipeline_internal.h"

using namespace uph;

namespace {

// The encode sources of a batch's output pages: page i = output page i % oc
// of sheet i / oc, in the plane that holds the sheet (jpeg_enc.h)
__global__ void k_jenc_sources(const SheetCtl* ctl, const uint8_t* p0, const uint8_t* p1,
                               int64_t pitch, int64_t stride, int oc, int64_t page_bytes,
                               JencImage* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int s = i / oc, j = i - s * oc;
  const uint8_t* base = (ctl[s].cur & 1) ? p1 : p0;
  out[i] = JencImage{base + (int64_t)s * stride + (int64_t)j * page_bytes, pitch};
}

int out_pages(const UphipBatch* b) { return b->o.output_count < 1 ? 1 : b->o.output_count; }

// The pages' sizes of a finished packed encode (`what`: jpeg, g4, png), read
// from the encoder's pinned `host_sizes`: each into `sizes` (-1: the page
// outgrew its share of the buffer), their total returned.  A codec without a
// single-page re-encode (missing_ok false) refuses a page without a size.
int64_t packed_sizes(UphipBatch* b, const int64_t* host_sizes, int npages, bool missing_ok, const char* what,
                     int64_t* sizes, int32_t max_pages) {
  if (!host_sizes || npages <= 0) return fail("batch_%s_sizes: no encode", what), -1;
  if (uphip_batch_query(b) != 1) return fail("batch_%s_sizes: the encode has not finished", what), -1;
  int64_t total = 0;
  for (int i = 0; i < npages; i++) {
    const int64_t s = host_sizes[i];
    if (s <= 0 && !missing_ok) return fail("batch_%s_sizes: page %d has no size", what, i), -1;
    if (sizes && i < max_pages) sizes[i] = s < 0 ? -1 : s;
    if (s > 0) total += s;
  }
  return total;
}

// Queue the copy of the `total` packed bytes at `out` into the caller's buffer.
int packed_download(UphipBatch* b, int64_t total, const uint8_t* out, void* host, int64_t capacity,
                    const char* what) {
  if (total == 0) return 0;  // every page came back -1: nothing to copy
  if (!host || capacity < total) return fail("batch_%s_download: buffer too small", what), -1;
  hipSetDevice(b->device);
  return UPH_HIP(hipMemcpyAsync(host, out, (size_t)total, hipMemcpyDeviceToHost, b->st)) ? 0 : -1;
}

}  // namespace

extern "C" {

UphipBatch* uphip_batch_create(const UphipOptions* options, const UphipBatchGeometry* geometry) {
  if (!options || !geometry) return fail("batch_create: null argument"), nullptr;
  if (!runtime_ready()) return fail("batch_create: no HIP device"), nullptr;
  if (geometry->capacity <= 0 || geometry->page_width <= 0 || geometry->page_height <= 0)
    return fail("batch_create: invalid geometry"), nullptr;
  if (options->input_count < 1 || options->input_count > UPHIP_MAX_PAGES)
    return fail("batch_create: input_count must be 1 or 2"), nullptr;
  if (geometry->page_format < UPHIP_FMT_GRAY8 || geometry->page_format > UPHIP_FMT_MONOBLACK)
    return fail("batch_create: invalid page format"), nullptr;
  UphipBatch* b = new UphipBatch();
  b->o = *options;
  b->geo = *geometry;
  b->cap = geometry->capacity;
  b->n_in = options->input_count;
  b->device = current_device();
  hipSetDevice(b->device);
  if (!UPH_HIP(hipStreamCreateWithFlags(&b->st, hipStreamNonBlocking)) || !batch_plan(b) ||
      !batch_allocate(b) || !batch_prepare(b)) {
    uphip_batch_destroy(b);
    return nullptr;
  }
  return b;
}

void uphip_batch_destroy(UphipBatch* b) {
  if (!b) return;
  hipSetDevice(b->device);
  if (b->st) hipStreamSynchronize(b->st);
  for (auto& r : b->runs)
    for (auto& m : r) hipEventDestroy(m.second);
  for (void* p : b->allocs) hipFree(p);
  delete b->jenc;
  delete b->g4;
  delete b->png;
  delete b->tiffenc;
  if (b->st) hipStreamDestroy(b->st);
  delete b;
}

int uphip_batch_output_info(UphipBatch* b, int32_t* width, int32_t* height, int32_t* format,
                            int64_t* bytes_per_sheet) {
  if (!b) return -1;
  if (width) *width = b->out_w;
  if (height) *height = b->out_h;
  if (format) *format = b->out_fmt;
  if (bytes_per_sheet) *bytes_per_sheet = row_bytes(b->out_w, b->out_fmt) * b->out_h;
  return 0;
}

int uphip_batch_device_bytes(UphipBatch* b, int64_t* bytes) {
  if (!b || !bytes) return fail("batch_device_bytes: null argument"), -1;
  *bytes = (int64_t)(b->dev_bytes + (b->png ? b->png->device_bytes() : 0) +
                     (b->tiffenc ? b->tiffenc->device_bytes() : 0));
  return 0;
}

void* uphip_batch_input_ptr(UphipBatch* b, int32_t slot, int64_t* pitch) {
  if (!b || slot < 0 || slot >= b->cap * b->n_in) return nullptr;
  if (pitch) *pitch = b->in_pitch;
  return b->inputs + (int64_t)slot * b->in_page_stride;
}

int uphip_batch_set_page_size(UphipBatch* b, int32_t slot, int32_t width, int32_t height) {
  if (!b) return fail("batch_set_page_size: null batch"), -1;
  if (b->o.sheet_size.width == -1 || b->o.sheet_size.height == -1)
    return fail("batch_set_page_size: options.sheet_size must be fully set (it is %dx%d): without it every "
                "sheet takes its size from its own page", b->o.sheet_size.width, b->o.sheet_size.height), -1;
  if (b->o.pre_rotate != 0)
    return fail("batch_set_page_size: options.pre_rotate is %d, per-slot page sizes need 0", b->o.pre_rotate), -1;
  if (slot < 0 || slot >= b->cap * b->n_in)
    return fail("batch_set_page_size: slot %d out of range (%d slots)", slot, b->cap * b->n_in), -1;
  if ((width == 0) != (height == 0) || width < 0 || width > b->geo.page_width)
    return fail("batch_set_page_size: width %d outside 1..%d (the geometry's page_width)", width,
                b->geo.page_width), -1;
  if (height < 0 || height > b->geo.page_height)
    return fail("batch_set_page_size: height %d outside 1..%d (the geometry's page_height)", height,
                b->geo.page_height), -1;
  if (b->slot_w.empty()) {
    if (width == 0) return 0;  // never sized: the plan's placements stand
    b->slot_w.assign((size_t)b->cap * b->n_in, 0);
    b->slot_h.assign((size_t)b->cap * b->n_in, 0);
  } else if (b->slot_w[(size_t)slot] == width && b->slot_h[(size_t)slot] == height) {
    return 0;  // nothing changes: the next run uploads nothing
  }
  b->slot_w[(size_t)slot] = width;
  b->slot_h[(size_t)slot] = height;
  batch_place(b);
  return 0;
}

int32_t uphip_batch_decode_route(UphipBatch* b) { return b ? b->route : -1; }

int uphip_batch_set_input(UphipBatch* b, int32_t slot, const void* host, int64_t linesize) {
  if (!b || slot < 0 || slot >= b->cap * b->n_in) return fail("batch_set_input: bad slot"), -1;
  hipSetDevice(b->device);
  const bool sized = !b->slot_w.empty() && b->slot_w[(size_t)slot];
  const int32_t w = sized ? b->slot_w[(size_t)slot] : b->geo.page_width;
  const int32_t h = sized ? b->slot_h[(size_t)slot] : b->geo.page_height;
  return UPH_HIP(hipMemcpy2DAsync(b->inputs + (int64_t)slot * b->in_page_stride, b->in_pitch, host,
                                  linesize, row_bytes(w, b->geo.page_format), h, hipMemcpyHostToDevice, b->st))
             ? 0
             : -1;
}

int uphip_batch_run(UphipBatch* b, int32_t count) {
  if (!b || count <= 0 || count > b->cap) return fail("batch_run: bad count"), -1;
  hipSetDevice(b->device);
  return run_batch(b, count, b->inputs, b->in_pitch, b->in_page_stride) ? 0 : -1;
}

int uphip_batch_run_device(UphipBatch* b, int32_t count, const void* pages, int64_t pitch,
                           int64_t page_stride) {
  if (!b || count <= 0 || count > b->cap || !pages)
    return fail("batch_run_device: bad arguments"), -1;
  if (pitch < row_bytes(b->geo.page_width, b->geo.page_format))
    return fail("batch_run_device: pitch too small"), -1;
  hipSetDevice(b->device);
  return run_batch(b, count, (const uint8_t*)pages, pitch, page_stride) ? 0 : -1;
}

int uphip_batch_wait(UphipBatch* b) {
  if (!b) return -1;
  hipSetDevice(b->device);
  if (!UPH_HIP(hipStreamSynchronize(b->st))) return -1;
  // surface device-side failures (overflowing candidate lists / DFS stack) of
  // every run since the previous wait, then re-arm the sticky word
  int32_t any = 0;
  if (!UPH_HIP(hipMemcpy(&any, b->sticky, sizeof(any), hipMemcpyDeviceToHost))) return -1;
  if (!any) return 0;
  UPH_HIP(hipMemset(b->sticky, 0, sizeof(int32_t)));
  std::vector<SheetCtl> c(b->last_count > 0 ? b->last_count : 1);
  if (b->last_count > 0) {
    UPH_HIP(hipMemcpy(c.data(), b->ctl, sizeof(SheetCtl) * b->last_count,
                      hipMemcpyDeviceToHost));
    for (int s = 0; s < b->last_count; s++)
      if (c[s].status)
        return fail("batch: sheet %d failed on the device (status 0x%x)", s, c[s].status), -1;
  }
  return fail("batch: a sheet of an earlier run since the last wait failed on the device "
              "(status 0x%x)", any), -1;
}

void* uphip_batch_output_ptr(UphipBatch* b, int32_t sheet, int64_t* pitch) {
  if (!b || sheet < 0 || sheet >= b->cap) return nullptr;
  // the pointer is handed out only once the batch's kernels have finished
  // writing it (the caller may read it from any stream or the host)
  hipSetDevice(b->device);
  if (!UPH_HIP(hipStreamSynchronize(b->st))) return nullptr;
  if (b->out) {
    if (pitch) *pitch = b->out_pitch;
    return b->out + (int64_t)sheet * b->out_stride;
  }
  int32_t cur = 0;
  hipMemcpy(&cur, &b->ctl[sheet].cur, 4, hipMemcpyDeviceToHost);
  if (pitch) *pitch = b->pitch;
  return b->planes[cur] + (int64_t)sheet * b->plane_stride;
}

int uphip_batch_get_output(UphipBatch* b, int32_t sheet, void* host, int64_t linesize) {
  int64_t pitch = 0;
  void* p = uphip_batch_output_ptr(b, sheet, &pitch);
  if (!p) return fail("batch_get_output: bad sheet"), -1;
  const int64_t rb = row_bytes(b->out_w, b->out_fmt);
  if (linesize < rb) return fail("batch_get_output: linesize too small"), -1;
  if (!UPH_HIP(hipMemcpy2DAsync(host, linesize, p, pitch, rb, b->out_h, hipMemcpyDeviceToHost,
                                b->st)))
    return -1;
  return UPH_HIP(hipStreamSynchronize(b->st)) ? 0 : -1;
}

int uphip_batch_get_report(UphipBatch* b, int32_t sheet, UphipSheetReport* r) {
  if (!b || !r || sheet < 0 || sheet >= b->cap) return -1;
  SheetCtl c;
  hipSetDevice(b->device);
  hipStreamSynchronize(b->st);
  if (!UPH_HIP(hipMemcpy(&c, &b->ctl[sheet], sizeof(c), hipMemcpyDeviceToHost))) return -1;
  memset(r, 0, sizeof(*r));
  r->mask_count = c.mask_count;
  for (int i = 0; i < UPHIP_MAX_PAGES; i++) {
    r->masks[i] = c.masks[i];
    r->rotation[i] = c.rotation[i];
    r->border_masks[i] = c.border_masks[i];
  }
  r->width = b->out_w;
  r->height = b->out_h;
  r->flags = (uint32_t)c.status;
  return 0;
}

int32_t uphip_batch_get_masks(UphipBatch* b, int32_t sheet, UphipRectangle* masks, float* rotations,
                              int32_t capacity) {
  if (!b || sheet < 0 || sheet >= b->cap || capacity < 0)
    return fail("batch_get_masks: bad arguments"), -1;
  SheetCtl c;
  hipSetDevice(b->device);
  hipStreamSynchronize(b->st);
  if (!UPH_HIP(hipMemcpy(&c, &b->ctl[sheet], sizeof(c), hipMemcpyDeviceToHost))) return -1;
  const int32_t n = imin(imin(c.mask_count, capacity), UPHIP_MAX_POINTS);
  // SheetCtl keeps UPHIP_MAX_PAGES rotations; a batch of more points keeps
  // every mask's in rot_all
  std::vector<float> all(b->rot_all ? b->points.size() : 0);
  if (!all.empty() && !UPH_HIP(hipMemcpy(all.data(), b->rot_all + (size_t)sheet * all.size(),
                                         sizeof(float) * all.size(), hipMemcpyDeviceToHost)))
    return -1;
  for (int32_t i = 0; i < n; i++) {
    if (masks) masks[i] = c.masks[i];
    if (rotations)
      rotations[i] = (size_t)i < all.size() ? all[i] : i < UPHIP_MAX_PAGES ? c.rotation[i] : 0.0f;
  }
  return c.mask_count;
}

int uphip_batch_set_mask_scan_route(UphipBatch* b, int32_t route) {
  if (!b) return fail("batch_set_mask_scan_route: null batch"), -1;
  if (route != 0 && route != 1)
    return fail("batch_set_mask_scan_route: unknown route %d (0 one launch, 1 looped)", route), -1;
  b->mask_scan_route = route;
  return 0;
}

void* uphip_batch_stream(UphipBatch* b) { return b ? (void*)b->st : nullptr; }

int uphip_batch_output_pitch(UphipBatch* b, int64_t* pitch) {
  if (!b || !pitch) return -1;
  *pitch = b->out ? b->out_pitch : b->pitch;
  return 0;
}

int uphip_batch_query(UphipBatch* b) {
  if (!b) return -1;
  hipSetDevice(b->device);
  const hipError_t e = hipStreamQuery(b->st);
  if (e == hipSuccess) return 1;
  if (e == hipErrorNotReady) return 0;
  return check_hip(e, "hipStreamQuery"), -1;
}

int uphip_batch_upload_async(UphipBatch* b, int32_t count, const void* host, int64_t linesize,
                             int64_t page_stride) {
  if (!b || !host || count <= 0 || count > b->cap)
    return fail("batch_upload_async: bad arguments"), -1;
  const int64_t rb = row_bytes(b->geo.page_width, b->geo.page_format);
  if (linesize < rb) return fail("batch_upload_async: linesize too small"), -1;
  hipSetDevice(b->device);
  const int64_t n = (int64_t)count * b->n_in;
  const uint8_t* h = (const uint8_t*)host;
  if (linesize == b->in_pitch && page_stride == b->in_page_stride)  // staging laid out like the slots
    return UPH_HIP(hipMemcpyAsync(b->inputs, h, (size_t)(n * page_stride), hipMemcpyHostToDevice,
                                  b->st))
               ? 0
               : -1;
  for (int64_t i = 0; i < n; i++)
    if (!UPH_HIP(hipMemcpy2DAsync(b->inputs + i * b->in_page_stride, b->in_pitch,
                                  h + i * page_stride, linesize, rb, b->geo.page_height,
                                  hipMemcpyHostToDevice, b->st)))
      return -1;
  return 0;
}

int uphip_batch_download_async(UphipBatch* b, void* host, int64_t linesize, int64_t sheet_stride) {
  if (!b || !host || b->last_count <= 0) return fail("batch_download_async: nothing to download"), -1;
  const int64_t rb = row_bytes(b->out_w, b->out_fmt);
  if (linesize < rb) return fail("batch_download_async: linesize too small"), -1;
  hipSetDevice(b->device);
  const hipError_t q = hipStreamQuery(b->st);
  if (q == hipErrorNotReady) return fail("batch_download_async: the run has not finished"), -1;
  if (!check_hip(q, "hipStreamQuery")) return -1;
  const int n = b->last_count;
  // which plane holds each sheet (ctl[s].cur; the stream is idle)
  std::vector<int32_t> cur((size_t)n, 0);
  if (!b->out &&
      !UPH_HIP(hipMemcpy2D(cur.data(), sizeof(int32_t), &b->ctl[0].cur, sizeof(SheetCtl),
                           sizeof(int32_t), n, hipMemcpyDeviceToHost)))
    return -1;
  uint8_t* h = (uint8_t*)host;
  const int64_t sp = b->out ? b->out_pitch : b->pitch;
  const int64_t ss = b->out ? b->out_stride : b->plane_stride;
  auto src_of = [&](int s) -> const uint8_t* {
    return b->out ? b->out + (int64_t)s * ss : b->planes[cur[s] & 1] + (int64_t)s * ss;
  };
  if (linesize == sp && sheet_stride == sp * b->out_h && ss == sheet_stride) {
    // host staging laid out like the planes: runs of sheets in the same plane
    // go as one linear DMA copy (2D copies run far below the link rate); the
    // last sheet of a run ends at its last row, so a caller's buffer need not
    // pad its final sheet to a whole stride
    const int64_t extent = (int64_t)(b->out_h - 1) * sp + rb;
    for (int s = 0; s < n;) {
      int e = s + 1;
      while (e < n && (b->out || (cur[e] & 1) == (cur[s] & 1))) e++;
      if (!UPH_HIP(hipMemcpyAsync(h + s * sheet_stride, src_of(s), (size_t)((e - s - 1) * ss + extent),
                                  hipMemcpyDeviceToHost, b->st)))
        return -1;
      s = e;
    }
    return 0;
  }
  for (int s = 0; s < n; s++)
    if (!UPH_HIP(hipMemcpy2DAsync(h + s * sheet_stride, linesize, src_of(s), sp, rb, b->out_h,
                                  hipMemcpyDeviceToHost, b->st)))
      return -1;
  return 0;
}

// ---- GPU JPEG output branch (sheet_stages.c:554-581) -----------------------
int uphip_batch_encode_jpeg_async(UphipBatch* b, int32_t quality, int32_t sampling) {
  if (!b || b->last_count <= 0) return fail("batch_encode_jpeg: nothing to encode"), -1;
  if (quality == 0) quality = UPHIP_JPEG_DEFAULT_QUALITY;
  hipSetDevice(b->device);
  const int oc = out_pages(b);
  const int n = b->last_count * oc;
  const int bpp = b->work_fmt == F_GRAY8 ? 1 : 3;
  const int32_t pw = b->out_w / oc;
  // bit stream per page: the page's pixel bytes (+64 KiB); pages that do not
  // fit (noise at high quality) come back as -1 for a single re-encode
  const int64_t page = (int64_t)pw * b->out_h * bpp + (64 << 10);
  if (!b->jenc) b->jenc = new JencContext();
  JencContext& c = *b->jenc;
  if (!c.setup(pw, b->out_h, b->work_fmt == F_GRAY8 ? UPHIP_FMT_GRAY8 : UPHIP_FMT_RGB24, sampling,
               quality, n, page / 4, page * n, b->st))
    return -1;
  hipLaunchKernelGGL(k_jenc_sources, dim3((n + 255) / 256), dim3(256), 0, b->st, b->ctl,
                     b->planes[0], b->planes[1], b->pitch, b->plane_stride, oc,
                     (int64_t)pw * bpp, c.B.images, n);
  if (!c.encode_async(b->st)) return -1;
  b->jenc_pages = n;
  return 0;
}

int64_t uphip_batch_jpeg_sizes(UphipBatch* b, int64_t* sizes, int32_t max_pages) {
  return packed_sizes(b, b && b->jenc ? b->jenc->host_sizes.as<int64_t>() : nullptr, b ? b->jenc_pages : 0, true, "jpeg", sizes,
                      max_pages);
}

int uphip_batch_jpeg_download_async(UphipBatch* b, void* host, int64_t capacity) {
  const int64_t total = uphip_batch_jpeg_sizes(b, nullptr, 0);
  return total < 0 ? -1 : packed_download(b, total, b->jenc->out.as(), host, capacity, "jpeg");
}

int uphip_batch_jpeg_page(UphipBatch* b, int32_t page, const void** device_src, int64_t* pitch,
                          int32_t* width, int32_t* height, int32_t* format) {
  const int oc = b ? out_pages(b) : 1;
  if (!b || page < 0 || page >= b->last_count * oc) return fail("batch_jpeg_page: bad page"), -1;
  hipSetDevice(b->device);
  if (!UPH_HIP(hipStreamSynchronize(b->st))) return -1;
  const int s = page / oc, j = page % oc;
  int32_t cur = 0;
  if (!UPH_HIP(hipMemcpy(&cur, &b->ctl[s].cur, 4, hipMemcpyDeviceToHost))) return -1;
  const int bpp = b->work_fmt == F_GRAY8 ? 1 : 3;
  const int32_t pw = b->out_w / oc;
  if (device_src)
    *device_src = b->planes[cur & 1] + (int64_t)s * b->plane_stride + (int64_t)j * pw * bpp;
  if (pitch) *pitch = b->pitch;
  if (width) *width = pw;
  if (height) *height = b->out_h;
  if (format) *format = b->work_fmt == F_GRAY8 ? UPHIP_FMT_GRAY8 : UPHIP_FMT_RGB24;
  return 0;
}

// ---- bilevel output branch: CCITT Group 4 (g4_enc.h) ----------------------
int uphip_batch_encode_g4_async(UphipBatch* b) {
  if (!b || b->last_count <= 0) return fail("batch_encode_g4: nothing to encode"), -1;
  if (b->out_fmt != F_MONOWHITE || !b->out)
    return fail("batch_encode_g4: the batch's output format is %d, Group 4 codes bilevel (MONOWHITE) "
                "sheets only", b->out_fmt), -1;
  hipSetDevice(b->device);
  const int oc = out_pages(b);
  const int32_t pw = b->out_w / oc;
  if (pw <= 0) return fail("batch_encode_g4: empty pages"), -1;
  // a page's share of the packed buffer: its packed rows + 1 KiB (text codes
  // to a small fraction; a noisy page above it comes back as -1)
  const int64_t share = row_bytes(pw, F_MONOWHITE) * b->out_h + 1024;
  if (!b->g4) b->g4 = new G4Context();
  const G4Pages pg{b->out, b->out_stride, b->out_pitch, oc, 0, pw, b->out_h, b->last_count * oc};
  if (!b->g4->encode_async(pg, share, b->st)) return -1;
  b->g4_pages = pg.npages;
  return 0;
}

int64_t uphip_batch_g4_sizes(UphipBatch* b, int64_t* sizes, int32_t max_pages) {
  return packed_sizes(b, b && b->g4 ? b->g4->host_sizes.as<int64_t>() : nullptr, b ? b->g4_pages : 0, true, "g4", sizes,
                      max_pages);
}

int uphip_batch_g4_download_async(UphipBatch* b, void* host, int64_t capacity) {
  const int64_t total = uphip_batch_g4_sizes(b, nullptr, 0);
  return total < 0 ? -1 : packed_download(b, total, b->g4->out.as(), host, capacity, "g4");
}

// ---- lossless output branch: PNG / Flate (png_enc.h) ----------------------
// The output pages of the last run as the lossless encoders address them.
static PngPages output_pages(const UphipBatch* b) {
  const int oc = out_pages(b);
  const int32_t pw = b->out_w / oc;
  if (b->out)
    return PngPages{{b->out, nullptr}, nullptr, 0, b->out_stride, b->out_pitch, oc, b->out_w, 0,
                    (int32_t)b->out_fmt, pw, b->out_h, b->last_count * oc};
  // the sheets lie in the plane their ctl names (as uphip_batch_download_async)
  return PngPages{{b->planes[0], b->planes[1]}, &b->ctl[0].cur, (int64_t)(sizeof(SheetCtl) / sizeof(int32_t)),
                  b->plane_stride, b->pitch, oc, b->out_w, 0, (int32_t)b->out_fmt, pw, b->out_h,
                  b->last_count * oc};
}

int uphip_batch_encode_png_async(UphipBatch* b) {
  if (!b || b->last_count <= 0) return fail("batch_encode_png: nothing to encode"), -1;
  hipSetDevice(b->device);
  const PngPages pg = output_pages(b);
  if (pg.width <= 0) return fail("batch_encode_png: empty pages"), -1;
  if (!b->png) b->png = new PngContext();
  if (!b->png->encode_async(pg, b->st)) return -1;
  b->png_pages = pg.npages;
  return 0;
}

int64_t uphip_batch_png_sizes(UphipBatch* b, int64_t* sizes, int32_t max_pages) {
  return packed_sizes(b, b && b->png ? b->png->host_sizes.as<int64_t>() : nullptr, b ? b->png_pages : 0, false, "png", sizes,
                      max_pages);
}

int uphip_batch_png_download_async(UphipBatch* b, void* host, int64_t capacity) {
  const int64_t total = uphip_batch_png_sizes(b, nullptr, 0);
  return total < 0 ? -1 : packed_download(b, total, b->png->out.as(), host, capacity, "png");
}

// ---- TIFF output branch: Deflate strips (tiff_enc.h) -----------------------
int uphip_batch_encode_tiff_async(UphipBatch* b) {
  if (!b || b->last_count <= 0) return fail("batch_encode_tiff: nothing to encode"), -1;
  if (b->out_fmt != F_GRAY8 && b->out_fmt != F_RGB24)
    return fail("batch_encode_tiff: the batch's output format is %d, Deflate strips code GRAY8 and RGB24 sheets "
                "(bilevel sheets take uphip_batch_encode_g4_async)", b->out_fmt), -1;
  hipSetDevice(b->device);
  const PngPages pg = output_pages(b);
  if (pg.width <= 0) return fail("batch_encode_tiff: empty pages"), -1;
  if (!b->tiffenc) b->tiffenc = new TiffEncContext();
  if (!b->tiffenc->encode_async(pg, b->st)) return -1;
  b->tiff_pages = pg.npages;
  return 0;
}

int64_t uphip_batch_tiff_sizes(UphipBatch* b, int64_t* sizes, int32_t max_pages) {
  return packed_sizes(b, b && b->tiffenc ? b->tiffenc->host_sizes.as<int64_t>() : nullptr, b ? b->tiff_pages : 0,
                      false, "tiff", sizes, max_pages);
}

int uphip_batch_tiff_download_async(UphipBatch* b, void* host, int64_t capacity) {
  const int64_t total = uphip_batch_tiff_sizes(b, nullptr, 0);
  return total < 0 ? -1 : packed_download(b, total, b->tiffenc->out.as(), host, capacity, "tiff");
}

int uphip_batch_set_timing(UphipBatch* b, int32_t enable) {
  if (!b) return -1;
  b->timing = enable != 0;
  return 0;
}

int uphip_batch_kernel_times(UphipBatch* b, const char** names, float* ms, int max_entries) {
  // per-stage totals over every run since the previous query (the events
  // bracket each stage on the batch stream); the record is then cleared
  if (!b) return -1;
  hipSetDevice(b->device);
  if (!UPH_HIP(hipStreamSynchronize(b->st))) return -1;
  std::vector<std::string> order;
  std::vector<double> tot;
  for (auto& r : b->runs) {
    for (size_t i = 1; i < r.size(); i++) {
      float t = 0.0f;
      hipEventElapsedTime(&t, r[i - 1].second, r[i].second);
      size_t k = 0;
      while (k < order.size() && order[k] != r[i].first) k++;
      if (k == order.size()) {
        order.push_back(r[i].first);
        tot.push_back(0.0);
      }
      tot[k] += t;
    }
    for (auto& m : r) hipEventDestroy(m.second);
  }
  b->runs.clear();
  b->time_names = order;
  int k = 0;
  for (; k < (int)order.size() && k < max_entries; k++) {
    if (names) names[k] = b->time_names[k].c_str();
    if (ms) ms[k] = (float)tot[k];
  }
  return k;
}

}  // extern "C"
