// kernels_tiff.hip — PackBits and LZW TIFF pages decoded on the device
// (tiff_dec.h): a lane per strip over the decoder of tiff_strip.h, then a wave
// per row for the predictor, the inversion and the palette.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "buffer.h"
#include "runtime.h"
#include "tiff_dec.h"
#include "unpaper_hip.h"

namespace uph {
namespace tiff {

namespace {

constexpr int kStripBlock = 64;  // one wave a block, a strip a lane
constexpr int kRowWaves = 4;     // rows a block of k_tiff_rows

// Lane t decodes jobs t, t + T, ... (T lanes in the grid); its LZW tables are
// the t-th kTableBytes of `pool`.  Every job is checked against the two
// buffers before a byte of it is touched; the decoder checks the rest.
__global__ __launch_bounds__(kStripBlock) void k_tiff_strips(const StripJob* __restrict__ jobs, int njobs,
                                                             const uint8_t* __restrict__ in, uint64_t in_bytes,
                                                             uint8_t* __restrict__ scratch, uint64_t scratch_bytes,
                                                             uint16_t* __restrict__ pool,
                                                             int32_t* __restrict__ status) {
  const int t = (int)blockIdx.x * kStripBlock + (int)threadIdx.x;
  const int T = (int)gridDim.x * kStripBlock;
  uint16_t* pos = pool ? pool + (size_t)t * 2 * kLzwCodes : nullptr;
  uint16_t* len = pool ? pos + kLzwCodes : nullptr;
  for (int j = t; j < njobs; j += T) {
    const StripJob job = jobs[j];
    int32_t st;
    if (job.in_off > in_bytes || job.in_len > in_bytes - job.in_off || job.out_off > scratch_bytes ||
        job.out_len > scratch_bytes - job.out_off) {
      st = kRange;
    } else if (job.comp == kCompPackBits) {
      st = packbits(in + job.in_off, job.in_len, scratch + job.out_off, job.out_len);
    } else if (job.comp == kCompLzw && pos) {
      st = lzw<uint16_t>(in + job.in_off, job.in_len, scratch + job.out_off, job.out_len, pos, len);
    } else {
      st = kRange;
    }
    if (st != kOk) atomicOr(status + job.page, st);
  }
}

// Block (x, y): rows [4 x, 4 x + 4) of page y, a wave a row, a lane a pixel
// (a byte of 1-bit data) of every 64.
__global__ __launch_bounds__(kRowWaves * 64) void k_tiff_rows(const RowsPage* __restrict__ pages,
                                                              const uint8_t* __restrict__ in, uint64_t in_bytes,
                                                              const uint8_t* __restrict__ scratch,
                                                              uint64_t scratch_bytes,
                                                              const int32_t* __restrict__ status) {
  const RowsPage pg = pages[blockIdx.y];
  const int y = (int)blockIdx.x * kRowWaves + ((int)threadIdx.x >> 6);
  const int lane = (int)threadIdx.x & 63;
  if (y >= pg.height || status[pg.page] != 0) return;
  const int n = pg.ops.src_bytes, spp = pg.ops.spp;
  if (spp < 1 || spp > 3 || n < 0 || pg.src_off > scratch_bytes ||
      (uint64_t)pg.height * (uint64_t)n > scratch_bytes - pg.src_off)
    return;
  if (pg.ops.palette && (pg.pal_off > in_bytes || in_bytes - pg.pal_off < 768)) return;
  const uint8_t* src = scratch + pg.src_off + (uint64_t)y * (uint64_t)n;
  const uint8_t* pal = in + pg.pal_off;
  uint8_t* dst = pg.dst + (int64_t)y * pg.pitch;
  const int npx = n / spp;
  const bool pred = pg.ops.predictor == 2;
  int carry[3] = {0, 0, 0};
  for (int base = 0; base < npx; base += 64) {
    const int x = base + lane;
    const bool live = x < npx;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      if (c >= spp) break;
      int v = live ? src[x * spp + c] : 0;
      if (pred) {
        // inclusive scan over the wave, then the sum of the pixels before it
        for (int d = 1; d < 64; d <<= 1) {
          const int u = __shfl_up(v, d);
          if (lane >= d) v += u;
        }
        v += carry[c];
        carry[c] = __shfl(v, 63) & 255;
        v &= 255;
      }
      if (!live) continue;
      if (pg.ops.palette) {
        const uint8_t* e = pal + 3 * v;
        dst[3 * x] = e[0];
        dst[3 * x + 1] = e[1];
        dst[3 * x + 2] = e[2];
      } else {
        dst[x * spp + c] = (uint8_t)((pg.ops.invert && c == 0) ? 255 - v : v);
      }
    }
  }
}

}  // namespace

size_t blob_bytes(const Page& p) {
  size_t n = p.ops.palette ? 768 : 0;
  for (uint32_t c : p.cnt) n += c;
  return n;
}

void blob_fill(const Document& doc, const Page& p, uint8_t* blob) {
  size_t o = 0;
  for (size_t s = 0; s < p.off.size(); s++) {
    const uint8_t* in = doc.bytes.data() + p.off[s];
    if (p.fill_order == 2)  // reversed before it is decoded (tiff_strip.h)
      for (uint32_t i = 0; i < p.cnt[s]; i++) blob[o + i] = bitrev8(in[i]);
    else
      memcpy(blob + o, in, p.cnt[s]);
    o += p.cnt[s];
  }
  if (p.ops.palette) memcpy(blob + o, p.pal.data(), 768);
}

void page_jobs(const Page& p, uint64_t in_base, uint64_t out_base, int32_t status_index, StripJob* jobs) {
  uint64_t o = 0;
  for (size_t s = 0; s < p.off.size(); s++) {
    jobs[s] = StripJob{in_base + o,
                       out_base + (uint64_t)s * p.rows_per_strip * (uint64_t)p.src_row_bytes,
                       p.cnt[s],
                       (uint32_t)(p.strip_rows(s) * (uint64_t)p.src_row_bytes),
                       p.compression,
                       status_index};
    o += p.cnt[s];
  }
}

RowsPage rows_page(const Page& p, uint64_t in_base, uint64_t out_base, int32_t status_index, uint8_t* dst,
                   int64_t pitch) {
  return RowsPage{out_base, in_base + blob_bytes(p) - (p.ops.palette ? 768 : 0), dst, pitch, p.height,
                  status_index, p.ops};
}

bool launch(const StripJob* jobs, int njobs, bool any_lzw, const RowsPage* pages, int npages, int max_height,
            const uint8_t* in, uint64_t in_bytes, uint8_t* scratch, uint64_t scratch_bytes, uint16_t* pool,
            int32_t* status, hipStream_t st) {
  if (njobs <= 0 || npages <= 0 || max_height <= 0) return true;
  if (any_lzw && !pool) return fail("tiff: no table pool for LZW strips");
  const int lanes = strip_lanes(njobs);
  k_tiff_strips<<<dim3((unsigned)(lanes / kStripBlock)), dim3(kStripBlock), 0, st>>>(
      jobs, njobs, in, in_bytes, scratch, scratch_bytes, pool, status);
  if (!UPH_HIP(hipGetLastError())) return false;
  k_tiff_rows<<<dim3((unsigned)((max_height + kRowWaves - 1) / kRowWaves), (unsigned)npages),
                dim3(kRowWaves * 64), 0, st>>>(pages, in, in_bytes, scratch, scratch_bytes, status);
  return UPH_HIP(hipGetLastError());
}

}  // namespace tiff
}  // namespace uph

using namespace uph;

extern "C" int uphip_tiff_decode(const void* data, size_t size, int32_t page, void* device_dst, int64_t pitch,
                                 UphipPnmInfo* info) {
  if (!data || !device_dst) return fail("tiff_decode: null argument"), -1;
  if (!runtime_ready()) return fail("tiff_decode: no HIP device"), -1;
  tiff::Document doc;
  const uint8_t* b = (const uint8_t*)data;
  if (!tiff::open(std::vector<uint8_t>(b, b + size), "<memory>", &doc)) return -1;
  const tiff::Page* p = tiff::page(doc, page);
  if (!p) return -1;
  if (info && info->width > 0 &&
      (info->width != p->width || info->height != p->height || info->format != p->format))
    return fail("tiff: page %d is %dx%d format %d, expected %dx%d format %d", page, p->width, p->height,
                p->format, info->width, info->height, info->format),
           -1;
  if (pitch < row_bytes(p->width, p->format)) return fail("tiff_decode: pitch too small"), -1;
  if (!tiff::device_decodable(*p))
    return fail("tiff_decode: page %d (Compression %d, strips of %llu bytes) does not decode on the device: "
                "PackBits or LZW strips of at most 65536 bytes do",
                page, p->compression, (unsigned long long)((uint64_t)p->src_row_bytes * p->rows_per_strip)),
           -1;
  const size_t nj = p->off.size();
  const size_t blob = tiff::blob_bytes(*p), jb = (sizeof(tiff::StripJob) * nj + 255) & ~(size_t)255;
  const size_t pb = 256;  // the page record
  const uint64_t raster = (uint64_t)p->src_row_bytes * (uint64_t)p->height;
  const bool lz = p->compression == tiff::kCompLzw;
  Buffer host{Buffer::Pinned}, dev{Buffer::Device}, scr{Buffer::Device}, pool{Buffer::Device};
  // device: jobs | page record | status | blob
  const size_t head = jb + pb + 256;
  if (!host.reserve(head + blob) || !dev.reserve(head + blob) || !scr.reserve((size_t)raster) ||
      (lz && !pool.reserve((size_t)tiff::strip_lanes((int64_t)nj) * tiff::kTableBytes)))
    return -1;
  memset(host.as(), 0, head);
  tiff::page_jobs(*p, 0, 0, 0, host.as<tiff::StripJob>());
  *(tiff::RowsPage*)(host.as() + jb) = tiff::rows_page(*p, 0, 0, 0, (uint8_t*)device_dst, pitch);
  tiff::blob_fill(doc, *p, host.as() + head);
  hipStream_t st = current_stream();
  int32_t status = 0;
  uint8_t* d = dev.as();
  if (!UPH_HIP(hipMemcpyAsync(d, host.as(), head + blob, hipMemcpyHostToDevice, st)) ||
      !tiff::launch((const tiff::StripJob*)d, (int)nj, lz, (const tiff::RowsPage*)(d + jb), 1, p->height,
                    d + head, blob, scr.as(), raster, pool.as<uint16_t>(), (int32_t*)(d + jb + pb), st) ||
      !UPH_HIP(hipMemcpyAsync(&status, d + jb + pb, 4, hipMemcpyDeviceToHost, st)) ||
      !UPH_HIP(hipStreamSynchronize(st)))
    return -1;
  if (status) return fail("tiff: page %d: %s (device decode)", page, tiff::strip_error(status)), -1;
  if (info) *info = UphipPnmInfo{p->width, p->height, p->format};
  return 0;
}
