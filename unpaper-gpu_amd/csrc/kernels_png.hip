// kernels_png.hip — lossless PNG (zlib) encode of pages on the device
// (png_enc.h): filter, count, table, scan, emit over the core of
// png_enc_core.h, which the host twin (png_enc.cpp) runs too.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "png_enc.h"
#include "png_enc_core.h"
#include "png_enc_dev.h"
#include "runtime.h"
#include "unpaper_hip.h"

namespace uph {

using namespace pngenc;

namespace {

constexpr int kThreads = 256;                    // per block: 4 waves; a lane per segment in the walks
constexpr int kFilterRows = 16;                  // rows a filter block takes at most
constexpr uint32_t kFilterLdsAim = 16u << 10;    // LDS a filter block takes when more than one row fits
constexpr uint32_t kLdsLimit = 160u << 10;       // the CU's LDS (allow_dynamic_lds)

// Block (x, y): rows [x * R, x * R + R) of page y.  LDS: R + 1 rows of
// `stride` words, row -1 of the block first (zeros above the page).
__global__ __launch_bounds__(kThreads) void k_png_filter(PngPages pg, Shape s, int R, int stride, uint8_t* filt,
                                                         int64_t filt_stride) {
  extern __shared__ uint32_t lds[];
  const int tid = (int)threadIdx.x;
  const int p = (int)blockIdx.y;
  const int r0 = (int)blockIdx.x * R;
  if (r0 >= s.height) return;
  const int nrows = min(R, s.height - r0);
  const int64_t row_bits = s.depth == 8 ? s.row_bytes * 8 : (int64_t)s.width;
  // Staging: the aligned dwords that hold a row's samples.  A dword that
  // holds one byte of the row lies in the same 4-byte granule of the
  // allocation, so the up to 3 bytes before and after the row are readable;
  // sample() takes bits [off, off + width) only.
  for (int idx = tid; idx < (nrows + 1) * stride; idx += kThreads) {
    const int q = idx / stride, i = idx - q * stride;
    const int row = r0 - 1 + q;
    uint32_t v = 0;
    if (row >= 0) {
      int bit;
      const uint8_t* a = row_start(pg, s, p, row, &bit);
      const int mis = (int)((uintptr_t)a & 3);
      const int64_t nw = (mis * 8 + bit + row_bits + 31) >> 5;
      if (i < nw) v = ((const uint32_t*)(a - mis))[i];
    }
    lds[idx] = v;
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  for (int r = wave; r < nrows; r += kThreads / 64) {
    const int row = r0 + r;
    int off, up_off = 0;
    const uint8_t* a = row_start(pg, s, p, row, &off);
    const LdsRow cur{(const uint8_t*)(lds + (r + 1) * stride) + ((uintptr_t)a & 3)};
    LdsRow up = cur;
    if (row > 0) {
      a = row_start(pg, s, p, row - 1, &up_off);
      up.p = (const uint8_t*)(lds + r * stride) + ((uintptr_t)a & 3);
    }
    uint32_t sum[3] = {0, 0, 0};
    if (s.depth == 8) {
      filter_sums(cur, off, up, up_off, row > 0, s, lane, 64, sum);
      for (int o = 32; o > 0; o >>= 1) {
        sum[0] += __shfl_xor(sum[0], o);
        sum[1] += __shfl_xor(sum[1], o);
        sum[2] += __shfl_xor(sum[2], o);
      }
    }
    const int f = choose_filter(s, sum);
    uint8_t* dst = filt + p * filt_stride + (int64_t)row * s.line;
    if (lane == 0) dst[0] = (uint8_t)f;
    filter_row(cur, off, up, up_off, row > 0, s, f, lane, 64, dst);
  }
}

// Lane g of page y: segment g's tokens into the block's histogram, flushed
// to the page's counts; the segment's Adler sums.
__global__ __launch_bounds__(kThreads) void k_png_hist(Shape s, const uint8_t* filt, int64_t filt_stride, int64_t nseg,
                                                       PageTab* tabs, uint2* segadler) {
  __shared__ uint32_t h[kSyms];
  const int tid = (int)threadIdx.x;
  const int p = (int)blockIdx.y;
  const int64_t g = (int64_t)blockIdx.x * kThreads + tid;
  for (int i = tid; i < kSyms; i += kThreads) h[i] = 0;
  __syncthreads();
  if (g < nseg) {
    const uint8_t* f = filt + p * filt_stride;
    const int64_t lo = g * kSegBytes, hi = min64(lo + kSegBytes, s.total);
    LdsHist v{h};
    parse_segment(f, lo, hi, s, v);
    uint32_t a, b;
    adler_segment(f + lo, (int)(hi - lo), &a, &b);
    segadler[p * nseg + g] = make_uint2(a, b);
  }
  __syncthreads();
  for (int i = tid; i < kSyms; i += kThreads)
    if (h[i]) atomicAdd(&tabs[p].freq[i], h[i]);
}

// Page blockIdx.x, one wave: the counts to codes.  The lanes place the used
// symbols in sorted order; lane 0 runs the serial build of the core.
__global__ __launch_bounds__(64) void k_png_table(PageTab* tabs) {
  __shared__ PageTab t;
  __shared__ uint16_t ll_order[kLL], dd_order[kDD];
  __shared__ uint32_t work[2 * kLL];
  __shared__ int used[2];
  const int lane = (int)threadIdx.x;
  PageTab* g = tabs + blockIdx.x;
  uint32_t* tw = (uint32_t*)&t;
  constexpr int kWords = (int)(sizeof(PageTab) / 4);
  for (int i = lane; i < kWords; i += 64) tw[i] = i < kSyms ? g->freq[i] : 0u;
  if (lane < 2) used[lane] = 0;
  __syncthreads();
  if (lane == 0) {
    t.freq[kEob]++;
    bool any = false;
    for (int i = 0; i < kDD; i++) any = any || t.freq[kLL + i];
    if (!any) t.freq[kLL] = 1;
  }
  __syncthreads();
  for (int sy = lane; sy < kLL; sy += 64)
    if (t.freq[sy]) {
      ll_order[sorted_place(t.freq, kLL, sy)] = (uint16_t)sy;
      atomicAdd(&used[0], 1);
    }
  if (lane < kDD && t.freq[kLL + lane]) {
    dd_order[sorted_place(t.freq + kLL, kDD, lane)] = (uint16_t)lane;
    atomicAdd(&used[1], 1);
  }
  __syncthreads();
  if (lane == 0) build_tables(&t, ll_order, used[0], dd_order, used[1], work);
  __syncthreads();
  uint32_t* gw = (uint32_t*)g;
  for (int i = lane; i < kWords; i += 64) gw[i] = tw[i];
}

// Lane g of page y: the bits of segment g's tokens.
__global__ __launch_bounds__(kThreads) void k_png_count(Shape s, const uint8_t* filt, int64_t filt_stride,
                                                        int64_t nseg, const PageTab* tabs, int64_t* segoff) {
  __shared__ uint32_t code[kSyms];
  const int tid = (int)threadIdx.x;
  const int p = (int)blockIdx.y;
  const int64_t g = (int64_t)blockIdx.x * kThreads + tid;
  for (int i = tid; i < kSyms; i += kThreads) code[i] = tabs[p].code[i];
  __syncthreads();
  if (g >= nseg) return;
  CountSink cs;
  CodeTokens<CountSink> v(code, cs);
  parse_segment(filt + p * filt_stride, g * kSegBytes, min64((g + 1) * kSegBytes, s.total), s, v);
  segoff[p * nseg + g] = cs.bits;
}

// Page blockIdx.x: the segments' bit counts to their exclusive prefix sums,
// their Adler sums combined, the page's size and form.
__global__ __launch_bounds__(kThreads) void k_png_scan(int64_t total, int64_t nseg, int64_t* segoff,
                                                       const uint2* segadler, PageTab* tabs, int64_t* sizes) {
  __shared__ int64_t part[kThreads];
  __shared__ uint32_t pa[kThreads], pb[kThreads];
  __shared__ int64_t pn[kThreads];
  int64_t* r = segoff + (int64_t)blockIdx.x * nseg;
  const uint2* ad = segadler + (int64_t)blockIdx.x * nseg;
  const int t = (int)threadIdx.x;
  const int64_t chunk = (nseg + kThreads - 1) / kThreads;
  const int64_t lo = min64(t * chunk, nseg), hi = min64(lo + chunk, nseg);
  int64_t sum = 0, bytes = 0;
  uint32_t A = 0, B = 0;  // the chunk's own sums
  for (int64_t i = lo; i < hi; i++) {
    sum += r[i];
    const int64_t n = min64(kSegBytes, total - i * kSegBytes);
    adler_append(&A, &B, (uint64_t)n, ad[i].x, ad[i].y);
    bytes += n;
  }
  part[t] = sum;
  pa[t] = A;
  pb[t] = B;
  pn[t] = bytes;
  __syncthreads();
  if (t == 0) {
    int64_t run = 0;
    uint32_t a = 1, b = 0;
    for (int i = 0; i < kThreads; i++) {
      const int64_t v = part[i];
      part[i] = run;
      run += v;
      adler_append(&a, &b, (uint64_t)pn[i], pa[i], pb[i]);
    }
    PageTab* pt = tabs + blockIdx.x;
    pt->token_bits = run;
    pt->adler = b << 16 | a;
    decide_size(pt, total);
    sizes[blockIdx.x] = pt->size;
  }
  __syncthreads();
  int64_t at = part[t];
  for (int64_t i = lo; i < hi; i++) {
    const int64_t v = r[i];
    r[i] = at;
    at += v;
  }
}

__global__ void k_png_offsets(const int64_t* sizes, int64_t* offs, int n) {
  if (threadIdx.x || blockIdx.x) return;
  int64_t at = 0;
  for (int i = 0; i < n; i++) {
    offs[i] = at;
    at += sizes[i];
  }
}

// Lane g of page y writes segment g's codes; the page's first lane the
// headers before them, its last lane what ends the stream after them.
__global__ __launch_bounds__(kThreads) void k_png_emit(Shape s, const uint8_t* filt, int64_t filt_stride, int64_t nseg,
                                                       const PageTab* tabs, const int64_t* segoff, const int64_t* offs,
                                                       uint32_t* out) {
  __shared__ uint32_t code[kSyms];
  const int tid = (int)threadIdx.x;
  const int p = (int)blockIdx.y;
  const PageTab& t = tabs[p];
  if (t.stored) return;
  const int64_t g = (int64_t)blockIdx.x * kThreads + tid;
  for (int i = tid; i < kSyms; i += kThreads) code[i] = t.code[i];
  __syncthreads();
  if (g >= nseg) return;
  const int64_t bit0 = offs[p] * 8;
  EmitSink sink(out, g == 0 ? bit0 : bit0 + 16 + t.head_bits + segoff[p * nseg + g]);
  if (g == 0) {
    sink.put(0x78, 8);
    sink.put(0x01, 8);
    put_block_header(t, sink);
  }
  CodeTokens<EmitSink> v(code, sink);
  parse_segment(filt + p * filt_stride, g * kSegBytes, min64((g + 1) * kSegBytes, s.total), s, v);
  if (g == nseg - 1) {
    sink.put(code[kEob] & 0xFFFFu, (int)(code[kEob] >> 16));
    sink.put(0, (8 - sink.n % 8) % 8);  // a page starts on a byte, so the word's bits tell
    for (int k = 0; k < 4; k++) sink.put((t.adler >> (24 - 8 * k)) & 0xFFu, 8);
  }
  sink.finish();
}

// Pages that go out stored: thread i copies filtered bytes i, i + grid, ..
// to their places and writes the header of a block that starts at its byte.
__global__ __launch_bounds__(kThreads) void k_png_stored(Shape s, const uint8_t* filt, int64_t filt_stride,
                                                         const PageTab* tabs, const int64_t* offs, uint8_t* out) {
  const int p = (int)blockIdx.y;
  const PageTab& t = tabs[p];
  if (!t.stored) return;
  uint8_t* o = out + offs[p];
  const uint8_t* f = filt + p * filt_stride;
  const int64_t first = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (first == 0) {
    o[0] = 0x78;
    o[1] = 0x01;
    for (int k = 0; k < 4; k++) o[t.size - 4 + k] = (uint8_t)(t.adler >> (24 - 8 * k));
  }
  for (int64_t i = first; i < s.total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t at = stored_place(i);
    if (i % kStoredBlock == 0) {
      uint8_t h[5];
      stored_header(i, s.total, h);
      for (int k = 0; k < 5; k++) o[at - 5 + k] = h[k];
    }
    o[at] = f[i];
  }
}

bool pages_ok(const PngPages& pg, Shape* s, const char* who) {
  if (!pg.plane[0]) return fail("%s: null source", who);
  if (pg.width <= 0 || pg.width > (1 << 20) || pg.height <= 0 || pg.height > (1 << 20))
    return fail("%s: invalid size %dx%d", who, pg.width, pg.height);
  if (!shape_of(pg.format, pg.width, pg.height, s)) return fail("%s: unknown pixel format %d", who, pg.format);
  if (pg.npages <= 0 || pg.npages > 65535 || pg.per_sheet <= 0) return fail("%s: %d pages", who, pg.npages);
  if (pg.offset < 0 || (s->depth == 8 && pg.offset != 0))
    return fail("%s: offset %d on a byte format (offset the pointer instead)", who, pg.offset);
  const int64_t last = (int64_t)pg.offset + (int64_t)(pg.per_sheet - 1) * pg.sheet_width / pg.per_sheet + pg.width;
  const int64_t need = s->depth == 8 ? last * s->channels : (last + 7) / 8;
  if (need > pg.pitch)
    return fail("%s: pixels %d..%lld do not fit rows of %lld bytes", who, pg.offset, (long long)last,
                (long long)pg.pitch);
  return true;
}

}  // namespace

bool png_plan(const Shape& s, PngLaunch* l) {
  // a row's samples start at most 31 bits into its first aligned dword
  const int64_t row_bits = s.depth == 8 ? s.row_bytes * 8 : (int64_t)s.width;
  const int64_t stride = ((row_bits + 31 + 31) / 32) | 1;
  if (2 * stride * 4 > (int64_t)kLdsLimit)
    return fail("k_png_filter: a row of %d pixels and the row above need %lld bytes of LDS, a block has %u",
                s.width, (long long)(2 * stride * 4), kLdsLimit);
  const int64_t fit = (int64_t)kFilterLdsAim / (stride * 4) - 1;
  l->rows = (int32_t)std::min<int64_t>(std::max<int64_t>(fit, 1), kFilterRows);
  l->stride_words = (int32_t)stride;
  l->lds_bytes = (uint32_t)((int64_t)(l->rows + 1) * stride * 4);
  return true;
}

void png_table_launch(PageTab* tabs, unsigned n, hipStream_t st) {
  hipLaunchKernelGGL(k_png_table, dim3(n), dim3(64), 0, st, tabs);
}

PngContext::~PngContext() { if (device >= 0) hipSetDevice(device); }

bool PngContext::encode_async(const PngPages& pg, hipStream_t st) {
  Shape s;
  PngLaunch l;
  if (!pages_ok(pg, &s, "png encode") || !png_plan(s, &l)) return false;
  device = current_device();
  const int64_t nseg = segments_of(s.total);
  const int64_t filt_stride = (s.total + 15) & ~(int64_t)15;
  const size_t np = (size_t)pg.npages;
  const size_t filt_need = (size_t)filt_stride * np;
  const size_t segoff_need = (size_t)nseg * np * sizeof(int64_t);
  const size_t segadler_need = (size_t)nseg * np * sizeof(uint2);
  const size_t tabs_need = np * sizeof(PageTab);
  const size_t meta_need = np * 2 * sizeof(int64_t);
  const size_t out_need = ((size_t)stored_size(s.total) * np + 3) / 4 * 4 + 4;
  const size_t sizes_need = np * sizeof(int64_t);
  if (filt_need > filt.capacity() || segoff_need > segoff.capacity() || segadler_need > segadler.capacity() ||
      tabs_need > tabs.capacity() || meta_need > meta.capacity() || out_need > out.capacity() ||
      sizes_need > host_sizes.capacity()) {
    // the stream's earlier encodes are the only users of the old buffers
    if (!UPH_HIP(hipStreamSynchronize(st))) return false;
    if (!filt.reserve(filt_need) || !segoff.reserve(segoff_need) || !segadler.reserve(segadler_need) ||
        !tabs.reserve(tabs_need) || !meta.reserve(meta_need) || !out.reserve(out_need) ||
        !host_sizes.reserve(sizes_need))
      return false;
  }
  n = pg.npages;
  int64_t* sizes = meta.as<int64_t>();
  int64_t* offs = sizes + pg.npages;
  // the kernels' views of the buffers
  uint8_t* filt = this->filt.as();
  int64_t* segoff = this->segoff.as<int64_t>();
  uint2* segadler = this->segadler.as<uint2>();
  PageTab* tabs = this->tabs.as<PageTab>();
  uint8_t* out = this->out.as();
  if (!UPH_HIP(hipMemsetAsync(out, 0, out_need, st)) || !UPH_HIP(hipMemsetAsync(tabs, 0, tabs_need, st))) return false;
  allow_dynamic_lds((const void*)k_png_filter, l.lds_bytes);
  const unsigned pages = (unsigned)pg.npages;
  const dim3 walk((unsigned)((nseg + kThreads - 1) / kThreads), pages);
  hipLaunchKernelGGL(k_png_filter, dim3((unsigned)((s.height + l.rows - 1) / l.rows), pages), dim3(kThreads),
                     l.lds_bytes, st, pg, s, l.rows, l.stride_words, filt, filt_stride);
  hipLaunchKernelGGL(k_png_hist, walk, dim3(kThreads), 0, st, s, (const uint8_t*)filt, filt_stride, nseg, tabs,
                     segadler);
  png_table_launch(tabs, pages, st);
  hipLaunchKernelGGL(k_png_count, walk, dim3(kThreads), 0, st, s, (const uint8_t*)filt, filt_stride, nseg,
                     (const PageTab*)tabs, segoff);
  hipLaunchKernelGGL(k_png_scan, dim3(pages), dim3(kThreads), 0, st, s.total, nseg, segoff,
                     (const uint2*)segadler, tabs, sizes);
  hipLaunchKernelGGL(k_png_offsets, dim3(1), dim3(1), 0, st, (const int64_t*)sizes, offs, pg.npages);
  hipLaunchKernelGGL(k_png_emit, walk, dim3(kThreads), 0, st, s, (const uint8_t*)filt, filt_stride, nseg,
                     (const PageTab*)tabs, (const int64_t*)segoff, (const int64_t*)offs, (uint32_t*)out);
  const unsigned copy_blocks = (unsigned)std::min<int64_t>((s.total + kThreads * 16 - 1) / (kThreads * 16), 1024);
  hipLaunchKernelGGL(k_png_stored, dim3(copy_blocks, pages), dim3(kThreads), 0, st, s, (const uint8_t*)filt,
                     filt_stride, (const PageTab*)tabs, (const int64_t*)offs, out);
  return UPH_HIP(hipGetLastError()) &&
         UPH_HIP(hipMemcpyAsync(host_sizes.as(), sizes, sizes_need, hipMemcpyDeviceToHost, st));
}

}  // namespace uph

using namespace uph;

extern "C" int64_t uphip_png_encode(const void* device_src, int64_t pitch, int32_t offset, int32_t width,
                                    int32_t height, int32_t format, int32_t dpi, void* out, int64_t capacity) {
  Shape s;
  if (!check_image("png_encode", device_src, pitch, offset, width, height, format, dpi, &s)) return -1;
  if (!runtime_ready()) return fail("png_encode: no HIP device"), -1;
  hipStream_t st = current_stream();
  PngContext c;
  const PngPages pg{{(const uint8_t*)device_src, nullptr}, nullptr, 0, 0, pitch, 1, width, offset,
                    format, width, height, 1};
  if (!c.encode_async(pg, st) || !UPH_HIP(hipStreamSynchronize(st))) return -1;
  const int64_t len = c.host_sizes.as<int64_t>()[0];
  if (len <= 0) return fail("png_encode: the scan gave no size"), -1;
  const int64_t size = uphip_png_wrap("", len, width, height, format, dpi, nullptr, 0);
  if (!out || size < 0) return size;
  if (capacity < size)
    return fail("png_encode: the file needs %lld bytes, the buffer has %lld", (long long)size, (long long)capacity), -1;
  std::vector<uint8_t> z((size_t)len);
  if (!UPH_HIP(hipMemcpyAsync(z.data(), c.out.as(), (size_t)len, hipMemcpyDeviceToHost, st)) ||
      !UPH_HIP(hipStreamSynchronize(st)))
    return -1;
  return uphip_png_wrap(z.data(), len, width, height, format, dpi, out, capacity);
}
