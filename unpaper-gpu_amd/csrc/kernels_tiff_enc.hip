// kernels_tiff_enc.hip — TIFF Deflate encode of pages on the device
// (tiff_enc.h): predict, then hist, table, count, scan, emit per strip over
// the cores of tiff_enc_core.h and png_enc_core.h, which the host twin
// (tiff_write.cpp) runs too.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "png_enc_dev.h"
#include "runtime.h"
#include "tiff_enc.h"
#include "tiff_write.h"
#include "unpaper_hip.h"

namespace uph {

using namespace pngenc;
using tiffenc::Layout;

namespace {

constexpr int kThreads = 256;                  // per block: 4 waves; a lane per segment in the walks
constexpr int kPredictRows = 16;               // rows a predict block takes at most
constexpr uint32_t kPredictLdsAim = 16u << 10; // LDS a predict block takes when more than one row fits
constexpr uint32_t kLdsLimit = 160u << 10;     // the CU's LDS (allow_dynamic_lds)

// The streams of one encode: stream sid is strip sid % nstrips of page
// sid / nstrips.  Its segments' records lie at sid * l.strip_segs.
struct Streams {
  Layout l;
  int64_t filt_stride;
  int32_t nstreams;
};

struct Stream {
  int32_t page, strip;
  int64_t base;   // of its predicted bytes in `filt`
  int64_t total;  // how many they are
};

__device__ inline Stream stream_of(const Streams& S, int sid) {
  Stream t;
  t.page = sid / S.l.nstrips;
  t.strip = sid - t.page * S.l.nstrips;
  t.base = t.page * S.filt_stride + (int64_t)t.strip * S.l.strip_bytes;
  t.total = tiffenc::strip_total(S.l, t.strip);
  return t;
}

// Block (x, y): rows [x * R, x * R + R) of page y.  LDS: R rows of `stride`
// words.
__global__ __launch_bounds__(kThreads) void k_tiff_predict(PngPages pg, Layout l, Shape s, int R, int stride,
                                                           uint8_t* filt, int64_t filt_stride) {
  extern __shared__ uint32_t lds[];
  const int tid = (int)threadIdx.x;
  const int p = (int)blockIdx.y;
  const int r0 = (int)blockIdx.x * R;
  if (r0 >= l.height) return;
  const int nrows = min(R, l.height - r0);
  const int64_t row_bits = l.row_bytes * 8;
  // Staging: the aligned dwords that hold a row's samples (as k_png_filter:
  // the up to 3 bytes before and after the row lie in the same 4-byte
  // granule of the allocation and are not used as samples).
  for (int idx = tid; idx < nrows * stride; idx += kThreads) {
    const int q = idx / stride, i = idx - q * stride;
    int bit;
    const uint8_t* a = row_start(pg, s, p, r0 + q, &bit);
    const int mis = (int)((uintptr_t)a & 3);
    const int64_t nw = (mis * 8 + row_bits + 31) >> 5;
    lds[idx] = i < nw ? ((const uint32_t*)(a - mis))[i] : 0u;
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  for (int r = wave; r < nrows; r += kThreads / 64) {
    const int row = r0 + r;
    int bit;
    const uint8_t* a = row_start(pg, s, p, row, &bit);
    const LdsRow cur{(const uint8_t*)(lds + r * stride) + ((uintptr_t)a & 3)};
    tiffenc::predict_row(cur, l, lane, 64, filt + p * filt_stride + (int64_t)row * l.row_bytes);
  }
}

// Lane g of each stream the block takes: segment g's tokens into the block's
// histogram, flushed to the stream's counts; the segment's Adler sums.
__global__ __launch_bounds__(kThreads) void k_tiff_hist(Streams S, const uint8_t* filt, PageTab* tabs,
                                                        uint2* segadler) {
  __shared__ uint32_t h[kSyms];
  const int tid = (int)threadIdx.x;
  const int64_t g = (int64_t)blockIdx.x * kThreads + tid;
  for (int sid = (int)blockIdx.y; sid < S.nstreams; sid += (int)gridDim.y) {
    for (int i = tid; i < kSyms; i += kThreads) h[i] = 0;
    __syncthreads();
    const Stream t = stream_of(S, sid);
    const int64_t lo = g * kSegBytes;
    if (lo < t.total) {
      const Shape s = tiffenc::strip_shape(S.l, t.total);
      const uint8_t* f = filt + t.base;
      const int64_t hi = min64(lo + kSegBytes, t.total);
      LdsHist v{h};
      parse_segment(f, lo, hi, s, v);
      uint32_t a, b;
      adler_segment(f + lo, (int)(hi - lo), &a, &b);
      segadler[(int64_t)sid * S.l.strip_segs + g] = make_uint2(a, b);
    }
    __syncthreads();
    for (int i = tid; i < kSyms; i += kThreads)
      if (h[i]) atomicAdd(&tabs[sid].freq[i], h[i]);
    __syncthreads();
  }
}

// Lane g of each stream the block takes: the bits of segment g's tokens.
__global__ __launch_bounds__(kThreads) void k_tiff_count(Streams S, const uint8_t* filt, const PageTab* tabs,
                                                         int64_t* segoff) {
  __shared__ uint32_t code[kSyms];
  const int tid = (int)threadIdx.x;
  const int64_t g = (int64_t)blockIdx.x * kThreads + tid;
  for (int sid = (int)blockIdx.y; sid < S.nstreams; sid += (int)gridDim.y) {
    for (int i = tid; i < kSyms; i += kThreads) code[i] = tabs[sid].code[i];
    __syncthreads();
    const Stream t = stream_of(S, sid);
    const int64_t lo = g * kSegBytes;
    if (lo < t.total) {
      const Shape s = tiffenc::strip_shape(S.l, t.total);
      CountSink cs;
      CodeTokens<CountSink> v(code, cs);
      parse_segment(filt + t.base, lo, min64(lo + kSegBytes, t.total), s, v);
      segoff[(int64_t)sid * S.l.strip_segs + g] = cs.bits;
    }
    __syncthreads();
  }
}

// Stream blockIdx.x: the segments' bit counts to their exclusive prefix sums,
// their Adler sums combined, the stream's size and form.
__global__ __launch_bounds__(kThreads) void k_tiff_scan(Streams S, int64_t* segoff, const uint2* segadler,
                                                        PageTab* tabs) {
  __shared__ int64_t part[kThreads];
  __shared__ uint32_t pa[kThreads], pb[kThreads];
  __shared__ int64_t pn[kThreads];
  const int sid = (int)blockIdx.x;
  const int64_t total = stream_of(S, sid).total;
  const int64_t nseg = segments_of(total);
  int64_t* r = segoff + (int64_t)sid * S.l.strip_segs;
  const uint2* ad = segadler + (int64_t)sid * S.l.strip_segs;
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
    PageTab* pt = tabs + sid;
    pt->token_bits = run;
    pt->adler = b << 16 | a;
    decide_size(pt, total);
  }
  __syncthreads();
  int64_t at = part[t];
  for (int64_t i = lo; i < hi; i++) {
    const int64_t v = r[i];
    r[i] = at;
    at += v;
  }
}

// Page blockIdx.x: each strip's place in the page's blob (after the counts)
// and the blob's size.
__global__ __launch_bounds__(kThreads) void k_tiff_pages(Streams S, const PageTab* tabs, int64_t* place,
                                                         int64_t* sizes) {
  __shared__ int64_t part[kThreads];
  const int p = (int)blockIdx.x, t = (int)threadIdx.x;
  const int n = S.l.nstrips;
  const PageTab* pt = tabs + (int64_t)p * n;
  const int chunk = (n + kThreads - 1) / kThreads;
  const int lo = min(t * chunk, n), hi = min(lo + chunk, n);
  int64_t sum = 0;
  for (int i = lo; i < hi; i++) sum += pt[i].size;
  part[t] = sum;
  __syncthreads();
  if (t == 0) {
    int64_t run = 4 * (int64_t)n;
    for (int i = 0; i < kThreads; i++) {
      const int64_t v = part[i];
      part[i] = run;
      run += v;
    }
    sizes[p] = run;
  }
  __syncthreads();
  int64_t at = part[t];
  for (int i = lo; i < hi; i++) {
    place[(int64_t)p * n + i] = at;
    at += pt[i].size;
  }
}

__global__ void k_tiff_offsets(const int64_t* sizes, int64_t* offs, int n) {
  if (threadIdx.x || blockIdx.x) return;
  int64_t at = 0;
  for (int i = 0; i < n; i++) {
    offs[i] = at;
    at += sizes[i];
  }
}

// Thread per stream: its StripByteCounts entry at the head of its page's
// blob; its place made one in the packed output.
__global__ __launch_bounds__(kThreads) void k_tiff_counts(Streams S, const PageTab* tabs, const int64_t* offs,
                                                          int64_t* place, uint8_t* out) {
  const int64_t sid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (sid >= S.nstreams) return;
  const Stream t = stream_of(S, (int)sid);
  const uint32_t n = (uint32_t)tabs[sid].size;
  const int64_t page = offs[t.page];
  uint8_t* o = out + page + 4 * (int64_t)t.strip;
  for (int k = 0; k < 4; k++) o[k] = (uint8_t)(n >> (8 * k));
  place[sid] += page;
}

// Lane g of each coded stream the block takes writes segment g's codes; the
// stream's first lane the headers before them, its last lane what ends the
// stream after them.
__global__ __launch_bounds__(kThreads) void k_tiff_emit(Streams S, const uint8_t* filt, const PageTab* tabs,
                                                        const int64_t* segoff, const int64_t* place,
                                                        uint32_t* out) {
  __shared__ uint32_t code[kSyms];
  const int tid = (int)threadIdx.x;
  const int64_t g = (int64_t)blockIdx.x * kThreads + tid;
  for (int sid = (int)blockIdx.y; sid < S.nstreams; sid += (int)gridDim.y) {
    const PageTab& t = tabs[sid];
    if (t.stored) continue;  // the whole block alike
    for (int i = tid; i < kSyms; i += kThreads) code[i] = t.code[i];
    __syncthreads();
    const Stream st = stream_of(S, sid);
    const int64_t lo = g * kSegBytes;
    if (lo < st.total) {
      const Shape s = tiffenc::strip_shape(S.l, st.total);
      const int64_t bit0 = place[sid] * 8;
      EmitSink sink(out, g == 0 ? bit0 : bit0 + 16 + t.head_bits + segoff[(int64_t)sid * S.l.strip_segs + g]);
      if (g == 0) {
        sink.put(0x78, 8);
        sink.put(0x01, 8);
        put_block_header(t, sink);
      }
      CodeTokens<EmitSink> v(code, sink);
      parse_segment(filt + st.base, lo, min64(lo + kSegBytes, st.total), s, v);
      if (g == segments_of(st.total) - 1) {
        sink.put(code[kEob] & 0xFFFFu, (int)(code[kEob] >> 16));
        // the stream starts on a byte, so the bits in the word tell the padding
        sink.put(0, (8 - sink.n % 8) % 8);
        for (int k = 0; k < 4; k++) sink.put((t.adler >> (24 - 8 * k)) & 0xFFu, 8);
      }
      sink.finish();
    }
    __syncthreads();
  }
}

// Streams that go out stored: thread i copies predicted bytes i, i + grid, ..
// to their places and writes the header of a block that starts at its byte.
__global__ __launch_bounds__(kThreads) void k_tiff_stored(Streams S, const uint8_t* filt, const PageTab* tabs,
                                                          const int64_t* place, uint8_t* out) {
  const int64_t first = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  for (int sid = (int)blockIdx.y; sid < S.nstreams; sid += (int)gridDim.y) {
    const PageTab& t = tabs[sid];
    if (!t.stored) continue;
    const Stream st = stream_of(S, sid);
    uint8_t* o = out + place[sid];
    const uint8_t* f = filt + st.base;
    if (first == 0) {
      o[0] = 0x78;
      o[1] = 0x01;
      for (int k = 0; k < 4; k++) o[t.size - 4 + k] = (uint8_t)(t.adler >> (24 - 8 * k));
    }
    for (int64_t i = first; i < st.total; i += (int64_t)gridDim.x * kThreads) {
      const int64_t at = stored_place(i);
      if (i % kStoredBlock == 0) {
        uint8_t h[5];
        stored_header(i, st.total, h);
        for (int k = 0; k < 5; k++) o[at - 5 + k] = h[k];
      }
      o[at] = f[i];
    }
  }
}

bool pages_ok(const PngPages& pg, Layout* l, const char* who) {
  if (!pg.plane[0]) return fail("%s: null source", who);
  if (pg.width <= 0 || pg.width > (1 << 20) || pg.height <= 0 || pg.height > (1 << 20))
    return fail("%s: invalid size %dx%d", who, pg.width, pg.height);
  if (!tiffenc::layout_of(pg.format, pg.width, pg.height, l))
    return fail("%s: format %d is not Deflate-coded (GRAY8, RGB24 or Y400A)", who, pg.format);
  if (pg.npages <= 0 || pg.npages > 65535 || pg.per_sheet <= 0) return fail("%s: %d pages", who, pg.npages);
  if ((int64_t)pg.npages * l->nstrips > 0x7FFFFFFFll)
    return fail("%s: %d pages of %d strips are more streams than one encode takes", who, pg.npages, l->nstrips);
  if (pg.offset != 0) return fail("%s: offset %d on a byte format (offset the pointer instead)", who, pg.offset);
  const int64_t last = (int64_t)(pg.per_sheet - 1) * pg.sheet_width / pg.per_sheet + pg.width;
  if (last * l->channels > pg.pitch)
    return fail("%s: pixels 0..%lld do not fit rows of %lld bytes", who, (long long)last, (long long)pg.pitch);
  return true;
}

}  // namespace

TiffEncContext::~TiffEncContext() { if (device >= 0) hipSetDevice(device); }

bool TiffEncContext::encode_async(const PngPages& pg, hipStream_t st, int32_t fold) {
  Layout l;
  if (!pages_ok(pg, &l, "tiff encode")) return false;
  if (fold < 1 || fold > kTiffFoldLimit) return fail("k_tiff_hist: a fold limit of %d streams (1..%d)", fold, kTiffFoldLimit);
  // a row's samples start at most 3 bytes into its first aligned dword
  const int64_t stride = ((l.row_bytes * 8 + 31 + 31) / 32) | 1;
  if (stride * 4 > (int64_t)kLdsLimit)
    return fail("k_tiff_predict: a row of %d pixels needs %lld bytes of LDS, a block has %u", l.width,
                (long long)(stride * 4), kLdsLimit);
  const int rows = (int)std::min<int64_t>(std::max<int64_t>((int64_t)kPredictLdsAim / (stride * 4), 1), kPredictRows);
  const uint32_t lds_bytes = (uint32_t)((int64_t)rows * stride * 4);
  device = current_device();
  const size_t np = (size_t)pg.npages;
  const size_t ns = np * (size_t)l.nstrips;
  const Streams S{l, (l.page_bytes + 15) & ~(int64_t)15, (int32_t)ns};
  const Shape s = tiffenc::strip_shape(l, l.page_bytes);  // row_start reads its depth and channels
  const size_t filt_need = (size_t)S.filt_stride * np;
  const size_t segoff_need = ns * (size_t)l.strip_segs * sizeof(int64_t);
  const size_t segadler_need = ns * (size_t)l.strip_segs * sizeof(uint2);
  const size_t tabs_need = ns * sizeof(PageTab);
  const size_t meta_need = (2 * np + ns) * sizeof(int64_t);
  const size_t out_need = ((size_t)tiffenc::blob_bound(l) * np + 3) / 4 * 4 + 4;
  const size_t sizes_need = np * sizeof(int64_t);
  if (lent && (((uintptr_t)lent & 3) || lent_capacity < out_need))
    return fail("tiff encode: the lent output needs %zu bytes on a 4-byte boundary, it has %zu", out_need,
                lent_capacity);
  if (filt_need > filt.capacity() || segoff_need > segoff.capacity() || segadler_need > segadler.capacity() ||
      tabs_need > tabs.capacity() || meta_need > meta.capacity() || (!lent && out_need > out.capacity()) ||
      sizes_need > host_sizes.capacity()) {
    // the stream's earlier encodes are the only users of the old buffers
    if (!UPH_HIP(hipStreamSynchronize(st))) return false;
    if (!filt.reserve(filt_need) || !segoff.reserve(segoff_need) || !segadler.reserve(segadler_need) ||
        !tabs.reserve(tabs_need) || !meta.reserve(meta_need) || (!lent && !out.reserve(out_need)) ||
        !host_sizes.reserve(sizes_need))
      return false;
  }
  n = pg.npages;
  int64_t* sizes = meta.as<int64_t>();
  int64_t* offs = sizes + pg.npages;
  int64_t* place = offs + pg.npages;
  // the kernels' views of the buffers
  uint8_t* filt = this->filt.as();
  int64_t* segoff = this->segoff.as<int64_t>();
  uint2* segadler = this->segadler.as<uint2>();
  PageTab* tabs = this->tabs.as<PageTab>();
  uint8_t* out = packed = lent ? lent : this->out.as();
  if (!UPH_HIP(hipMemsetAsync(out, 0, out_need, st)) || !UPH_HIP(hipMemsetAsync(tabs, 0, tabs_need, st))) return false;
  allow_dynamic_lds((const void*)k_tiff_predict, lds_bytes);
  const unsigned pages = (unsigned)pg.npages, streams = (unsigned)ns;
  const unsigned folded = std::min<unsigned>(streams, (unsigned)fold);
  const dim3 walk((unsigned)((l.strip_segs + kThreads - 1) / kThreads), folded);
  hipLaunchKernelGGL(k_tiff_predict, dim3((unsigned)((l.height + rows - 1) / rows), pages), dim3(kThreads), lds_bytes,
                     st, pg, l, s, rows, (int)stride, filt, S.filt_stride);
  hipLaunchKernelGGL(k_tiff_hist, walk, dim3(kThreads), 0, st, S, (const uint8_t*)filt, tabs, segadler);
  png_table_launch(tabs, streams, st);
  hipLaunchKernelGGL(k_tiff_count, walk, dim3(kThreads), 0, st, S, (const uint8_t*)filt, (const PageTab*)tabs, segoff);
  hipLaunchKernelGGL(k_tiff_scan, dim3(streams), dim3(kThreads), 0, st, S, segoff, (const uint2*)segadler, tabs);
  hipLaunchKernelGGL(k_tiff_pages, dim3(pages), dim3(kThreads), 0, st, S, (const PageTab*)tabs, place, sizes);
  hipLaunchKernelGGL(k_tiff_offsets, dim3(1), dim3(1), 0, st, (const int64_t*)sizes, offs, pg.npages);
  hipLaunchKernelGGL(k_tiff_counts, dim3((streams + kThreads - 1) / kThreads), dim3(kThreads), 0, st, S,
                     (const PageTab*)tabs, (const int64_t*)offs, place, out);
  hipLaunchKernelGGL(k_tiff_emit, walk, dim3(kThreads), 0, st, S, (const uint8_t*)filt, (const PageTab*)tabs,
                     (const int64_t*)segoff, (const int64_t*)place, (uint32_t*)out);
  const unsigned copy_blocks = (unsigned)std::min<int64_t>((l.strip_bytes + kThreads * 16 - 1) / (kThreads * 16), 1024);
  hipLaunchKernelGGL(k_tiff_stored, dim3(copy_blocks, folded), dim3(kThreads), 0, st, S, (const uint8_t*)filt,
                     (const PageTab*)tabs, (const int64_t*)place, out);
  return UPH_HIP(hipGetLastError()) &&
         UPH_HIP(hipMemcpyAsync(host_sizes.as(), sizes, sizes_need, hipMemcpyDeviceToHost, st));
}

namespace {

// `npages` pages coded on the current device and brought to the host: each
// blob's size and the blobs one after another.
bool encode_to_host(const char* who, const PngPages& pg, int32_t fold, uint8_t* lent, size_t lent_capacity,
                    std::vector<int64_t>* sizes, std::vector<uint8_t>* data) {
  if (!runtime_ready()) return fail("%s: no HIP device", who);
  hipStream_t st = current_stream();
  TiffEncContext c;
  c.lent = lent;
  c.lent_capacity = lent_capacity;
  if (!c.encode_async(pg, st, fold) || !UPH_HIP(hipStreamSynchronize(st))) return false;
  int64_t total = 0;
  sizes->assign(c.host_sizes.as<int64_t>(), c.host_sizes.as<int64_t>() + pg.npages);
  for (int64_t n : *sizes) {
    if (n <= 0) return fail("%s: the scan gave a page no size", who);
    total += n;
  }
  data->resize((size_t)total);
  return UPH_HIP(hipMemcpyAsync(data->data(), c.packed, (size_t)total, hipMemcpyDeviceToHost, st)) &&
         UPH_HIP(hipStreamSynchronize(st));
}

}  // namespace

}  // namespace uph

using namespace uph;

extern "C" int64_t uphip_tiff_encode_pages(const void* device_src, int64_t pitch, int64_t page_stride, int32_t npages,
                                           int32_t width, int32_t height, int32_t format, int32_t fold, int64_t* sizes,
                                           void* out, int64_t capacity, void* device_out,
                                           int64_t device_capacity) {
  if (!device_src || page_stride < 0 || device_capacity < 0) return fail("tiff_encode_pages: bad arguments"), -1;
  const PngPages pg{{(const uint8_t*)device_src, nullptr}, nullptr, 0, page_stride, pitch, 1, width, 0,
                    format, width, height, npages};
  std::vector<int64_t> sz;
  std::vector<uint8_t> data;
  if (!encode_to_host("tiff_encode_pages", pg, fold ? fold : kTiffFoldLimit, (uint8_t*)device_out,
                      (size_t)device_capacity, &sz, &data))
    return -1;
  if (sizes) std::copy(sz.begin(), sz.end(), sizes);
  return tiffenc::give_file("tiff_encode_pages", data, out, capacity);
}

extern "C" int64_t uphip_tiff_encode(const void* device_src, int64_t pitch, int32_t offset, int32_t width,
                                     int32_t height, int32_t format, int32_t dpi, void* out, int64_t capacity) {
  tiffenc::Layout l;
  bool bilevel = false;
  if (!tiffenc::check_image("tiff_encode", device_src, pitch, offset, width, height, format, dpi, &l, &bilevel))
    return -1;
  if (!runtime_ready()) return fail("tiff_encode: no HIP device"), -1;
  std::vector<uint8_t> data, file;
  if (bilevel) {
    const int64_t n = uphip_g4_encode(device_src, pitch, offset, width, height, nullptr, 0);
    if (n <= 0) return -1;
    data.resize((size_t)n);
    if (uphip_g4_encode(device_src, pitch, offset, width, height, data.data(), n) != n ||
        !tiff::g4_file(data.data(), data.size(), width, height, dpi ? dpi : 300, &file))
      return -1;
  } else {
    const PngPages pg{{(const uint8_t*)device_src, nullptr}, nullptr, 0, 0, pitch, 1, width, 0,
                      format, width, height, 1};
    std::vector<int64_t> sz;
    if (!encode_to_host("tiff_encode", pg, kTiffFoldLimit, nullptr, 0, &sz, &data) ||
        !tiff::deflate_file(data.data(), data.size(), width, height, format, dpi, &file))
      return -1;
  }
  return tiffenc::give_file("tiff_encode", file, out, capacity);
}
