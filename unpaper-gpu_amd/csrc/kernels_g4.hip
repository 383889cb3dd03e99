// kernels_g4.hip — CCITT Group 4 encode of bilevel pages on the device
// (g4_enc.h): count, scan, emit; a lane per row over the coder of g4_row.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "g4_enc.h"
#include "g4_row.h"
#include "runtime.h"
#include "unpaper_hip.h"

namespace uph {

namespace {

constexpr int kG4Lanes = 64;                       // one wave a block, a row a lane
constexpr int kG4TabWords = 2 * g4::kRunCodes;     // the run-code tables' LDS copy
constexpr uint32_t kG4LdsBudget = 64u << 10;       // dynamic LDS a block may ask for without opting in

// A staged row: big-endian words (pixel order), pixel 0 at bit `off`.  (Every
// search reads its word from LDS: keeping the word read last in registers
// measured 30 % slower on A4 text)
struct LdsRow {
  const uint32_t* w;
  int off;
  __device__ uint32_t word(int i) const { return w[i]; }
};

// Writes codes from bit `at` of the zeroed stream `out` on.  Words that lie
// wholly inside the row's bits are stored; the first word and the last,
// partial one are shared with the neighbouring rows and merged with atomicOr.
struct EmitSink {
  uint32_t* out;
  int64_t w;     // word being filled
  uint64_t acc;  // its bits and the next word's, left-aligned
  int n;         // bits in acc (the first word's bits before `at` count as zeros)
  bool first = true;
  __device__ EmitSink(uint32_t* o, int64_t at) : out(o), w(at >> 5), acc(0), n((int)(at & 31)) {}
  __device__ void put(uint32_t code, int len) {
    acc |= (uint64_t)code << (64 - n - len);
    n += len;
    if (n >= 32) {
      const uint32_t v = __builtin_bswap32((uint32_t)(acc >> 32));  // byte order of the stream
      if (first)
        atomicOr(out + w, v);
      else
        out[w] = v;
      first = false;
      w++;
      acc <<= 32;
      n -= 32;
    }
  }
  __device__ void finish() {
    if (n > 0) atomicOr(out + w, __builtin_bswap32((uint32_t)(acc >> 32)));
  }
};

// The byte that holds pixel 0 of row `row` of page p.
__device__ inline const uint8_t* row_start(const G4Pages& pg, int p, int row, int* bit) {
  const int sheet = p / pg.per_sheet;
  const int64_t b = (int64_t)pg.bit_offset + (int64_t)(p - sheet * pg.per_sheet) * pg.width;
  *bit = (int)(b & 7);
  return pg.base + sheet * pg.sheet_stride + (int64_t)row * pg.pitch + (b >> 3);
}

// Block (x, y): rows [x * R, x * R + R) of page y, lane r the r-th of them.
// LDS: the run-code tables, then R + 1 rows of `stride` words (row -1 of the
// block first: the reference of its first row, zeros above the page).
template <bool kEmit>
__global__ __launch_bounds__(kG4Lanes) void k_g4_rows(G4Pages pg, int R, int stride, int64_t* rowoff,
                                                      const int64_t* sizes, const int64_t* offs,
                                                      uint32_t* out) {
  extern __shared__ uint32_t lds[];
  const int lane = (int)threadIdx.x;
  const int p = (int)blockIdx.y;
  const int r0 = (int)blockIdx.x * R;
  if (r0 >= pg.height) return;
  if (kEmit && sizes[p] < 0) return;  // larger than its share: left out
  const int nrows = min(R, pg.height - r0);
  for (int i = lane; i < kG4TabWords; i += kG4Lanes) lds[i] = (&g4::kRun[0][0])[i];
  uint32_t* rows = lds + kG4TabWords;
  // Staging: the aligned dwords that hold a row's pixels.  A dword that holds
  // one byte of the row lies in the same 4-byte granule of the allocation, so
  // the up to 3 bytes before and after the row are readable; the coder masks
  // them (g4_row.h reads bits [off, off + width) only).
  for (int idx = lane; idx < (nrows + 1) * stride; idx += kG4Lanes) {
    const int q = idx / stride, i = idx - q * stride;
    const int row = r0 - 1 + q;
    uint32_t v = 0;
    if (row >= 0) {
      int bit;
      const uint8_t* a = row_start(pg, p, row, &bit);
      const int mis = (int)((uintptr_t)a & 3);
      const int nw = (mis * 8 + bit + pg.width + 31) >> 5;
      if (i < nw) v = __builtin_bswap32(((const uint32_t*)(a - mis))[i]);
    }
    rows[idx] = v;
  }
  __syncthreads();
  if (lane >= nrows) return;
  const int row = r0 + lane;  // < height
  int bit;
  const uint8_t* a = row_start(pg, p, row, &bit);
  const LdsRow cur{rows + (lane + 1) * stride, (int)((uintptr_t)a & 3) * 8 + bit};
  LdsRow ref{rows + lane * stride, 0};
  if (row > 0) {
    a = row_start(pg, p, row - 1, &bit);
    ref.off = (int)((uintptr_t)a & 3) * 8 + bit;
  }
  const uint32_t(*tab)[g4::kRunCodes] = (const uint32_t(*)[g4::kRunCodes])lds;
  const int64_t slot = (int64_t)p * pg.height + row;
  if (!kEmit) {
    g4::CountSink s;
    g4::encode_row(cur, ref, pg.width, tab, s);
    rowoff[slot] = s.bits;
  } else {
    EmitSink s(out, offs[p] * 8 + rowoff[slot]);
    g4::encode_row(cur, ref, pg.width, tab, s);
    if (row == pg.height - 1) {
      s.put(g4::kEol, g4::kEolBits);
      s.put(g4::kEol, g4::kEolBits);
    }
    s.finish();
  }
}

// Page blockIdx.x: the rows' bit counts to their exclusive prefix sums, the
// page's size in bytes (EOFB and padding included; -1 above `share`).
__global__ __launch_bounds__(256) void k_g4_scan(int H, int64_t* rowoff, int64_t* sizes, int64_t share) {
  __shared__ int64_t part[256];
  int64_t* r = rowoff + (int64_t)blockIdx.x * H;
  const int t = (int)threadIdx.x;
  const int chunk = (H + 255) / 256;
  const int lo = min(t * chunk, H), hi = min(lo + chunk, H);
  int64_t s = 0;
  for (int i = lo; i < hi; i++) s += r[i];
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    int64_t run = 0;
    for (int i = 0; i < 256; i++) {
      const int64_t v = part[i];
      part[i] = run;
      run += v;
    }
    const int64_t bytes = (run + g4::kEofbBits + 7) >> 3;
    sizes[blockIdx.x] = bytes > share ? -1 : bytes;
  }
  __syncthreads();
  int64_t at = part[t];
  for (int i = lo; i < hi; i++) {
    const int64_t v = r[i];
    r[i] = at;
    at += v;
  }
}

__global__ void k_g4_offsets(const int64_t* sizes, int64_t* offs, int n) {
  if (threadIdx.x || blockIdx.x) return;
  int64_t at = 0;
  for (int i = 0; i < n; i++) {
    offs[i] = at;
    if (sizes[i] > 0) at += sizes[i];
  }
}

bool pages_ok(const G4Pages& pg, const char* who) {
  if (!pg.base) return fail("%s: null source", who);
  if (pg.width <= 0 || pg.width > (1 << 20) || pg.height <= 0 || pg.height > (1 << 20))
    return fail("%s: invalid size %dx%d", who, pg.width, pg.height);
  if (pg.npages <= 0 || pg.npages > 65535 || pg.per_sheet <= 0)
    return fail("%s: %d pages", who, pg.npages);
  if (pg.bit_offset < 0 || (int64_t)pg.bit_offset + (int64_t)pg.per_sheet * pg.width > pg.pitch * 8)
    return fail("%s: bits %d..%lld do not fit rows of %lld bytes", who, pg.bit_offset,
                (long long)pg.bit_offset + (long long)pg.per_sheet * pg.width, (long long)pg.pitch);
  return true;
}

}  // namespace

bool g4_plan(int32_t width, G4Launch* l) {
  // a row's pixels start at most 31 bits into its first aligned dword; an odd
  // stride keeps the lanes of a wave (a row each) on different banks
  const int64_t words = ((int64_t)width + 31 + 31) / 32;
  const int64_t stride = words | 1;
  int dev = 0, granted = 0;
  if (!UPH_HIP(hipGetDevice(&dev)) ||
      !UPH_HIP(hipDeviceGetAttribute(&granted, hipDeviceAttributeMaxSharedMemoryPerBlock, dev)))
    return false;
  const int64_t budget = std::min<int64_t>(granted, kG4LdsBudget) - kG4TabWords * 4;
  const int64_t fit = budget / (stride * 4) - 1;  // rows beside the reference row
  if (fit < 1)
    return fail("k_g4_rows: a row of %d pixels and its reference need %lld bytes of LDS, the block has %lld",
                width, (long long)(2 * stride * 4), (long long)budget);
  l->rows = (int32_t)std::min<int64_t>(fit, kG4Lanes);
  l->stride_words = (int32_t)stride;
  l->lds_bytes = (uint32_t)(kG4TabWords * 4 + (int64_t)(l->rows + 1) * stride * 4);
  return true;
}

bool g4_measure(const G4Pages& pg, const G4Launch& l, int64_t* rowoff, int64_t* sizes, int64_t* offs,
                int64_t share, hipStream_t st) {
  const dim3 grid((unsigned)((pg.height + l.rows - 1) / l.rows), (unsigned)pg.npages);
  hipLaunchKernelGGL((k_g4_rows<false>), grid, dim3(kG4Lanes), l.lds_bytes, st, pg, l.rows, l.stride_words,
                     rowoff, (const int64_t*)nullptr, (const int64_t*)nullptr, (uint32_t*)nullptr);
  hipLaunchKernelGGL(k_g4_scan, dim3((unsigned)pg.npages), dim3(256), 0, st, pg.height, rowoff, sizes, share);
  hipLaunchKernelGGL(k_g4_offsets, dim3(1), dim3(1), 0, st, (const int64_t*)sizes, offs, pg.npages);
  return UPH_HIP(hipGetLastError());
}

bool g4_emit(const G4Pages& pg, const G4Launch& l, const int64_t* rowoff, const int64_t* sizes,
             const int64_t* offs, uint8_t* out, hipStream_t st) {
  const dim3 grid((unsigned)((pg.height + l.rows - 1) / l.rows), (unsigned)pg.npages);
  hipLaunchKernelGGL((k_g4_rows<true>), grid, dim3(kG4Lanes), l.lds_bytes, st, pg, l.rows, l.stride_words,
                     (int64_t*)rowoff, sizes, offs, (uint32_t*)out);
  return UPH_HIP(hipGetLastError());
}

G4Context::~G4Context() { if (device >= 0) hipSetDevice(device); }

bool G4Context::encode_async(const G4Pages& pg, int64_t share, hipStream_t st) {
  G4Launch l;
  if (!pages_ok(pg, "g4 encode") || !g4_plan(pg.width, &l)) return false;
  device = current_device();
  const size_t rows_need = (size_t)pg.npages * pg.height * sizeof(int64_t);
  const size_t meta_need = (size_t)pg.npages * 2 * sizeof(int64_t);
  const size_t out_need = ((size_t)share * pg.npages + 3) / 4 * 4 + 4;
  const size_t sizes_need = (size_t)pg.npages * sizeof(int64_t);
  if (rows_need > rowoff.capacity() || meta_need > meta.capacity() || out_need > out.capacity() ||
      sizes_need > host_sizes.capacity()) {
    // the stream's earlier encodes are the only users of the old buffers
    if (!UPH_HIP(hipStreamSynchronize(st))) return false;
    if (!rowoff.reserve(rows_need) || !meta.reserve(meta_need) || !out.reserve(out_need) ||
        !host_sizes.reserve(sizes_need))
      return false;
  }
  n = pg.npages;
  int64_t* sizes = meta.as<int64_t>();
  int64_t* offs = sizes + pg.npages;
  return UPH_HIP(hipMemsetAsync(out.as(), 0, out_need, st)) &&
         g4_measure(pg, l, rowoff.as<int64_t>(), sizes, offs, share, st) &&
         g4_emit(pg, l, rowoff.as<int64_t>(), sizes, offs, out.as(), st) &&
         UPH_HIP(hipMemcpyAsync(host_sizes.as(), sizes, sizes_need, hipMemcpyDeviceToHost, st));
}

}  // namespace uph

using namespace uph;

extern "C" int64_t uphip_g4_encode(const void* device_src, int64_t pitch, int32_t bit_offset, int32_t width,
                                   int32_t height, void* out, int64_t capacity) {
  if (!runtime_ready()) return fail("g4_encode: no HIP device"), -1;
  const G4Pages pg{(const uint8_t*)device_src, 0, pitch, 1, bit_offset, width, height, 1};
  G4Launch l;
  if (!pages_ok(pg, "g4_encode") || !g4_plan(width, &l)) return -1;
  hipStream_t st = current_stream();
  // count, read the size, then emit into a buffer of exactly that size
  Buffer rows(Buffer::Device), stream(Buffer::Device);
  int64_t size = -1;
  bool ok = rows.reserve(sizeof(int64_t) * ((size_t)height + 2));
  if (ok) {
    int64_t* rowoff = rows.as<int64_t>();
    int64_t* sizes = rowoff + height;
    int64_t* offs = sizes + 1;
    ok = g4_measure(pg, l, rowoff, sizes, offs, INT64_MAX, st) &&
         UPH_HIP(hipMemcpyAsync(&size, sizes, sizeof(size), hipMemcpyDeviceToHost, st)) &&
         UPH_HIP(hipStreamSynchronize(st));
    if (ok && size <= 0) ok = fail("g4_encode: the count pass gave no size");
    if (ok && out && capacity >= size) {
      const size_t padded = ((size_t)size + 3) / 4 * 4;  // the last word is written whole
      ok = stream.reserve(padded) && UPH_HIP(hipMemsetAsync(stream.as(), 0, padded, st)) &&
           g4_emit(pg, l, rowoff, sizes, offs, stream.as(), st) &&
           UPH_HIP(hipMemcpyAsync(out, stream.as(), (size_t)size, hipMemcpyDeviceToHost, st));
      ok = UPH_HIP(hipStreamSynchronize(st)) && ok;
    }
  }
  return ok ? size : -1;
}
