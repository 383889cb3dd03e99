// kernels_blur.hip — the blurfilter for gfx950 (the split into a parallel
// pass and an exact resolution: see kernels_gray.hip).
#include "filters_common.h"

namespace uph {

// =========================================================================
// BLURFILTER (filters.c:149-232)
//   Every count the reference takes is of the unmodified image (no wipe ever
//   overlaps a rectangle counted later), so all counts are computed in
//   parallel; the reference's three count rows are pointers into ONE row of
//   its VLA at offsets 0/1/2 that rotate every row, so the wipe decisions are
//   the literal pointer recurrence replayed by one lane over those counts.
//   The slot read before it is written (prev[0] on the first row, an
//   uninitialised stack value in the reference) is 0 here.
// =========================================================================
bool blur_geometry(int32_t W, int32_t H, const UphipBlurfilterParameters& p, uint8_t white,
                   BlurGeom* g) {
  if (p.scan_size.width <= 0 || p.scan_size.height <= 0) return false;
  g->W = W;
  g->H = H;
  g->sw = p.scan_size.width;
  g->sh = p.scan_size.height;
  g->step_y = p.scan_step.vertical;
  g->bpr = (int32_t)((uint32_t)(W / g->sw));
  g->T = H >= g->sh ? (H - g->sh) / g->sh + 1 : 0;
  g->nrect = g->bpr + g->T * (g->bpr + 1);
  g->white = white;
  g->intensity = p.intensity;
  return true;
}

// Per sheet: [nrect] u32 counts, [T * bpr] wipe flags, then k_blur_resolve's
// three count rows for the geometries whose counts do not fit LDS.
UPH_HD size_t blur_rows_off(const BlurGeom& g) {
  const size_t b = (size_t)g.nrect * 4 + (size_t)g.T * (g.bpr > 0 ? g.bpr : 1);
  return (b + 7) & ~(size_t)7;
}
size_t blur_scratch_bytes(const BlurGeom& g) {
  const size_t b = blur_rows_off(g) + sizeof(uint64_t) * 3 * (size_t)(g.bpr + 2);
  return (b + 255) & ~(size_t)255;
}

__device__ __forceinline__ void blur_rect_origin(const BlurGeom& g, int32_t r, int32_t* x,
                                                 int32_t* y) {
  if (r < g.bpr) {
    *x = r * g.sw;
    *y = 0;
  } else {
    const int32_t q = r - g.bpr, t = q / (g.bpr + 1), j = q % (g.bpr + 1);
    *x = j * g.sw;
    *y = t * g.sh + g.step_y;
  }
}

// k_blur_counts for a gray plane: one workgroup per row of rectangles (the
// first row at y = 0, row t at step_y + t*sh).  Lanes count dark pixels
// (gray <= white) of aligned dwords over the strip's rows into per-column
// 16-bit totals in LDS, then one lane per rectangle adds its sw columns.
// V16: 16-byte loads, 16 columns a lane (A/B 146.5 -> 140.6 us a launch
// against 4-byte loads); the host takes it only for planes whose bases,
// stride and pitch are 16-byte aligned with pitch >= round16(W), so the last
// vector of a row stays inside the row.
template <bool V16>
__global__ void __launch_bounds__(256) k_blur_counts_g(PlaneRef img, BlurGeom g, uint8_t* scratch,
                                                       int64_t sstride) {
  const int s = blockIdx.y;
  const int32_t row = blockIdx.x;  // 0: the top row of rectangles, 1 + t: row t
  const int32_t ry = row == 0 ? 0 : (row - 1) * g.sh + g.step_y;
  const int32_t y0 = imax(ry, 0), y1 = imin(ry + g.sh, g.H);  // [y0, y1)
  const uint8_t* base = plane_ptr(img, s);
  extern __shared__ uint16_t ccount[];
  // V16: a lane counts 16 columns, 8 rows' loads in flight
  const int32_t nv = V16 ? (g.W + 15) >> 4 : 0;
  for (int32_t vi = threadIdx.x; vi < nv; vi += 256) {
    uint32_t c[16];
#pragma unroll
    for (int j = 0; j < 16; j++) c[j] = 0;
    for (int32_t y = y0; y < y1; y += 8) {
      uint4 v[8];
#pragma unroll
      for (int k = 0; k < 8; k++)
        v[k] = *reinterpret_cast<const uint4*>(base + (int64_t)imin(y + k, y1 - 1) * img.P.pitch + 16 * vi);
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const uint32_t keep = y + k < y1 ? 1u : 0u;
        const uint32_t w4[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
          for (int j = 0; j < 4; j++) c[4 * q + j] += keep & (((w4[q] >> (8 * j)) & 0xFF) <= g.white ? 1u : 0u);
      }
    }
#pragma unroll
    for (int j = 0; j < 16; j++)
      if (16 * vi + j < g.W) ccount[16 * vi + j] = (uint16_t)c[j];
  }
  const int32_t nd = V16 ? 0 : (g.W + 3) >> 2;
  for (int32_t d = threadIdx.x; d < nd; d += 256) {
    uint32_t c[4] = {0, 0, 0, 0};
    for (int32_t y = y0; y < y1; y += 8) {
      uint32_t v[8];
#pragma unroll
      for (int k = 0; k < 8; k++)
        v[k] = *reinterpret_cast<const uint32_t*>(base + (int64_t)imin(y + k, y1 - 1) * img.P.pitch +
                                                  4 * d);
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const uint32_t keep = y + k < y1 ? 1u : 0u;
#pragma unroll
        for (int j = 0; j < 4; j++) c[j] += keep & (((v[k] >> (8 * j)) & 0xFF) <= g.white ? 1u : 0u);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) ccount[4 * d + j] = (uint16_t)c[j];
  }
  __syncthreads();
  const int32_t nr = row == 0 ? g.bpr : g.bpr + 1;
  uint32_t* counts = (uint32_t*)(scratch + s * sstride);
  for (int32_t j = threadIdx.x; j < nr; j += 256) {
    const int32_t x0 = imax(j * g.sw, 0), x1 = imin(j * g.sw + g.sw, g.W);
    uint32_t n = 0;
    if (y0 < y1)
      for (int32_t x = x0; x < x1; x++) n += ccount[x];
    counts[row == 0 ? j : g.bpr + (row - 1) * (g.bpr + 1) + j] = n;
  }
}

// k_blur_counts_g from the bit-plane of pixels <= white (1/8 of the plane's
// bytes; SheetBits::bbits, kept current by the black- and noisefilter's
// clears).  Rectangles at least 32 wide, so a 32-pixel word meets at most two
// of them: a lane per (word column, row phase) keeps two popcount sums over
// its rows of the strip, then adds them into per-rectangle LDS counters.
__global__ void __launch_bounds__(256) k_blur_counts_bits(BlurGeom g, const uint32_t* bbits,
                                                          int64_t bb_stride, uint8_t* scratch,
                                                          int64_t sstride) {
  const int s = blockIdx.y;
  const int32_t row = blockIdx.x;
  const int32_t ry = row == 0 ? 0 : (row - 1) * g.sh + g.step_y;
  const int32_t y0 = imax(ry, 0), y1 = imin(ry + g.sh, g.H);
  const int32_t nr = row == 0 ? g.bpr : g.bpr + 1;
  const int32_t nwr = (g.W + 31) >> 5;
  extern __shared__ uint32_t rcount[];
  for (int32_t j = threadIdx.x; j < nr + 1; j += 256) rcount[j] = 0;
  __syncthreads();
  const uint32_t* plane = bbits + s * bb_stride;
  const int32_t nph = nwr >= 256 ? 1 : 256 / nwr;  // row phases
  const int32_t lanes = nph * nwr;
  for (int32_t t = threadIdx.x; t < (nwr >= 256 ? nwr : lanes); t += 256) {
    const int32_t wi = nwr >= 256 ? t : t % nwr, ph = nwr >= 256 ? 0 : t / nwr;
    const int32_t x0 = 32 * wi;
    const int32_t j0 = x0 / g.sw;
    // bits [0, cut) of a word belong to rectangle j0, [cut, 32) to j0 + 1
    const int32_t cut = imin((j0 + 1) * g.sw - x0, 32);
    const uint32_t m0 = cut >= 32 ? ~0u : (1u << cut) - 1u;
    uint32_t a0 = 0, a1 = 0;
    const uint32_t* col = plane + wi;
    int32_t y = y0 + ph;
    for (; y + 3 * nph < y1; y += 4 * nph) {
      uint32_t v[4];
#pragma unroll
      for (int k = 0; k < 4; k++) v[k] = col[(int64_t)(y + k * nph) * nwr];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        a0 += __popc(v[k] & m0);
        a1 += __popc(v[k] & ~m0);
      }
    }
    for (; y < y1; y += nph) {
      const uint32_t v = col[(int64_t)y * nwr];
      a0 += __popc(v & m0);
      a1 += __popc(v & ~m0);
    }
    if (a0 && j0 < nr) atomicAdd(&rcount[j0], a0);
    if (a1 && j0 + 1 < nr) atomicAdd(&rcount[j0 + 1], a1);
  }
  __syncthreads();
  uint32_t* counts = (uint32_t*)(scratch + s * sstride);
  for (int32_t j = threadIdx.x; j < nr; j += 256)
    counts[row == 0 ? j : g.bpr + (row - 1) * (g.bpr + 1) + j] = rcount[j];
}

template <int FMT>
__global__ void __launch_bounds__(256) k_blur_counts(PlaneRef img, BlurGeom g, uint8_t* scratch,
                                                     int64_t sstride) {
  const int s = blockIdx.y;
  const int32_t r = blockIdx.x;
  int32_t rx, ry;
  blur_rect_origin(g, r, &rx, &ry);
  const uint8_t* base = plane_ptr(img, s);
  // count_pixels_within_brightness(0, white): unclipped, outside = white
  const int32_t x0 = imax(rx, 0), x1 = imin(rx + g.sw - 1, g.W - 1);
  const int32_t y0 = imax(ry, 0), y1 = imin(ry + g.sh - 1, g.H - 1);
  uint32_t acc = 0;
  if (x0 <= x1 && y0 <= y1) {
    const int32_t w = x1 - x0 + 1;
    const int32_t n = w * (y1 - y0 + 1);
    for (int32_t i = threadIdx.x; i < n; i += 256) {
      const int32_t yy = y0 + i / w, xx = x0 + i % w;
      acc += gray_of(load_px_row<FMT>(base + (int64_t)yy * img.P.pitch, xx)) <= g.white ? 1u : 0u;
    }
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  __shared__ uint32_t red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t* counts = (uint32_t*)(scratch + s * sstride);
    counts[r] = red[0] + red[1] + red[2] + red[3];
  }
}

// IN_LDS: the counts and the three rows staged in LDS; else (more counted
// rectangles than LDS holds: blur_resolve_arm) the counts read where they are
// and the rows in the sheet's scratch.
template <bool IN_LDS>
__global__ void __launch_bounds__(256) k_blur_resolve(BlurGeom g, uint8_t* scratch,
                                                      int64_t sstride) {
  const int s = blockIdx.x;
  const uint32_t* counts = (const uint32_t*)(scratch + s * sstride);
  uint8_t* wipe = scratch + s * sstride + (size_t)g.nrect * 4;
  extern __shared__ uint64_t sh[];  // [nrect] counts + [3*(bpr+2)] buffers
  uint64_t* cnt = sh;
  uint64_t* buf = IN_LDS ? sh + g.nrect : (uint64_t*)(scratch + s * sstride + blur_rows_off(g));
  const int32_t nbuf = 3 * (g.bpr + 2);
  if (IN_LDS)
    for (int32_t i = threadIdx.x; i < g.nrect; i += blockDim.x) cnt[i] = counts[i];
  for (int32_t i = threadIdx.x; i < nbuf; i += blockDim.x) buf[i] = 0;
  for (int32_t i = threadIdx.x; i < g.T * g.bpr; i += blockDim.x) wipe[i] = 0;
  __syncthreads();
  if (threadIdx.x != 0) return;
  const uint64_t total = (uint64_t)(g.sw * g.sh);
  const int32_t bpr = g.bpr;
  int32_t op = 0, oc = 1, on = 2;  // prev / cur / next offsets into buf
  buf[oc + 0] = total;
  buf[oc + bpr] = total;
  buf[on + 0] = total;
  buf[on + bpr] = total;
  const auto count = [&](int32_t i) -> uint64_t { return IN_LDS ? cnt[i] : (uint64_t)counts[i]; };
  for (int32_t b = 0; b < bpr; b++) buf[oc + 1 + b] = count(b);
  for (int32_t t = 0; t < g.T; t++) {
    const int32_t base = bpr + t * (bpr + 1);
    buf[on + 0] = count(base + 0);
    for (int32_t block = 1; block <= bpr; block++) {
      buf[on + block + 1] = count(base + block);
      const uint64_t a = buf[op + block - 1], b = buf[op + block + 1], c = buf[oc + block];
      const uint64_t m1 = a > b ? (a > c ? a : c) : (b > c ? b : c);
      const uint64_t d = buf[on + block - 1], e = buf[on + block + 1];
      const uint64_t mx = d > e ? (d > m1 ? d : m1) : (e > m1 ? e : m1);
      if ((((float)mx) / total) <= g.intensity) {
        wipe[t * bpr + block - 1] = 1;
        buf[oc + block] = total;
      }
    }
    const int32_t tmp = op;
    op = oc;
    oc = on;
    on = tmp;
  }
}

// The same recurrence on the scalar unit, one wave per sheet, for rows of at
// most 56 blocks.  All three pointers of blurfilter_cpu index one array A
// (prev, cur, next at offsets op, oc, on, a rotation of 0, 1, 2), so block k
// of a row reads and writes only A[k-1 .. k+3]: that window lives in scalar
// registers and slides one entry a block.  A itself is one VGPR (lane j holds
// A[j]): the entry leaving the window is written into its lane, the one
// entering (untouched so far in this row) read from its lane; the row's
// counts are a second VGPR.  No memory access inside a row.  With the row's
// rotation the reads are
//   (0,1,2): next[k+1] = A[k+3]; the rest A[k-1], A[k+1] (three times); wipe A[k+1]
//   (1,2,0): next[k+1] = A[k+1]; A[k], A[k+2] (twice), A[k-1];          wipe A[k+2]
//   (2,0,1): next[k+1] = A[k+2]; A[k+1], A[k+3], A[k] (twice);          wipe A[k]
// and the float test ((float)max / total <= intensity) is monotone in max, so
// it is the integer compare max <= tmax with tmax found once per sheet.
__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t lane_get(uint32_t v, int32_t l) {
  return (uint32_t)__builtin_amdgcn_readlane((int32_t)v, l);
}
__device__ __forceinline__ uint32_t lane_set(uint32_t v, uint32_t x, int32_t l) {
  return (int32_t)(threadIdx.x & 63) == l ? x : v;
}

// one row of type OP: blocks 1 .. bpr; returns the row's wipe bits (bit k-1)
// entries 0 .. 127 of an array over two VGPRs (lane l: entries l and 64 + l)
struct Lanes2 {
  uint32_t v0, v1;
};
__device__ __forceinline__ uint32_t lane_get(const Lanes2& v, int32_t l) {
  const uint32_t a = lane_get(v.v0, l & 63), b = lane_get(v.v1, l & 63);
  return l < 64 ? a : b;
}
__device__ __forceinline__ void lane_set(Lanes2& v, uint32_t x, int32_t l) {
  v.v0 = lane_set(v.v0, x, l);
  v.v1 = lane_set(v.v1, x, l - 64);
}

template <int OP>
__device__ __forceinline__ void blur_row(Lanes2& Av, Lanes2 rowv, int32_t bpr, uint32_t total,
                                         int32_t tmax, uint64_t (&wipes)[2]) {
  constexpr int ON = OP == 0 ? 2 : OP == 1 ? 0 : 1;
  uint32_t W0 = lane_get(Av, 0), W1 = lane_get(Av, 1), W2 = lane_get(Av, 2);
  uint32_t W3 = lane_get(Av, 3), W4 = lane_get(Av, 4);
  const uint32_t n0 = lane_get(rowv, 0);  // next[0] = A[on]
  if (ON == 0) W0 = n0;
  else if (ON == 1) W1 = n0;
  else W2 = n0;
  wipes[0] = wipes[1] = 0;  // bit k-1 of the pair: block k
#pragma unroll 4
  for (int32_t k = 1;; k++) {
    const uint32_t e = lane_get(rowv, k);
    uint32_t mx;
    bool w;
    if (OP == 0) {
      W4 = e;
      mx = umax(W0, umax(W2, W4));
      w = (int32_t)mx <= tmax;
      W2 = w ? total : W2;
    } else if (OP == 1) {
      W2 = e;
      mx = umax(umax(W0, W1), umax(W2, W3));
      w = (int32_t)mx <= tmax;
      W3 = w ? total : W3;
    } else {
      W3 = e;
      mx = umax(umax(W1, W2), umax(W3, W4));
      w = (int32_t)mx <= tmax;
      W1 = w ? total : W1;
    }
    const uint64_t bit = (uint64_t)w << ((k - 1) & 63);
    if (k <= 64) wipes[0] |= bit;
    else wipes[1] |= bit;
    if (k == bpr) break;
    lane_set(Av, W0, k - 1);
    W0 = W1;
    W1 = W2;
    W2 = W3;
    W3 = W4;
    W4 = lane_get(Av, k + 4);
  }
  lane_set(Av, W0, bpr - 1);
  lane_set(Av, W1, bpr);
  lane_set(Av, W2, bpr + 1);
  lane_set(Av, W3, bpr + 2);
  lane_set(Av, W4, bpr + 3);
}

// The same row for a row length known at compile time: the whole row's A in
// scalar registers (read from its lanes once, written back once), every
// block a handful of scalar operations.
template <int OP, int BPR>
__device__ __forceinline__ uint64_t blur_row_fixed(uint32_t& Av, uint32_t rowv, uint32_t total,
                                                   int32_t tmax) {
  constexpr int ON = OP == 0 ? 2 : OP == 1 ? 0 : 1;
  uint32_t a[BPR + 4];
#pragma unroll
  for (int j = 0; j < BPR + 4; j++) a[j] = lane_get(Av, j);
  a[ON] = lane_get(rowv, 0);  // next[0]
  uint64_t wipes = 0;
#pragma unroll
  for (int k = 1; k <= BPR; k++) {
    const uint32_t e = lane_get(rowv, k);
    uint32_t mx;
    if (OP == 0) {
      a[k + 3] = e;
      mx = umax(a[k - 1], umax(a[k + 1], a[k + 3]));
    } else if (OP == 1) {
      a[k + 1] = e;
      mx = umax(umax(a[k - 1], a[k]), umax(a[k + 1], a[k + 2]));
    } else {
      a[k + 2] = e;
      mx = umax(umax(a[k], a[k + 1]), umax(a[k + 2], a[k + 3]));
    }
    const bool w = (int32_t)mx <= tmax;
    if (OP == 0) a[k + 1] = w ? total : a[k + 1];
    else if (OP == 1) a[k + 2] = w ? total : a[k + 2];
    else a[k] = w ? total : a[k];
    wipes |= (uint64_t)w << (k - 1);
  }
#pragma unroll
  for (int j = 0; j < BPR + 4; j++) Av = lane_set(Av, a[j], j);
  return wipes;
}

// Rows of 33 .. 112 blocks.  Within a row the recurrence only READS A as it
// was before the row (an entry entering the window, A[k+4] at block k, has
// not been written in this row yet), so the scalar window reads the row's
// A and counts from their lanes and writes nothing back per block; the row's
// final A is then made lane-parallel from its counts and wipe bits (the last
// write of each entry, below), a handful of vector operations a row.
// 16 blocks KC+1 .. KC+16 of a row: their counts and the A entries entering
// the window read from lanes known at compile time up front, then a chain of
// scalar operations per block.  Blocks past bpr run too (their wipe bits are
// masked off; the row's state is rebuilt from the bits, not from the window).
__device__ __forceinline__ uint32_t lane_c(const Lanes2& v, int l) {
  return l < 64 ? lane_get(v.v0, l) : lane_get(v.v1, l - 64);
}
template <int OP, int KC>
__device__ __forceinline__ void blur_chunk_ro(const Lanes2& Aold, const Lanes2& rowv, int32_t bpr,
                                              uint32_t total, int32_t tmax, uint32_t (&W)[5],
                                              uint64_t& w0, uint64_t& w1) {
  if (KC + 1 > bpr) return;
  uint32_t e[16], nx[16];
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const int k = KC + 1 + i;
    e[i] = k < 128 ? lane_c(rowv, k) : 0u;
    nx[i] = k + 4 < 128 ? lane_c(Aold, k + 4) : 0u;
  }
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const int k = KC + 1 + i;
    uint32_t mx;
    bool w;
    if (OP == 0) {
      W[4] = e[i];
      mx = umax(W[0], umax(W[2], W[4]));
      w = (int32_t)mx <= tmax;
      W[2] = w ? total : W[2];
    } else if (OP == 1) {
      W[2] = e[i];
      mx = umax(umax(W[0], W[1]), umax(W[2], W[3]));
      w = (int32_t)mx <= tmax;
      W[3] = w ? total : W[3];
    } else {
      W[3] = e[i];
      mx = umax(umax(W[1], W[2]), umax(W[3], W[4]));
      w = (int32_t)mx <= tmax;
      W[1] = w ? total : W[1];
    }
    if (k <= 64) w0 |= w ? 1ull << (k - 1) : 0ull;
    else if (k <= 128) w1 |= w ? 1ull << (k - 65) : 0ull;
    W[0] = W[1];
    W[1] = W[2];
    W[2] = W[3];
    W[3] = W[4];
    W[4] = nx[i];
  }
}
template <int OP>
__device__ __forceinline__ void blur_row_ro(const Lanes2& Aold, const Lanes2& rowv, int32_t bpr,
                                            uint32_t total, int32_t tmax, uint64_t (&wipes)[2]) {
  constexpr int ON = OP == 0 ? 2 : OP == 1 ? 0 : 1;
  uint32_t W[5];
#pragma unroll
  for (int j = 0; j < 5; j++) W[j] = lane_get(Aold.v0, j);
  W[ON] = lane_get(rowv.v0, 0);  // next[0] = A[on]
  uint64_t w0 = 0, w1 = 0;  // bit k-1: block k
  blur_chunk_ro<OP, 0>(Aold, rowv, bpr, total, tmax, W, w0, w1);
  blur_chunk_ro<OP, 16>(Aold, rowv, bpr, total, tmax, W, w0, w1);
  blur_chunk_ro<OP, 32>(Aold, rowv, bpr, total, tmax, W, w0, w1);
  blur_chunk_ro<OP, 48>(Aold, rowv, bpr, total, tmax, W, w0, w1);
  blur_chunk_ro<OP, 64>(Aold, rowv, bpr, total, tmax, W, w0, w1);
  blur_chunk_ro<OP, 80>(Aold, rowv, bpr, total, tmax, W, w0, w1);
  blur_chunk_ro<OP, 96>(Aold, rowv, bpr, total, tmax, W, w0, w1);
  wipes[0] = bpr >= 64 ? w0 : w0 & ((1ull << bpr) - 1);
  wipes[1] = bpr <= 64 ? 0 : bpr >= 128 ? w1 : w1 & ((1ull << (bpr - 64)) - 1);
}
// The row's final A, entry j per lane (j = lane, 64 + lane): the last write
// of entry j during the row of type OP (next[0] first, then per block k the
// count write and the wipe write):
//   OP 0: count A[k+3] = row[k], wipe A[k+1] = total, next[0] at A[2]
//   OP 1: count A[k+1] = row[k], wipe A[k+2] = total, next[0] at A[0]
//   OP 2: count A[k+2] = row[k], wipe A[k]   = total, next[0] at A[1]
template <int OP>
__device__ __forceinline__ Lanes2 blur_row_state(const Lanes2& Aold, const Lanes2& rowv,
                                                 int32_t bpr, uint32_t total,
                                                 const uint64_t (&wipes)[2]) {
  constexpr int S = OP == 0 ? 3 : OP == 1 ? 1 : 2;  // count shift: A[j] = row[j - S]
  constexpr int ON = OP == 0 ? 2 : OP == 1 ? 0 : 1;
  const int lane = threadIdx.x & 63;
  const uint32_t r0 = lane_get(rowv.v0, 0);
  auto wbit = [&](int32_t k) -> bool {  // block k wiped
    if (k < 1 || k > bpr) return false;
    const uint64_t m = k <= 64 ? wipes[0] : wipes[1];
    return (m >> ((k - 1) & 63)) & 1;
  };
  auto entry = [&](int32_t j, uint32_t old, uint32_t shifted) -> uint32_t {
    // shifted = row[j - S] (valid for j >= S)
    if (OP == 0) {
      if (j >= 2 && j <= bpr + 1 && wbit(j - 1)) return total;
      if (j >= 4 && j <= bpr + 3) return shifted;
      return j == ON ? r0 : old;
    } else if (OP == 1) {
      if (j >= 2 && j <= bpr + 1) return shifted;
      if (j == bpr + 2 && wbit(bpr)) return total;
      return j == ON ? r0 : old;
    } else {
      if (j >= 1 && j <= bpr && wbit(j)) return total;
      if (j >= 3 && j <= bpr + 2) return shifted;
      return j == ON ? r0 : old;
    }
  };
  // row[j - S] for j = lane and j = 64 + lane
  const int src0 = (lane - S) & 63;
  const uint32_t a0 = (uint32_t)__shfl((int)rowv.v0, src0, 64);
  const uint32_t b0 = (uint32_t)__shfl((int)rowv.v1, src0, 64);
  const uint32_t sh0 = a0;                      // lane >= S: row[lane - S] (v0)
  const uint32_t sh1 = lane >= S ? b0 : a0;     // row[64 + lane - S]: v1 or the top of v0
  Lanes2 r;
  r.v0 = entry(lane, Aold.v0, sh0);
  r.v1 = entry(64 + lane, Aold.v1, sh1);
  return r;
}

template <int BPR>
__device__ __forceinline__ void blur_rows_fixed(uint32_t Av, const uint32_t* counts, uint8_t* wipe,
                                                int32_t T, uint32_t total, int32_t tmax) {
  const int lane = threadIdx.x & 63;
  constexpr int32_t rl = BPR + 1;
  uint32_t rowv = T > 0 && lane < rl ? counts[BPR + lane] : 0;
  for (int32_t t = 0; t < T; t++) {
    const uint32_t cur = rowv;
    if (t + 1 < T) rowv = lane < rl ? counts[BPR + (t + 1) * rl + lane] : 0;
    const int op = t % 3;
    const uint64_t wipes = op == 0   ? blur_row_fixed<0, BPR>(Av, cur, total, tmax)
                           : op == 1 ? blur_row_fixed<1, BPR>(Av, cur, total, tmax)
                                     : blur_row_fixed<2, BPR>(Av, cur, total, tmax);
    if (lane < BPR) wipe[t * BPR + lane] = (uint8_t)((wipes >> lane) & 1);
  }
}

// CHUNKED: rows of 33 .. 112 blocks (blur_row_ro + blur_row_state); otherwise the fixed
// row lengths 12 .. 32 and the generic sliding window.  Separate kernels keep
// the chunked path's scalar registers free of the fixed rows' pressure.
template <bool CHUNKED>
__global__ void __launch_bounds__(64) k_blur_resolve_w(BlurGeom g, uint8_t* scratch,
                                                       int64_t sstride) {
  const int s = blockIdx.x;
  const uint32_t* counts = (const uint32_t*)(scratch + s * sstride);
  uint8_t* wipe = scratch + s * sstride + (size_t)g.nrect * 4;
  const int lane = threadIdx.x;
  const int32_t bpr = g.bpr;
  const uint32_t total = (uint32_t)(g.sw * g.sh);
  // blurfilter_cpu's set-up (A zero where the reference reads uninitialised
  // stack, as the other resolver): cur[0], cur[bpr], next[0], next[bpr], then
  // cur[1 .. bpr] = the first row's counts (A[2] and A[bpr + 1] overwritten)
  // entries l (and 64 + l, for rows past 56 blocks) of A in lane l
  auto a_init = [&](int32_t j) -> uint32_t {
    uint32_t v = 0;
    if (j == 1 || j == bpr + 1 || j == 2 || j == bpr + 2) v = total;
    if (j >= 2 && j < 2 + bpr) v = counts[j - 2];
    return v;
  };
  uint32_t Av = a_init(lane);
  // the largest max that is wiped (-1: none)
  auto wiped = [&](uint32_t m) { return ((float)m) / (float)(uint64_t)total <= g.intensity; };
  int32_t tmax = -1;
  if (wiped(0u)) {
    uint32_t lo = 0, hi = total;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo + 1) / 2;
      if (wiped(mid)) lo = mid;
      else hi = mid - 1;
    }
    tmax = (int32_t)lo;
  }
  tmax = __builtin_amdgcn_readfirstlane(tmax);
  // row lengths of 150-400 dpi pages at the default 100-pixel blocks
  if (!CHUNKED) switch (bpr) {
#define UPH_BLUR_FIXED(n) \
  case n:                 \
    blur_rows_fixed<n>(Av, counts, wipe, g.T, total, tmax); \
    return;
    UPH_BLUR_FIXED(12) UPH_BLUR_FIXED(13) UPH_BLUR_FIXED(14) UPH_BLUR_FIXED(15)
    UPH_BLUR_FIXED(16) UPH_BLUR_FIXED(17) UPH_BLUR_FIXED(18) UPH_BLUR_FIXED(19)
    UPH_BLUR_FIXED(20) UPH_BLUR_FIXED(21) UPH_BLUR_FIXED(22) UPH_BLUR_FIXED(23)
    UPH_BLUR_FIXED(24) UPH_BLUR_FIXED(25) UPH_BLUR_FIXED(26) UPH_BLUR_FIXED(27)
    UPH_BLUR_FIXED(28) UPH_BLUR_FIXED(29) UPH_BLUR_FIXED(30) UPH_BLUR_FIXED(31)
    UPH_BLUR_FIXED(32)
#undef UPH_BLUR_FIXED
    default:
      break;
  }
  // the next row's counts one row ahead (entries l and 64 + l in lane l)
  const int32_t rl = bpr + 1;
  Lanes2 A2{Av, a_init(64 + lane)};
  auto row_of = [&](int32_t t) {
    const int64_t r0 = bpr + (int64_t)t * rl;
    return Lanes2{lane < rl ? counts[r0 + lane] : 0u, 64 + lane < rl ? counts[r0 + 64 + lane] : 0u};
  };
  Lanes2 rowv = g.T > 0 ? row_of(0) : Lanes2{0u, 0u};
  for (int32_t t = 0; t < g.T; t++) {
    const Lanes2 cur = rowv;
    if (t + 1 < g.T) rowv = row_of(t + 1);
    const int op = t % 3;
    uint64_t wipes[2];
    if (CHUNKED) {
      if (op == 0) {
        blur_row_ro<0>(A2, cur, bpr, total, tmax, wipes);
        A2 = blur_row_state<0>(A2, cur, bpr, total, wipes);
      } else if (op == 1) {
        blur_row_ro<1>(A2, cur, bpr, total, tmax, wipes);
        A2 = blur_row_state<1>(A2, cur, bpr, total, wipes);
      } else {
        blur_row_ro<2>(A2, cur, bpr, total, tmax, wipes);
        A2 = blur_row_state<2>(A2, cur, bpr, total, wipes);
      }
    } else if (op == 0) {
      blur_row<0>(A2, cur, bpr, total, tmax, wipes);
    } else if (op == 1) {
      blur_row<1>(A2, cur, bpr, total, tmax, wipes);
    } else {
      blur_row<2>(A2, cur, bpr, total, tmax, wipes);
    }
    if (lane < bpr) wipe[t * bpr + lane] = (uint8_t)((wipes[0] >> lane) & 1);
    if (64 + lane < bpr) wipe[t * bpr + 64 + lane] = (uint8_t)((wipes[1] >> lane) & 1);
  }
}

template <int FMT>
__global__ void __launch_bounds__(256) k_blur_wipe(PlaneRef img, BlurGeom g, uint8_t* scratch,
                                                   int64_t sstride) {
  const int s = blockIdx.y;
  const int32_t b = blockIdx.x;  // t*bpr + j
  const uint8_t* wipe = scratch + s * sstride + (size_t)g.nrect * 4;
  if (!wipe[b]) return;
  const int32_t t = b / g.bpr, j = b % g.bpr;
  const Rect r = clip(rect_from_size(j * g.sw, t * g.sh, g.sw, g.sh), g.W, g.H);
  uint8_t* base = plane_ptr(img, s);
  const int32_t w = r.x1 - r.x0 + 1;
  if (w <= 0 || r.y1 < r.y0) return;
  const int32_t n = w * (r.y1 - r.y0 + 1);
  for (int32_t i = threadIdx.x; i < n; i += 256) {
    const int32_t yy = r.y0 + i / w, xx = r.x0 + i % w;
    white_px<FMT>(base + (int64_t)yy * img.P.pitch, xx);
  }
}

template <int FMT>
static void launch_blur_t(const PlaneRef& img, const BlurGeom& g, uint8_t* scr, int64_t ss,
                          int count, hipStream_t st, const uint32_t* bbits, int64_t bb_stride) {
  const auto a16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  const bool v16 = img.P.pitch % 16 == 0 && img.P.stride % 16 == 0 && img.P.pitch >= ((g.W + 15) & ~15) &&
                   a16(img.P.base[0]) && a16(img.P.base[1]);
  switch (blur_counts_arm(g, FMT, bbits != nullptr, v16)) {
    case BLUR_COUNTS_BITS:  // blur_bits_usable
      UPH_LAUNCH_DIAG(64, k_blur_counts_bits, dim3(1 + g.T, count), dim3(256),
                      4 * (size_t)(g.bpr + 2), st, g, bbits, bb_stride, scr, ss);
      break;
    case BLUR_COUNTS_GRAY_V16:
      UPH_LAUNCH_DIAG(64, k_blur_counts_g<true>, dim3(1 + g.T, count), dim3(256),
                      2 * (size_t)((g.W + 3) & ~3), st, img, g, scr, ss);
      break;
    case BLUR_COUNTS_GRAY:
      UPH_LAUNCH_DIAG(64, k_blur_counts_g<false>, dim3(1 + g.T, count), dim3(256),
                      2 * (size_t)((g.W + 3) & ~3), st, img, g, scr, ss);
      break;
    case BLUR_COUNTS_GENERIC:
      hipLaunchKernelGGL(k_blur_counts<FMT>, dim3(g.nrect, count), dim3(256), 0, st, img, g, scr, ss);
      break;
    case BLUR_COUNTS_NONE: break;
  }
  const BlurResolveArm resolve = blur_resolve_arm(g);
  if (diag_skip() & 8) {
  } else if (resolve == BLUR_RESOLVE_WAVE_CHUNKED) {
    hipLaunchKernelGGL(k_blur_resolve_w<true>, dim3(count), dim3(64), 0, st, g, scr, ss);
  } else if (resolve == BLUR_RESOLVE_WAVE) {
    hipLaunchKernelGGL(k_blur_resolve_w<false>, dim3(count), dim3(64), 0, st, g, scr, ss);
  } else if (resolve == BLUR_RESOLVE_GENERIC) {
    hipLaunchKernelGGL(k_blur_resolve<true>, dim3(count), dim3(256), blur_resolve_lds(g), st, g, scr,
                       ss);
  } else {
    hipLaunchKernelGGL(k_blur_resolve<false>, dim3(count), dim3(256), 0, st, g, scr, ss);
  }
  if (g.T * g.bpr > 0)
    hipLaunchKernelGGL(k_blur_wipe<FMT>, dim3(g.T * g.bpr, count), dim3(256), 0, st, img, g, scr,
                       ss);
}

bool blur_bits_usable(const BlurGeom& g, int fmt) {
  return fmt == F_GRAY8 && g.white < 255 && g.nrect > 0 && g.sw >= 32 && g.W <= (1 << 16);
}

void launch_blurfilter(const PlaneRef& img, const BlurGeom& g, void* scratch,
                       int64_t scratch_stride, int count, hipStream_t st, const SheetBits& bits) {
  uint8_t* scr = (uint8_t*)scratch;
  const uint32_t* bbits = blur_bits_usable(g, img.P.fmt) ? bits.bbits : nullptr;
  switch (img.P.fmt) {
    case F_GRAY8:
      launch_blur_t<F_GRAY8>(img, g, scr, scratch_stride, count, st, bbits, bits.stride);
      break;
    case F_Y400A:
      launch_blur_t<F_Y400A>(img, g, scr, scratch_stride, count, st, nullptr, 0);
      break;
    default: launch_blur_t<F_RGB24>(img, g, scr, scratch_stride, count, st, nullptr, 0); break;
  }
}

}  // namespace uph
